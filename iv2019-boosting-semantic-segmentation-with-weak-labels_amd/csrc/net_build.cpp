// Graph construction: the layer table in TF variable-creation order, the flat parameter layout,
// the all-reduce buckets and streams, and every allocation of a context (seg_create).
#include "net.h"

namespace segnet {
namespace {

// ------------------------------------------------------------------------------------------
// architecture (slim resnet_v1 / stack_blocks_dense; reference models/* — see oracle/tfseg)
// ------------------------------------------------------------------------------------------
int add_conv(seg_ctx* c, const std::string& name, int ci, int co, int k, int stride, int rate,
             bool explicit_pad, bool relu) {
  ConvL L;
  L.name = name; L.ci = ci; L.co = co; L.k = k; L.stride = stride; L.rate = rate;
  L.explicit_pad = explicit_pad; L.relu = relu;
  c->convs.push_back(L);
  return (int)c->convs.size() - 1;
}

struct UnitSpec { std::string scope; int din, d, dbn, s, r; };

std::vector<UnitSpec> resnet_units(int depth, int output_stride) {
  const int n3 = depth == 101 ? 23 : 6;
  struct B { const char* n; int base, units, stride; } blocks[4] = {
      {"block1", 64, 3, 2}, {"block2", 128, 4, 2}, {"block3", 256, n3, 2}, {"block4", 512, 3, 1}};
  const int target = output_stride / 4;
  int current = 1, rate = 1, din = 64;
  std::vector<UnitSpec> out;
  for (auto& b : blocks) {
    for (int i = 0; i < b.units; ++i) {
      int us = i == b.units - 1 ? b.stride : 1;
      std::string scope = std::string(b.n) + "/unit_" + std::to_string(i + 1) + "/bottleneck_v1";
      if (current == target) {
        out.push_back({scope, din, b.base * 4, b.base, 1, rate});
        rate *= us;
      } else {
        out.push_back({scope, din, b.base * 4, b.base, us, 1});
        current *= us;
      }
      din = b.base * 4;
    }
  }
  return out;
}

void add_bottleneck(seg_ctx* c, Unit& u, const std::string& scope, int din, int d, int dbn, int s,
                    int r) {
  if (d != din) {
    u.sc = add_conv(c, scope + "/shortcut", din, d, 1, s, 1, false, false);
    u.kind = SC_CONV;
  } else {
    u.kind = s > 1 ? SC_SUBSAMPLE : SC_IDENTITY;
  }
  u.stride = s;
  u.c1 = add_conv(c, scope + "/conv1", din, dbn, 1, 1, 1, false, true);
  u.c2 = add_conv(c, scope + "/conv2", dbn, dbn, 3, s, r, s > 1, true);
  u.c3 = add_conv(c, scope + "/conv3", dbn, d, 1, 1, 1, false, false);
}

void fill_tables(LossTables& t, int dataset) {
  memset(&t, 0, sizeof(t));
  if (dataset == SEG_DATASET_VISTAS) {
    // define_losses_hierarchical.py:37-74; hierarchical.py:146-156
    t.c1 = 53; t.c2 = 12; t.c3 = 5; t.n_pp = 66; t.n_pb = 15;
    t.cid_l1_vehicle = 49; t.cid_l1_human = 19; t.l1_wmax = 51;
    const int pp2l1[66] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19,
                           19, 19, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34,
                           35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 49, 49, 49,
                           49, 49, 49, 49, 49, 49, 49, 50, 51, 52};
    const int pb2l1[15] = {49, 49, 49, 49, 49, 49, 19, 19, 19, 19, 19, 52, 52, 52, 52};
    (void)pb2l1;
    int pp2veh[66], pp2hum[66];
    for (int i = 0; i < 66; ++i) { pp2veh[i] = 11; pp2hum[i] = 4; }
    for (int i = 0; i < 11; ++i) pp2veh[52 + i] = i;
    pp2hum[19] = 0; pp2hum[20] = 1; pp2hum[21] = 2; pp2hum[22] = 3;
    const int pb2veh[15] = {0, 2, 3, 5, 6, 9, 11, 11, 11, 11, 11, 11, 11, 11, 11};
    const int pb2hum[15] = {4, 4, 4, 4, 4, 4, 0, 0, 0, 0, 0, 4, 4, 4, 4};
    for (int i = 0; i < 66; ++i) { t.pp2l1[i] = pp2l1[i]; t.pp2veh[i] = pp2veh[i]; t.pp2hum[i] = pp2hum[i]; }
    for (int i = 0; i < 15; ++i) { t.pb2veh[i] = pb2veh[i]; t.pb2hum[i] = pb2hum[i]; }
    for (int i = 0; i < 20; ++i) t.l1_to_common[i] = i;
    for (int i = 20; i < 50; ++i) t.l1_to_common[i] = i + 3;
    t.l1_to_common[50] = 63; t.l1_to_common[51] = 64; t.l1_to_common[52] = 65;
    for (int i = 0; i < 11; ++i) t.veh_to_common[i] = 52 + i;
    t.veh_to_common[11] = 65;
    const int h2c[5] = {19, 20, 21, 22, 65};
    for (int i = 0; i < 5; ++i) t.hum_to_common[i] = h2c[i];
  } else {
    // define_losses_hierarchical.py:75-93; hierarchical.py:157-162
    t.c1 = 14; t.c2 = 7; t.c3 = 3; t.n_pp = 20; t.n_pb = 15;
    t.cid_l1_vehicle = 12; t.cid_l1_human = 11; t.l1_wmax = 12;
    const int pp2l1[20] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 11, 12, 12, 12, 12, 12, 12, 13};
    const int pp2veh[20] = {6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 0, 1, 2, 3, 4, 5, 6};
    const int pp2hum[20] = {2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 0, 1, 2, 2, 2, 2, 2, 2, 2};
    const int pb2veh[15] = {5, 2, 0, 4, 3, 1, 6, 6, 6, 6, 6, 6, 6, 6, 6};
    const int pb2hum[15] = {2, 2, 2, 2, 2, 2, 0, 0, 0, 0, 0, 2, 2, 2, 2};
    for (int i = 0; i < 20; ++i) { t.pp2l1[i] = pp2l1[i]; t.pp2veh[i] = pp2veh[i]; t.pp2hum[i] = pp2hum[i]; }
    for (int i = 0; i < 15; ++i) { t.pb2veh[i] = pb2veh[i]; t.pb2hum[i] = pb2hum[i]; }
    const int l1c[14] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 19};
    const int vc[7] = {13, 14, 15, 16, 17, 18, 19};
    const int hc[3] = {11, 12, 19};
    for (int i = 0; i < 14; ++i) t.l1_to_common[i] = l1c[i];
    for (int i = 0; i < 7; ++i) t.veh_to_common[i] = vc[i];
    for (int i = 0; i < 3; ++i) t.hum_to_common[i] = hc[i];
  }
}

// TF ResizeBilinear(align_corners=True) legacy index/lerp (float arithmetic)
void tf_lerp_host(int o, int n_in, int n_out, int& lo, int& hi, float& l) {
  float scale = n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f;
  float fin = (float)o * scale;
  lo = (int)fin;
  hi = std::min(lo + 1, n_in - 1);
  l = fin - (float)lo;
}

// ReLU-output activation with its bit mask (C % 8 == 0)
int alloc_relu_act(seg_ctx* c, Act& a, int N, int H, int W, int C, int ld = 0) {
  if (int r = alloc_act(c, a, N, H, W, C, ld)) return r;
  if (C % 8) return 0;
  return dalloc(c, &a.mask, (size_t)a.M() * (C / 8));
}

int alloc_conv(seg_ctx* c, ConvL& L, int N, int H, int W, int ldy = 0) {
  conv_geom(L, N, H, W);
  L.co_pad = (L.co % 8) ? ((L.co + 15) / 16) * 16 : L.co;
  int ld = ldy ? ldy : L.co_pad;
  if (int r = alloc_act(c, L.y, N, L.Ho, L.Wo, L.co, ld)) return r;
  if (int r = alloc_act(c, L.dy, N, L.Ho, L.Wo, L.co, ld)) return r;
  float* v;
  if (int r = dalloc(c, &v, (size_t)6 * L.co)) return r;
  L.st.mean = v; L.st.invstd = v + L.co; L.st.scale = v + 2 * L.co; L.st.var_unb = v + 3 * L.co;
  L.st.sdy = v + 4 * L.co; L.st.sdyx = v + 5 * L.co;
  long M = (long)N * L.Ho * L.Wo;
  if (int r = dalloc(c, &L.stats_part, (size_t)conv_nt_mtiles(M) * L.co * 2)) return r;
  if (c->gn) {
    const long hw = (long)L.Ho * L.Wo;
    L.rb = bn_bwd_rowblocks(hw);
    if (int r = dalloc(c, &L.bwd_part, (size_t)N * L.rb * L.co * 2)) return r;
    if (int r = dalloc(c, &L.gn_part, (size_t)N * gn_chunks(hw) * L.co * 2)) return r;
    float* sv;
    if (int r = dalloc(c, &sv, (size_t)N * 6 * L.co)) return r;
    L.st_img.resize(N);
    for (int n = 0; n < N; ++n) {
      float* b = sv + (size_t)n * 6 * L.co;
      L.st_img[n] = BnState{b, b + L.co, b + 2 * L.co, b + 3 * L.co, b + 4 * L.co, b + 5 * L.co};
    }
    if (int r = dalloc(c, &L.st_dev, (size_t)N)) return r;
    HIPCALL(c, hipMemcpy(L.st_dev, L.st_img.data(), N * sizeof(BnState), hipMemcpyHostToDevice));
  } else {
    L.rb = bn_bwd_rowblocks(M);
    if (int r = dalloc(c, &L.bwd_part, (size_t)L.rb * L.co * 2)) return r;
  }
  return 0;
}

int alloc_unit(seg_ctx* c, Unit& u, const Act& in) {
  u.in = in;
  if (u.sc >= 0)
    if (int r = alloc_conv(c, c->convs[u.sc], in.N, in.H, in.W)) return r;
  ConvL& c1 = c->convs[u.c1];
  if (int r = alloc_conv(c, c1, in.N, in.H, in.W)) return r;
  if (int r = alloc_relu_act(c, u.z1, in.N, c1.Ho, c1.Wo, c1.co)) return r;
  if (int r = alloc_act(c, u.dz1, in.N, c1.Ho, c1.Wo, c1.co)) return r;
  ConvL& c2 = c->convs[u.c2];
  if (int r = alloc_conv(c, c2, in.N, c1.Ho, c1.Wo)) return r;
  if (int r = alloc_relu_act(c, u.z2, in.N, c2.Ho, c2.Wo, c2.co)) return r;
  if (int r = alloc_act(c, u.dz2, in.N, c2.Ho, c2.Wo, c2.co)) return r;
  ConvL& c3 = c->convs[u.c3];
  if (int r = alloc_conv(c, c3, in.N, c2.Ho, c2.Wo)) return r;
  if (int r = alloc_relu_act(c, u.out, in.N, c3.Ho, c3.Wo, c3.co)) return r;
  if (int r = alloc_act(c, u.dout, in.N, c3.Ho, c3.Wo, c3.co)) return r;
  if (u.kind != SC_CONV)
    if (int r = alloc_act(c, u.dpre, in.N, c3.Ho, c3.Wo, c3.co)) return r;
  return 0;
}

// ------------------------------------------------------------------------------------------
// pyramid tables
// ------------------------------------------------------------------------------------------
int upload_grid(seg_ctx* c, GridSpec& g, const std::vector<float>& rt, const std::vector<float>& ct) {
  float *drt, *dct;
  if (int r = dalloc(c, &drt, rt.size())) return r;
  if (int r = dalloc(c, &dct, ct.size())) return r;
  HIPCALL(c, hipMemcpy(drt, rt.data(), rt.size() * 4, hipMemcpyHostToDevice));
  HIPCALL(c, hipMemcpy(dct, ct.data(), ct.size() * 4, hipMemcpyHostToDevice));
  g.rowtab = drt;
  g.coltab = dct;
  return 0;
}

// VALID avg pools with (kh, kw) windows over an (H, W) map (remainders dropped)
int make_pool_grids(seg_ctx* c, GridSpec& g, int H, int W, const std::vector<std::pair<int, int>>& win) {
  memset(&g, 0, sizeof(g));
  g.n = (int)win.size();
  for (int i = 0; i < g.n; ++i) {
    if (win[i].first < 1 || win[i].second < 1)   // PSP: dims // 6 of a map under 6 x 6
      return set_err(&c->err, -EINVAL, "the %d x %d feature map is too small for the pyramid's "
                     "pooling grids (PSP needs at least 6 x 6: an input of 48 x 48)", H, W);
    g.kh[i] = win[i].first; g.kw[i] = win[i].second;
    g.kr[i] = (H - g.kh[i]) / g.kh[i] + 1;
    g.kc[i] = (W - g.kw[i]) / g.kw[i] + 1;
    g.ccell_off[i] = g.total_ccells; g.total_ccells += g.kc[i];
    g.rcell_off[i] = g.total_rcells; g.total_rcells += g.kr[i];
    g.scale[i] = 1.f / (float)(g.kh[i] * g.kw[i]);
  }
  if (g.total_ccells > SEG_MAX_CELLS) return set_err(&c->err, -EINVAL, "too many pyramid cells");
  std::vector<float> rt((size_t)g.total_ccells * W, 0.f), ct((size_t)g.total_rcells * H, 0.f);
  for (int i = 0; i < g.n; ++i) {
    for (int j = 0; j < g.kc[i]; ++j)
      for (int w = j * g.kw[i]; w < (j + 1) * g.kw[i]; ++w) rt[(size_t)(g.ccell_off[i] + j) * W + w] = 1.f;
    for (int r = 0; r < g.kr[i]; ++r)
      for (int h = r * g.kh[i]; h < (r + 1) * g.kh[i]; ++h) ct[(size_t)(g.rcell_off[i] + r) * H + h] = 1.f;
  }
  return upload_grid(c, g, rt, ct);
}

// transpose of an align-corners resize (kr, kc) -> (H, W)
int make_resize_grid(seg_ctx* c, GridSpec& g, int kr, int kc, int H, int W) {
  memset(&g, 0, sizeof(g));
  g.n = 1; g.kr[0] = kr; g.kc[0] = kc; g.total_ccells = kc; g.total_rcells = kr; g.scale[0] = 1.f;
  std::vector<float> rt((size_t)kc * W, 0.f), ct((size_t)kr * H, 0.f);
  for (int w = 0; w < W; ++w) {
    int lo, hi; float l;
    tf_lerp_host(w, kc, W, lo, hi, l);
    rt[(size_t)lo * W + w] += 1.f - l;
    rt[(size_t)hi * W + w] += l;
  }
  for (int h = 0; h < H; ++h) {
    int lo, hi; float l;
    tf_lerp_host(h, kr, H, lo, hi, l);
    ct[(size_t)lo * H + h] += 1.f - l;
    ct[(size_t)hi * H + h] += l;
  }
  return upload_grid(c, g, rt, ct);
}

// one pooled pyramid branch over a (kr, kc) grid of the (Hf, Wf) map: the pooled input, the
// BN + ReLU output and their gradients, the branch's conv and its resize-transpose grid
int alloc_pool_branch(seg_ctx* c, int conv, int N, int kr, int kc, int Hf, int Wf) {
  const int fd = c->cfg.feature_dims;
  Act pa, dpa, za, dza;
  if (int r = alloc_act(c, pa, N, kr, kc, fd)) return r;
  if (int r = alloc_act(c, dpa, N, kr, kc, fd)) return r;
  if (int r = alloc_act(c, za, N, kr, kc, fd)) return r;
  if (int r = alloc_act(c, dza, N, kr, kc, fd)) return r;
  c->pooled.push_back(pa); c->dpooled.push_back(dpa); c->zb.push_back(za); c->dzb.push_back(dza);
  if (int r = alloc_conv(c, c->convs[conv], N, kr, kc)) return r;
  GridSpec ug;
  if (int r = make_resize_grid(c, ug, kr, kc, Hf, Wf)) return r;
  c->up_grids.push_back(ug);
  return 0;
}

// ------------------------------------------------------------------------------------------
// build(), step by step
// ------------------------------------------------------------------------------------------
// the layers in TF variable-creation order
int build_layers(seg_ctx* c) {
  const seg_cfg& g = c->cfg;
  const int fd = g.feature_dims;
  const std::string rn = "feature_extractor/base/resnet_v1_" + std::to_string(g.depth);
  c->stem = add_conv(c, rn + "/conv1", 3, 64, 7, 2, 1, true, true);
  for (auto& us : resnet_units(g.depth, g.output_stride)) {
    Unit u;
    add_bottleneck(c, u, rn + "/" + us.scope, us.din, us.d, us.dbn, us.s, us.r);
    c->units.push_back(u);
  }
  c->dfd = add_conv(c, "feature_extractor/extension/decrease_fdims", 2048, fd, 1, 1, 1, false, true);
  if (g.fov_k < 0 || g.fov_rate < 0 || (g.fov_k > 0) != (g.fov_rate > 0))
    return set_err(&c->err, -EINVAL, "fov_k and fov_rate must both be set (hierarchical.py:272-274)");
  if (g.fov_k > 0)   // slim.conv2d(fe, fd, fov_k, rate=fov_rate): SAME, BN, ReLU
    c->fov = add_conv(c, "feature_extractor/extension/increase_fov", fd, fd, g.fov_k, 1, g.fov_rate,
                      false, true);
  if (g.pyramid == SEG_PYRAMID_PSP) {
    const char* nm[4] = {"Conv", "Conv_1", "Conv_2", "Conv_3"};
    for (int i = 0; i < 4; ++i)
      c->pyr_conv.push_back(add_conv(c, std::string("feature_extractor/pyramid_module/") + nm[i], fd, fd, 1, 1, 1, false, true));
    c->pyr_final = add_conv(c, "feature_extractor/pyramid_module/Conv_4", 5 * fd, fd, 1, 1, 1, false, true);
  } else if (g.pyramid == SEG_PYRAMID_ASPP) {
    // the commented _create_aspp_module (hierarchical.py:209-226), in the PSP call site's scope
    const std::string sc = "feature_extractor/pyramid_module/";
    c->pyr_conv.push_back(add_conv(c, sc + "Conv", fd, fd, 1, 1, 1, false, true));     // image pool
    c->pyr_conv.push_back(add_conv(c, sc + "Conv_1", fd, fd, 1, 1, 1, false, true));   // 1x1
    const int rates[3] = {6, 12, 18};
    for (int i = 0; i < 3; ++i)
      c->pyr_conv.push_back(add_conv(c, sc + "Conv_" + std::to_string(i + 2), fd, fd, 3, 1, rates[i], false, true));
    c->pyr_final = add_conv(c, sc + "Conv_5", 5 * fd, fd, 1, 1, 1, false, true);
  }
  const char* hn[3] = {"l1", "l2_vehicle", "l2_human"};
  for (int h = 0; h < 3; ++h)
    add_bottleneck(c, c->heads[h], std::string("adaptation_module/") + hn[h] + "_features", fd, fd, fd, 1, 1);
  fill_tables(c->tables, g.dataset);
  c->nc[0] = c->tables.c1; c->nc[1] = c->tables.c2; c->nc[2] = c->tables.c3;
  for (int h = 0; h < 3; ++h)
    c->logit_conv[h] = add_conv(c, std::string("softmax_classifier/") + hn[h] + "_logits", fd, c->nc[h], 1, 1, 1, false, false);
  c->convs[c->stem].need_dgrad = false;

  if (g.upsampling != SEG_UPSAMPLING_BILINEAR && g.upsampling != SEG_UPSAMPLING_HYBRID)
    return set_err(&c->err, -EINVAL, "upsampling must be bilinear or hybrid");
  c->hybrid = g.upsampling == SEG_UPSAMPLING_HYBRID;
  if (g.norm != SEG_NORM_BATCH && g.norm != SEG_NORM_GROUP)
    return set_err(&c->err, -EINVAL, "norm must be batch or group");
  c->gn = g.norm == SEG_NORM_GROUP;
  if (c->gn) {   // module_arg_scope groups (32), the softmax_classifier scope's groups=1
    const int G = g.groups > 0 ? g.groups : 32;
    for (auto& L : c->convs) {
      const bool logit = &L == &c->convs[c->logit_conv[0]] || &L == &c->convs[c->logit_conv[1]] ||
                         &L == &c->convs[c->logit_conv[2]];
      L.groups = logit ? 1 : G;
      if (L.co % L.groups || L.co / L.groups > 256)
        return set_err(&c->err, -EINVAL, "group norm: %s has %d channels for %d groups", L.name.c_str(),
                       L.co, L.groups);
    }
  }
  return 0;
}

// the flat parameter layout:
// [conv weights | hybrid deconv weights] (weight decay) [BN gamma/beta | deconv biases]
void build_param_layout(seg_ctx* c) {
  long off = 0;
  for (auto& L : c->convs) { L.w_off = off; off += (long)L.co * L.k * L.k * L.ci; }
  if (c->hybrid)
    for (int h = 0; h < 3; ++h) { c->dc_w_off[h] = off; off += 9L * c->nc[h] * c->nc[h]; }
  c->n_decay = off;
  for (auto& L : c->convs) { L.g_off = off; off += L.co; L.b_off = off; off += L.co; }
  c->dc_b_lo = off;
  if (c->hybrid)
    for (int h = 0; h < 3; ++h) { c->dc_b_off[h] = off; off += c->nc[h]; }
  c->n_train = off;
  long moff = 0;
  for (auto& L : c->convs) { L.mv_off = moff; moff += L.co; }
  c->n_moving = 2 * moff;
  c->n_stats = c->n_moving;
}

int build_buckets_and_streams(seg_ctx* c) {
  // runtime knob (deliberate): the all-reduce bucket size, a property of the interconnect
  // rather than of the kernels (seg_grad_buckets); results are identical for any value
  const char* e = getenv("SEG_BUCKET_MB");
  const long cap = (e ? std::max(1L, atol(e)) : 32L) * (1L << 20) / 4;   // floats per bucket
  long hi = c->n_decay;
  std::vector<int> cur;
  for (int li = (int)c->convs.size() - 1; li >= 0; --li) {
    cur.push_back(li);
    const long lo = c->convs[li].w_off;
    if (hi - lo >= cap || li == 0) {
      c->bk_lo.push_back(lo); c->bk_hi.push_back(hi); c->bk_convs.push_back(cur);
      cur.clear();
      hi = lo;
    }
  }
  c->bk_lo.push_back(c->n_decay); c->bk_hi.push_back(c->n_train + c->n_stats);
  c->bk_ev.resize(c->bk_lo.size());
  for (auto& ev : c->bk_ev) HIPCALL(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  c->wg_done.assign(c->convs.size(), 0);
  // runtime knob (deliberate): SEG_SIDE_STREAM=0 runs the backward on one stream, so a
  // rocprofv3 trace sees kernel-alone durations (tools/session.sh stats, pmc_traffic.sh);
  // results are bitwise identical either way
  const char* se = getenv("SEG_SIDE_STREAM");
  c->side_on = !(se && se[0] == '0');
  if (c->side_on) {
    HIPCALL(c, hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
    c->ev_dy.resize(c->convs.size());
    for (auto& ev : c->ev_dy) HIPCALL(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIPCALL(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    HIPCALL(c, hipEventCreateWithFlags(&c->ev_prestem, hipEventDisableTiming));
  }
  return 0;
}

void build_param_info(seg_ctx* c) {
  const long moff = c->n_moving / 2;
  for (auto& L : c->convs) {
    c->pinfo.push_back({L.name + "/weights", L.w_off, (long)L.co * L.k * L.k * L.ci, SEG_PARAM_WEIGHTS, {L.co, L.k, L.k, L.ci}});
    if (c->gn) {   // tf.contrib.layers.group_norm variables: no moving statistics
      c->pinfo.push_back({L.name + "/GroupNorm/beta", L.b_off, L.co, SEG_PARAM_BETA, {L.co, 1, 1, 1}});
      c->pinfo.push_back({L.name + "/GroupNorm/gamma", L.g_off, L.co, SEG_PARAM_GAMMA, {L.co, 1, 1, 1}});
      continue;
    }
    c->pinfo.push_back({L.name + "/BatchNorm/beta", L.b_off, L.co, SEG_PARAM_BETA, {L.co, 1, 1, 1}});
    c->pinfo.push_back({L.name + "/BatchNorm/gamma", L.g_off, L.co, SEG_PARAM_GAMMA, {L.co, 1, 1, 1}});
    c->pinfo.push_back({L.name + "/BatchNorm/moving_mean", L.mv_off, L.co, SEG_PARAM_MOVING_MEAN, {L.co, 1, 1, 1}});
    c->pinfo.push_back({L.name + "/BatchNorm/moving_variance", moff + L.mv_off, L.co, SEG_PARAM_MOVING_VAR, {L.co, 1, 1, 1}});
  }
  if (c->hybrid) {
    // slim.conv2d_transpose default scopes inside softmax_classifier/upsampling, created after
    // the three logits convs (hierarchical.py:84-86,168-180)
    const char* sfx[3] = {"", "_1", "_2"};
    for (int h = 0; h < 3; ++h) {
      const std::string nm = std::string("softmax_classifier/upsampling/Conv2d_transpose") + sfx[h];
      const int C = c->nc[h];
      c->pinfo.push_back({nm + "/weights", c->dc_w_off[h], 9L * C * C, SEG_PARAM_WEIGHTS, {C, 3, 3, C}});
      c->pinfo.push_back({nm + "/biases", c->dc_b_off[h], C, SEG_PARAM_BIASES, {C, 1, 1, 1}});
    }
  }
}

// the pyramid module over the (Hf, Wf) extension output and the final conv's output feat
int build_pyramid(seg_ctx* c, int N, int Hf, int Wf) {
  const seg_cfg& g = c->cfg;
  const int fd = g.feature_dims;
  if (g.pyramid != SEG_PYRAMID_PSP && g.pyramid != SEG_PYRAMID_ASPP) {
    if (int r = alloc_relu_act(c, c->z_dfd, N, Hf, Wf, fd)) return r;
    c->feat = c->z_dfd;
    c->dfeat = c->dz_dfd;
    return 0;
  }
  if (g.pyramid == SEG_PYRAMID_ASPP)
    if (int r = alloc_relu_act(c, c->z_dfd, N, Hf, Wf, fd)) return r;
  if (int r = alloc_act(c, c->concat, N, Hf, Wf, 5 * fd)) return r;
  if (int r = alloc_act(c, c->dconcat, N, Hf, Wf, 5 * fd)) return r;
  if (g.pyramid == SEG_PYRAMID_PSP) {
    c->z_dfd = slice(c, c->concat, 0, fd);
    // _create_psp_module: spatial dims = (hf, wf) // stride; kernel = stride = dims // k
    const int sh = g.height / g.output_stride, sw = g.width / g.output_stride;
    std::vector<std::pair<int, int>> win;
    for (int k : {1, 2, 3, 6}) win.push_back({sh / k, sw / k});
    if (int r = make_pool_grids(c, c->pool_grids, Hf, Wf, win)) return r;
    size_t gp = (size_t)N * Hf * c->pool_grids.total_ccells * fd;
    for (int b = 0; b < 4; ++b) {
      const int kr = c->pool_grids.kr[b], kc = c->pool_grids.kc[b];
      if (int r = alloc_pool_branch(c, c->pyr_conv[b], N, kr, kc, Hf, Wf)) return r;
      gp = std::max(gp, (size_t)N * Hf * kc * fd);
    }
    if (int r = dalloc(c, &c->grid_part, gp)) return r;
  } else {
    std::vector<std::pair<int, int>> win{{Hf, Wf}};   // global average pool
    if (int r = make_pool_grids(c, c->pool_grids, Hf, Wf, win)) return r;
    if (int r = alloc_pool_branch(c, c->pyr_conv[0], N, 1, 1, Hf, Wf)) return r;
    if (int r = dalloc(c, &c->grid_part, (size_t)N * Hf * fd)) return r;
    for (int b = 1; b < 5; ++b)
      if (int r = alloc_conv(c, c->convs[c->pyr_conv[b]], N, Hf, Wf)) return r;
  }
  if (int r = alloc_conv(c, c->convs[c->pyr_final], N, Hf, Wf)) return r;
  if (int r = alloc_relu_act(c, c->feat, N, Hf, Wf, fd)) return r;
  return alloc_act(c, c->dfeat, N, Hf, Wf, fd);
}

int build_activations(seg_ctx* c, int N) {
  const seg_cfg& g = c->cfg;
  const int fd = g.feature_dims;
  const int H = g.height, W = g.width;
  // the stem input is context-owned in every dtype (the 16-bit space-to-depth image, or an fp32
  // copy): the stem's weight gradient reads it in seg_backward, after the caller's buffer may
  // be gone
  c->stem_s2d = seg_half(c->dt);
  ConvL& st = c->convs[c->stem];
  if (int r = alloc_conv(c, st, N, H, W)) return r;
  if (c->stem_s2d) {
    if (st.k != 7 || st.stride != 2 || st.ci != 3)
      return set_err(&c->err, -EINVAL, "space-to-depth stem expects a 7x7/2 conv of 3 channels");
    if (int r = alloc_act(c, c->img, N, st.Ho + 3, st.Wo + 3, 16)) return r;
  } else {
    if (int r = alloc_act(c, c->img, N, H, W, 3)) return r;
  }
  if (int r = alloc_relu_act(c, c->z0, N, st.Ho, st.Wo, 64)) return r;
  if (int r = alloc_act(c, c->dz0, N, st.Ho, st.Wo, 64)) return r;
  {  // max_pool2d 3x3/2 SAME
    int Ho = (st.Ho + 1) / 2, Wo = (st.Wo + 1) / 2;
    int th = std::max((Ho - 1) * 2 + 3 - st.Ho, 0), tw = std::max((Wo - 1) * 2 + 3 - st.Wo, 0);
    c->pool_ph = th / 2; c->pool_pw = tw / 2;
    if (int r = alloc_act(c, c->p0, N, Ho, Wo, 64)) return r;
    if (int r = dalloc(c, &c->pool_arg, (size_t)N * Ho * Wo * 64)) return r;
    if (int r = alloc_act(c, c->dp0, N, Ho, Wo, 64)) return r;
  }
  Act x = c->p0;
  for (auto& u : c->units) {
    if (int r = alloc_unit(c, u, x)) return r;
    x = u.out;
  }
  ConvL& dfd = c->convs[c->dfd];
  if (int r = alloc_conv(c, dfd, N, x.H, x.W)) return r;
  const int Hf = dfd.Ho, Wf = dfd.Wo;
  if (int r = alloc_act(c, c->dz_dfd, N, Hf, Wf, fd)) return r;
  if (c->fov >= 0) {
    if (int r = alloc_relu_act(c, c->z_pre, N, Hf, Wf, fd)) return r;
    if (int r = alloc_act(c, c->dz_pre, N, Hf, Wf, fd)) return r;
    if (int r = alloc_conv(c, c->convs[c->fov], N, Hf, Wf)) return r;
  }
  if (int r = build_pyramid(c, N, Hf, Wf)) return r;
  for (int h = 0; h < 3; ++h) {
    if (int r = alloc_unit(c, c->heads[h], c->feat)) return r;
    if (int r = alloc_conv(c, c->convs[c->logit_conv[h]], N, Hf, Wf)) return r;
  }
  c->ldl = ((c->nc[0] + c->nc[1] + c->nc[2] + 3) / 4) * 4;
  if (int r = alloc_act(c, c->logits, N, Hf, Wf, c->nc[0] + c->nc[1] + c->nc[2], c->ldl, 4)) return r;
  if (int r = dalloc(c, &c->grad_un, (size_t)N * Hf * Wf * c->ldl)) return r;
  c->head_in = (const float*)c->logits.p;
  if (c->gn)
    if (int r = dalloc(c, &c->gn_gscaled, (size_t)N * Hf * Wf * c->ldl)) return r;
  if (c->hybrid) {
    if (int r = dalloc(c, &c->up_in, (size_t)N * Hf * Wf * c->ldl)) return r;
    if (int r = dalloc(c, &c->dc_dx, (size_t)N * Hf * Wf * c->ldl)) return r;
    const size_t np = (size_t)deconv_wgrad_blocks(N, Hf, Wf, c->nc[0] + c->nc[1] + c->nc[2]) * deconv_nw(c->nc);
    if (int r = dalloc(c, &c->dc_part, np)) return r;
    c->head_in = c->up_in;
  }
  c->loss_blocks = loss_head_blocks(N, Hf, Wf);
  if (int r = dalloc(c, &c->loss_part, (size_t)c->loss_blocks * 8)) return r;
  if (int r = dalloc(c, &c->loss_out, 16)) return r;
  if (int r = dalloc(c, &c->dzscale, c->ldl)) return r;
  if (int r = dalloc(c, &c->reg_part, sgdm_blocks(c->n_decay) + 2)) return r;   // + the split update's
  return dalloc(c, &c->reg_out, 4);
}

// compute weight copies and workspace
int build_workspace(seg_ctx* c) {
  if (seg_half(c->dt))
    if (int r = dalloc(c, (bf16_t**)&c->w_lp_flat, c->n_decay)) return r;
  size_t slab = 0;
  for (auto& L : c->convs) {
    if (L.need_dgrad) {
      char* p;
      if (int r = dalloc(c, &p, (size_t)L.co * L.k * L.k * L.ci * c->esz)) return r;
      L.wt_lp = p;
    }
    if (seg_half(c->dt)) L.w_lp = (uint16_t*)c->w_lp_flat + L.w_off;   // bf16 or fp16 bits
    const bool s2d = &L == &c->convs[c->stem] && c->stem_s2d;
    const WgradArgs a = wgrad_problem(L, s2d);
    const int sp = std::max(wgrad_splits(a, c->dt, false), wgrad_splits(a, c->dt, true));
    slab = std::max(slab, (size_t)sp * a.Co * a.KH * a.KW * a.C);
  }
  if (c->stem_s2d) {
    const ConvL& st = c->convs[c->stem];
    if (int r = dalloc(c, &c->stem_wpad, (size_t)st.co * 256)) return r;
  }
  c->slab_floats = slab;
  return dalloc(c, &c->slab, slab);
}

// linear BN-backward fold: per-layer coefficients and the shared scratch (lbf.h)
int build_fold_scratch(seg_ctx* c) {
  size_t wts = 0, hh = 0, hs = 0, ci_max = 0;
  for (auto& u : c->units) {
    if (!lbf_shape_ok(c, u)) continue;
    ConvL& L3 = c->convs[u.c3];
    if (int r = dalloc(c, &L3.lbf_coef, 3 * (size_t)L3.co)) return r;
    // per layer: conv2's BN reduce writes it on the compute stream while the side stream may
    // still be combining an earlier unit's gradient
    if (int r = dalloc(c, &L3.lbf_cs, (size_t)c->convs[u.c2].rb * L3.ci)) return r;
    wts = std::max(wts, (size_t)L3.co * L3.ci);
    hh = std::max(hh, (size_t)L3.ci * L3.ci);
    hs = std::max(hs, (size_t)lbf_hsplits(L3) * L3.ci * L3.ci);
    ci_max = std::max(ci_max, (size_t)L3.ci);
  }
  if (!wts) return 0;
  char* p;
  if (int r = dalloc(c, &p, wts * c->esz)) return r;
  c->lbf_wts = p;
  if (int r = dalloc(c, &p, wts * c->esz)) return r;
  c->lbf_xd = p;
  if (int r = dalloc(c, &p, hh * c->esz)) return r;
  c->lbf_h = p;
  if (int r = dalloc(c, &c->lbf_hslab, hs)) return r;
  if (int r = dalloc(c, &c->lbf_bias, ci_max)) return r;
  if (int r = dalloc(c, &c->lbf_bpart, (wts / 128) + ci_max)) return r;   // [co / 128][ci]
  return dalloc(c, &c->lbf_p1, wts + hh);   // [P1 (co x ci) | G (ci x ci)]
}

}  // namespace

// geometry of a conv on an input of spatial size (H, W)
void conv_geom(ConvL& L, int N, int H, int W) {
  L.N = N; L.H = H; L.W = W;
  const int keff = L.k + (L.k - 1) * (L.rate - 1);
  if (L.explicit_pad) {  // conv2d_same, stride > 1: pad (keff-1)//2 before, rest after, VALID
    L.pad_h = L.pad_w = (keff - 1) / 2;
    L.Ho = (H + keff - 1 - keff) / L.stride + 1;
    L.Wo = (W + keff - 1 - keff) / L.stride + 1;
  } else {               // SAME (only stride 1 here): out = ceil(n/s)
    L.Ho = (H + L.stride - 1) / L.stride;
    L.Wo = (W + L.stride - 1) / L.stride;
    int tot_h = std::max((L.Ho - 1) * L.stride + keff - H, 0);
    int tot_w = std::max((L.Wo - 1) * L.stride + keff - W, 0);
    L.pad_h = tot_h / 2;
    L.pad_w = tot_w / 2;
  }
}

// linear BN-backward fold (lbf.h): the unit shapes it applies to -- a 16-bit batch-norm
// bottleneck (identity, subsample, or projection with its output gradient pre-masked) whose conv3 is an expansion 1 x 1 (co >= 2 ci, ci a multiple of 64; its data
// gradient is a ping-pong launch for ci > 128, a v2 launch otherwise: C2 = ci, Co = ci) and whose
// conv2 output gate is kept as bits
bool lbf_shape_ok(const seg_ctx* c, const Unit& u) {
  if (!seg_half(c->dt) || c->gn || u.c3 < 0 || u.c2 < 0) return false;
  const ConvL& L3 = c->convs[u.c3];
  const ConvL& L2 = c->convs[u.c2];
  return L3.k == 1 && L3.stride == 1 && L3.rate == 1 && L3.co >= 2 * L3.ci && L3.ci >= 64 &&
         L3.co <= 2048 && L3.ci % 64 == 0 && L3.co % 128 == 0 && L2.co == L3.ci && L2.relu;
}

int build(seg_ctx* c) {
  const seg_cfg& g = c->cfg;
  const int N = g.nb_pp + g.nb_pb + g.nb_pi;
  if (N <= 0 || g.height < 32 || g.width < 32) return set_err(&c->err, -EINVAL, "bad batch/size");
  if (g.depth != 50 && g.depth != 101) return set_err(&c->err, -EINVAL, "depth must be 50|101");
  if (g.output_stride != 8) return set_err(&c->err, -EINVAL, "output_stride must be 8");
  if (g.feature_dims % 8) return set_err(&c->err, -EINVAL, "feature_dims must be a multiple of 8");
  if (int r = build_layers(c)) return r;
  build_param_layout(c);
  if (int r = build_buckets_and_streams(c)) return r;
  build_param_info(c);
  if (int r = build_activations(c, N)) return r;
  if (int r = build_workspace(c)) return r;
  return build_fold_scratch(c);
}

}  // namespace segnet
