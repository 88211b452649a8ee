// Exact K-th-largest radix select on float bits (see bootstrap.h).
#include "bootstrap.h"

namespace {

constexpr int BT = 1024;              // threads of both kernels
constexpr int BINS = BOOTSTRAP_BINS;  // bins of a slab row (the 10-bit pass uses the first 1024)
constexpr int PER_THREAD = 8;         // entries per thread that size the hist grid

// digit passes, most significant first: bits [31:21], [20:10], [9:0]
template <int PASS> struct Digit {
  static constexpr int SHIFT = PASS == 0 ? 21 : PASS == 1 ? 10 : 0;
  static constexpr int BITS = PASS == 2 ? 10 : 11;
  static constexpr unsigned MASK = (1u << BITS) - 1u;
};

template <int PASS>
__global__ __launch_bounds__(BT) void bootstrap_hist_kernel(const float* __restrict__ v, long long n,
                                                            const BootstrapState* __restrict__ st,
                                                            unsigned* __restrict__ slab) {
  typedef Digit<PASS> D;
  __shared__ unsigned h[BINS];
  for (int i = threadIdx.x; i < BINS; i += BT) h[i] = 0u;
  __syncthreads();
  unsigned prefix = 0u;
  if constexpr (PASS > 0) prefix = st->prefix;
  const long long stride = (long long)gridDim.x * BT;
  for (long long i = (long long)blockIdx.x * BT + threadIdx.x; i < n; i += stride) {
    const unsigned b = __float_as_uint(v[i]);
    bool match = true;
    if constexpr (PASS > 0) match = (b >> (D::SHIFT + D::BITS)) == prefix;
    if (match) atomicAdd(&h[(b >> D::SHIFT) & D::MASK], 1u);
  }
  __syncthreads();
  unsigned* row = slab + (size_t)blockIdx.x * BINS;
  for (int i = threadIdx.x; i < BINS; i += BT) row[i] = h[i];
}

// one workgroup: per-bin totals over the slab rows (thread t owns bins 2t, 2t + 1), a suffix
// scan over the thread pairs, and the one thread whose pair holds the rank picks the digit
template <int PASS>
__global__ __launch_bounds__(BT) void bootstrap_scan_kernel(const unsigned* __restrict__ slab,
                                                            int nblk, long long k,
                                                            BootstrapState* st) {
  typedef Digit<PASS> D;
  __shared__ unsigned long long suf[BT];
  const int t = threadIdx.x;
  // the state is read here, barriers before the one thread that rewrites it
  long long rank = k, above = 0;
  unsigned prefix = 0u;
  if constexpr (PASS > 0) { rank = st->rank; above = st->above; prefix = st->prefix; }
  unsigned long long c0 = 0, c1 = 0;
  const uint2* col = reinterpret_cast<const uint2*>(slab) + t;   // row stride BINS / 2 pairs
  constexpr int U = 16;   // loads in flight per thread: the loop is latency-bound (one workgroup)
  int b = 0;
  for (; b + U <= nblk; b += U) {
    uint2 u[U];
#pragma unroll
    for (int j = 0; j < U; ++j) u[j] = col[(size_t)(b + j) * (BINS / 2)];
#pragma unroll
    for (int j = 0; j < U; ++j) { c0 += u[j].x; c1 += u[j].y; }
  }
  for (; b < nblk; ++b) {
    const uint2 u = col[(size_t)b * (BINS / 2)];
    c0 += u.x;
    c1 += u.y;
  }
  suf[t] = c0 + c1;
  __syncthreads();
  for (int off = 1; off < BT; off <<= 1) {
    const unsigned long long add = t + off < BT ? suf[t + off] : 0ull;
    __syncthreads();
    suf[t] += add;
    __syncthreads();
  }
  const unsigned long long incl = suf[t], excl = t + 1 < BT ? suf[t + 1] : 0ull;
  // bins > 2t + 1 hold excl entries, bins >= 2t hold incl: exactly one t has excl < rank <= incl
  if ((long long)excl < rank && rank <= (long long)incl) {
    unsigned long long gt = excl;   // entries in bins above the chosen one
    unsigned d = 2 * t + 1;
    unsigned long long cd = c1;
    if ((long long)(gt + c1) < rank) { gt += c1; d = 2 * t; cd = c0; }
    prefix = (prefix << D::BITS) | d;
    st->prefix = prefix;
    st->rank = rank - (long long)gt;
    st->above = above + (long long)gt;
    if constexpr (PASS == 2) {
      st->tau = __uint_as_float(prefix);
      st->n_ge = above + (long long)gt + (long long)cd;
    }
  }
}

template <int PASS>
hipError_t select_pass(const float* v, long long n, long long k, int nblk, unsigned* slab,
                       BootstrapState* state, hipStream_t s) {
  hipLaunchKernelGGL((bootstrap_hist_kernel<PASS>), dim3(nblk), dim3(BT), 0, s, v, n, state, slab);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((bootstrap_scan_kernel<PASS>), dim3(1), dim3(BT), 0, s, slab, nblk, k, state);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_bootstrap_select(const float* v, long long n, long long k, unsigned* slab,
                                   BootstrapState* state, hipStream_t s) {
  if (!v || !slab || !state || n < 1 || n > 2147483647ll || k < 1 || k > n)
    return hipErrorInvalidValue;
  long long nb = (n + (long long)BT * PER_THREAD - 1) / ((long long)BT * PER_THREAD);
  const int nblk = (int)(nb < 1 ? 1 : nb > BOOTSTRAP_MAX_BLOCKS ? BOOTSTRAP_MAX_BLOCKS : nb);
  hipError_t e = select_pass<0>(v, n, k, nblk, slab, state, s);
  if (e == hipSuccess) e = select_pass<1>(v, n, k, nblk, slab, state, s);
  if (e == hipSuccess) e = select_pass<2>(v, n, k, nblk, slab, state, s);
  return e;
}
