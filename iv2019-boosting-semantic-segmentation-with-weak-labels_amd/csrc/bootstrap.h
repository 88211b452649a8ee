// Exact K-th-largest selection over a device array of non-negative floats (the bootstrapped
// per-pixel loss of seg_set_bootstrap): the threshold tau and the count of entries >= tau, on the
// stream, without a host round trip.
//
// Non-negative IEEE floats order as their bit patterns do, so the select is an MSB-first radix
// select on the uint32 bits in three digit passes of 11 + 11 + 10 bits. Each pass is two launches:
//   hist   every workgroup histograms the digit of its grid-stride share of the entries that
//          still match the prefix chosen so far (LDS integer atomics) and stores its 2048 counts
//          to its own slab row (plain stores: nothing to zero, no global atomics);
//   scan   one workgroup sums the slab rows per bin, suffix-scans the bins from the top, picks
//          the digit that holds the remaining rank and updates {prefix, rank, above} in the
//          device state; the last pass writes tau and n_ge.
// Integer counts do not depend on arrival order: the result is bitwise reproducible.
// Entries must be finite and >= +0 (a set sign bit -- -0.0f included -- would order above every
// positive value).
#pragma once
#include "seg_common.h"

struct BootstrapState {
  unsigned prefix;        // the digits chosen so far (high bits of tau)
  float tau;              // result: the k-th largest entry
  long long rank;         // remaining rank among the entries matching prefix
  long long above;        // entries strictly greater than every entry matching prefix
  long long n_ge;         // result: entries >= tau
};

constexpr int BOOTSTRAP_BINS = 2048;
constexpr int BOOTSTRAP_MAX_BLOCKS = 256;
// workspace: slab of BOOTSTRAP_MAX_BLOCKS x BOOTSTRAP_BINS uint32 counts
constexpr size_t BOOTSTRAP_SLAB_BYTES = (size_t)BOOTSTRAP_MAX_BLOCKS * BOOTSTRAP_BINS * 4;

// 1 <= k <= n <= 2^31 - 1 (hipErrorInvalidValue otherwise); six launches on s
hipError_t launch_bootstrap_select(const float* v, long long n, long long k, unsigned* slab,
                                   BootstrapState* state, hipStream_t s);
