// The MVCC version store's shared pieces: (key, ts) pairs sorted by (key, ts)
// in two buffers (dcc_ctx::mv_sk / mv_st), searched and merged by the epoch
// engine (mvcc.hip) and by the engine with txns in flight (mvcc_live.hip).
// The kernels are per file, as rowtab.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "dcc_scan.h"

namespace dcc {
namespace {

constexpr uint32_t MVS_T = 256;       // threads per workgroup of k_mv_merge
constexpr uint32_t MVS_OFF_T = 1024;  // threads of the tile-offset scan

// Exclusive scan of the tile counts in place, one workgroup; the sum to *total.
__global__ __launch_bounds__(MVS_OFF_T) void k_mv_offsets(uint64_t* toff, uint64_t tiles, uint64_t* total) {
  __shared__ uint64_t s_w[MVS_OFF_T / 64];
  uint64_t carry = 0;
  for (uint64_t c0 = 0; c0 < tiles; c0 += MVS_OFF_T) {
    const uint64_t i = c0 + threadIdx.x;
    const uint64_t v = i < tiles ? toff[i] : 0;
    uint64_t sum;
    const uint64_t ex = block_excl_reuse<MVS_OFF_T / 64, AddOp<uint64_t>>(v, s_w, sum);
    if (i < tiles) toff[i] = carry + ex;
    carry += sum;
  }
  if (threadIdx.x == 0) *total = carry;
}

// The number of leading elements of (k[], t[]) with (key, ts) <= (K, T).
__device__ inline uint64_t mv_upper(const uint64_t* __restrict__ k, const uint64_t* __restrict__ t, uint64_t n,
                                    uint64_t K, uint64_t T) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    const uint64_t kk = k[mid];
    if (kk < K || (kk == K && t[mid] <= T)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

struct MvStore {
  const uint64_t* k;
  const uint64_t* t;
  uint64_t n;
};

// Merge by rank into (dk, dt): old element i goes to i + the new elements with
// a smaller key, new element j to j + the old elements with a key <= its own.
// (Within a key every old ts <= every new one, so this is (key, ts) order.)
__global__ __launch_bounds__(MVS_T) void k_mv_merge(MvStore S, const uint64_t* __restrict__ ek,
                                                   const uint64_t* __restrict__ et,
                                                   const uint64_t* __restrict__ nc_p, uint64_t* __restrict__ dk,
                                                   uint64_t* __restrict__ dt) {
  const uint64_t nc = *nc_p, all = S.n + nc;
  for (uint64_t g = (uint64_t)blockIdx.x * MVS_T + threadIdx.x; g < all; g += (uint64_t)gridDim.x * MVS_T) {
    uint64_t k, t, pos;
    if (g < S.n) {
      k = S.k[g], t = S.t[g];
      uint64_t lo = 0, hi = nc;  // new elements with key < k
      while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (ek[mid] < k) lo = mid + 1;
        else hi = mid;
      }
      pos = g + lo;
    } else {
      const uint64_t j = g - S.n;
      k = ek[j], t = et[j];
      pos = j + mv_upper(S.k, S.t, S.n, k, ~0ull);
    }
    dk[pos] = k;
    dt[pos] = t;
  }
}

}  // namespace
}  // namespace dcc
