// The skeleton that the TIMESTAMP / MVCC (tso_kernels.h), WAIT_DIE
// (waitdie.hip) and NO_WAIT (nowait.hip) epochs share: the
// batch check's rules, the one-workgroup scan of tile aggregates and the
// rounds loop with its ring of undecided counts.  Nothing here knows an
// engine's tile geometry, txn words or elements; the kernels are per file, as
// rowtab.h's.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <type_traits>

#include "dcc.h"
#include "dcc_ctx.h"
#include "dcc_device.h"
#include "dcc_scan.h"
#include "occ_kernels.h"

namespace dcc {
namespace {

constexpr uint32_t SEG_RING = 64;     // undecided-count ring (> the rounds of one host batch)
constexpr uint32_t SEG_AGG_T = 1024;  // threads of the aggregate scan
constexpr uint32_t CHK_T = 256;       // threads of k_batch_check
// error bits and counter words every engine's check uses; KOR / KNOR are u64.
// An engine's own bits and words lie next to them.
constexpr uint32_t CHK_ERR_OFF = 1, CHK_ERR_KEY = 2;
constexpr uint32_t SEG_C_ERR = 0, SEG_C_MAXLEN = 1, SEG_C_KOR = 8, SEG_C_KNOR = 10;

// ---------------------------------------------------------------- check
// The span of txn t: off[0] == 0, off[n] == nnz, no span runs backwards.
// False for one that does; else its length in `len` and into `maxlen`.
__device__ inline bool check_span(const uint32_t* __restrict__ off, uint64_t t, uint64_t n, uint64_t nnz,
                                  uint32_t& err, uint32_t& maxlen, uint32_t& len) {
  const uint32_t a0 = off[t], b0 = off[t + 1];
  if (t == 0 && a0 != 0) err |= CHK_ERR_OFF;
  if (t == n - 1 && b0 != nnz) err |= CHK_ERR_OFF;
  if (b0 < a0) {
    err |= CHK_ERR_OFF;
    return false;
  }
  len = b0 - a0;
  maxlen = max(maxlen, len);
  return true;
}

// A key: not the reserved one; its bits into the OR of the keys and the OR of
// their complements (a bit set in both varies).
__device__ inline void check_key(uint64_t k, uint32_t& err, uint64_t& kor, uint64_t& knor) {
  if (k == KEY_EMPTY) err |= CHK_ERR_KEY;
  kor |= k;
  knor |= ~k;
}

// The batch's validity before anything indexes with its offsets and before
// any state changes; KEYBITS: the key bits that vary, for the sort's KeyPack.
template <bool KEYBITS>
__global__ __launch_bounds__(CHK_T) void k_batch_check(const uint32_t* __restrict__ off, uint64_t n,
                                                       const uint64_t* __restrict__ keys, uint64_t nnz,
                                                       uint32_t* __restrict__ cnt) {
  __shared__ uint64_t s_a[CHK_T / 64], s_b[CHK_T / 64];
  __shared__ uint32_t s_c[CHK_T / 64], s_d[CHK_T / 64];
  uint32_t maxlen = 0, err = 0, len;
  uint64_t kor = 0, knor = 0;
  const uint64_t tid = (uint64_t)blockIdx.x * CHK_T + threadIdx.x, stride = (uint64_t)gridDim.x * CHK_T;
  for (uint64_t t = tid; t < n; t += stride) check_span(off, t, n, nnz, err, maxlen, len);
  for (uint64_t x = tid; x < nnz; x += stride) check_key(keys[x], err, kor, knor);
  if (KEYBITS) {
    kor = block_reduce<CHK_T / 64, OrOp<uint64_t>>(kor, s_a);
    knor = block_reduce<CHK_T / 64, OrOp<uint64_t>>(knor, s_b);
  }
  maxlen = block_reduce<CHK_T / 64, MaxOp<uint32_t>>(maxlen, s_c);
  err = block_reduce<CHK_T / 64, OrOp<uint32_t>>(err, s_d);
  if (threadIdx.x == 0) {
    if (KEYBITS && kor) atomicOr((unsigned long long*)&cnt[SEG_C_KOR], (unsigned long long)kor);
    if (KEYBITS && knor) atomicOr((unsigned long long*)&cnt[SEG_C_KNOR], (unsigned long long)knor);
    if (maxlen) atomicMax(&cnt[SEG_C_MAXLEN], maxlen);
    if (err) atomicOr(&cnt[SEG_C_ERR], err);
  }
}

// What the check left in the pinned mirror `hc` of the counter words: the
// rejection, or the longest txn, the log2 of the lanes a txn takes and the key
// bits that vary (`keybits` false: the words were not collected).
struct BatchShape {
  uint32_t maxlen = 0, lp = 0;
  uint64_t varying = 0;
};
inline int batch_checked(dcc_ctx* ctx, const uint32_t* hc, uint64_t nnz, bool keybits, BatchShape& s) {
  if (hc[SEG_C_ERR] & CHK_ERR_OFF) return ctx->fail(DCC_EINVAL, "batch: malformed offsets");
  if (hc[SEG_C_ERR] & CHK_ERR_KEY) return ctx->fail(DCC_EINVAL, "batch: key equal to DCC_KEY_RESERVED");
  s.maxlen = hc[SEG_C_MAXLEN];
  if (s.maxlen > MAX_TXN_LEN)
    return ctx->fail(DCC_EINVAL, "batch: a txn has %u accesses (> MAX_ROW_PER_TXN=%u)", s.maxlen, MAX_TXN_LEN);
  s.lp = 0;
  while ((1u << s.lp) < s.maxlen) s.lp++;
  s.varying = 0;
  if (keybits && nnz) {
    uint64_t kor, knor;
    memcpy(&kor, hc + SEG_C_KOR, 8);
    memcpy(&knor, hc + SEG_C_KNOR, 8);
    s.varying = kor & knor;  // a bit set in some key and clear in another
  }
  return DCC_OK;
}

// ----------------------------------------------------------------- scan
// Exclusive scan of the tile aggregates, one workgroup; it also clears the
// ring word this round's advance counts into.
template <class Op>
__global__ __launch_bounds__(SEG_AGG_T) void k_tile_aggscan(const typename Op::T* __restrict__ agg,
                                                            typename Op::T* __restrict__ pre, uint64_t tiles,
                                                            const uint32_t* left, uint32_t* left_out) {
  using T = typename Op::T;
  __shared__ T s_w[SEG_AGG_T / 64];
  if (left_out && threadIdx.x == 0) *left_out = 0;
  if (left && *left == 0) return;
  T carry = Op::identity();
  for (uint64_t c0 = 0; c0 < tiles; c0 += SEG_AGG_T) {
    const uint64_t i = c0 + threadIdx.x;
    const T v = i < tiles ? agg[i] : Op::identity();
    T total;
    const T ex = block_excl_reuse<SEG_AGG_T / 64, Op>(v, s_w, total);
    if (i < tiles) pre[i] = Op::combine(carry, ex);
    carry = Op::combine(carry, total);
  }
}

// --------------------------------------------------------------- rounds
// The rounds of a fixed point.  `ring` is SEG_RING device words: round r reads
// the count round r - 1 left undecided from ring[r % SEG_RING] (nothing to do
// at 0) and counts into ring[(r + 1) % SEG_RING], which one of round r's own
// launches clears before the counting one runs.  Before round 1 the engine has
// put its count into ring[1] and cleared the rest.  `enqueue(r, left, left_out,
// bound)` launches round r; bound: the last undecided count the host has read
// (n before the first read-back), an upper bound of *left for a grid's size.
// Several rounds are enqueued between host synchronisations -- 2, then
// doubling up to DCC_OPT_BATCH_MAX and at most half the ring, so that no round
// of a host batch clears a word the host has yet to read -- and rounds past
// the fixed point return at once.  An enqueue that returns int (one with a
// collective in it) ends the call with its failure.  `rounds` is the first round that left no
// txn undecided; past round `max_r` without one the call fails.  pev[2] is
// recorded behind round 1, pev[3] at the end.
template <class Enqueue>
int rounds_loop(dcc_ctx* ctx, uint32_t* ring, uint64_t n, uint64_t max_r, const char* name, uint32_t& rounds,
                Enqueue enqueue) {
  hipStream_t stream = ctx->stream;
  const bool prof = ctx->profiling;
  uint32_t r = 1;
  uint64_t bound = n;
  uint32_t batch = std::min<uint32_t>(2, ctx->batch_max);
  bool done = false;
  while (!done) {
    const uint32_t r0 = r;
    for (uint32_t q = 0; q < batch; q++, r++) {
      const uint32_t* left = &ring[r % SEG_RING];
      uint32_t* left_out = &ring[(r + 1) % SEG_RING];
      if constexpr (std::is_void_v<decltype(enqueue(r, left, left_out, bound))>) enqueue(r, left, left_out, bound);
      else CR(enqueue(r, left, left_out, bound));
      if (prof && r == 1) CK(hipEventRecord(ctx->pev[2], stream));
    }
    CK(hipGetLastError());
    CK(hipMemcpyAsync(ctx->hmisc, ring, SEG_RING * 4, hipMemcpyDeviceToHost, stream));
    CK(hipStreamSynchronize(stream));
    const uint32_t* hr = (const uint32_t*)ctx->hmisc;
    for (uint32_t q = r0; q < r; q++) {
      const uint32_t left = hr[(q + 1) % SEG_RING];
      if (left == 0) {
        rounds = q;
        done = true;
        break;
      }
      bound = left;
    }
    if (!done && r > max_r) return ctx->fail(DCC_EIO, "%s: fixed point did not converge", name);
    batch = std::min<uint32_t>(batch * 2, std::min<uint32_t>(ctx->batch_max, SEG_RING / 2));
  }
  if (prof) CK(hipEventRecord(ctx->pev[3], stream));
  return DCC_OK;
}

}  // namespace
}  // namespace dcc
