// Stream compaction over a ragged CSR: the tile bodies shared by the select
// (select.hip) and the abort queue (abortq.hip).
//
// Position t of [0, n) names the source txn s = S.src(t) of the CSR `off`;
// it is taken iff S.take(t, s).  Taken txns keep their position order and
// their accesses their list order.  The pair (taken ? 1 : 0, taken ? len : 0)
// travels as the two halves of one u64 (dcc_scan.h), so one scan places the
// txn rows and the accesses.
//
// Bodies:  csr_count_tiles    one pair per tile of SEL_T consecutive positions;
//                             with CHECK the offsets are checked here, before
//                             anything indexes with them
//          csr_scan_tiles     one workgroup: exclusive scan of the tile pairs,
//                             the totals, the verdict (offsets / capacities)
//          csr_scatter_tiles  per tile: the scan again in LDS, the per-txn rows
//                             (S.row), then the tile's output range [0, tile
//                             accesses) walked by all lanes: lane p finds its
//                             txn by binary search over the tile's LDS scan
// No workgroup waits on another: the tile bases come from the launch before.
// The scatter reads the verdict first and writes nothing unless it is clear.
//
// A Sel provides
//   void begin()                        once per thread, before the first tile
//   uint64_t src(uint64_t t) const      the source txn of position t
//   bool take(uint64_t t, uint64_t s) const
//   void row(uint64_t q, uint64_t t, uint64_t s) const   per-txn arrays of taken row q
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "dcc_scan.h"

namespace dcc {

constexpr uint32_t SEL_T = 256;  // threads per workgroup = positions per tile
constexpr uint32_t SEL_NW = SEL_T / 64;
constexpr uint32_t SEL_KU = 4;  // keys per lane and step of the gather
constexpr uint32_t SEL_ERR_OFF = 1, SEL_ERR_CAP = 2;

using PairOp = AddOp<uint64_t>;  // low word: txns, high word: accesses

__device__ inline uint64_t sel_pair(bool sel, uint32_t len) { return sel ? (1ull | ((uint64_t)len << 32)) : 0ull; }

// The source CSR and where the taken txns go.
struct CsrMove {
  uint64_t n, n_tiles;
  const uint32_t* off;
  const uint64_t* keys;
  const uint8_t* at;
  uint64_t nnz_base;  // value of o_off[0]
  // outputs, already at the bases: row q of the selection is o_*[q]
  uint32_t* o_off;  // [taken + 1]
  uint64_t* o_keys;
  uint8_t* o_at;
  const uint64_t* part;  // exclusive prefix of the tile pairs
  const uint64_t* err;   // the verdict word
};

template <bool CHECK, class Sel>
__device__ __forceinline__ void csr_count_tiles(const uint32_t* __restrict__ off, uint64_t n, uint64_t nnz, Sel S,
                                                uint64_t n_tiles, uint64_t* __restrict__ part,
                                                uint64_t* __restrict__ err_word) {
  __shared__ uint64_t s_w[SEL_NW];
  uint32_t err = 0;
  S.begin();
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t t = tile * SEL_T + threadIdx.x;
    uint64_t v = 0;
    if (t < n) {
      const uint64_t s = S.src(t);
      const uint32_t a0 = off[s], b0 = off[s + 1];
      if (CHECK) {
        if (b0 < a0) err = SEL_ERR_OFF;
        if (t == 0 && a0 != 0) err = SEL_ERR_OFF;
        if (t == n - 1 && b0 != nnz) err = SEL_ERR_OFF;
      }
      v = sel_pair(S.take(t, s), b0 - a0);
    }
    const uint64_t tot = block_reduce_reuse<PairOp>(v, s_w, SEL_NW);
    if (threadIdx.x == 0) part[tile] = tot;
  }
  if (CHECK && err) atomicOr((unsigned long long*)err_word, (unsigned long long)err);
}

// part[tile] becomes the exclusive prefix of the tile pairs.  With well-formed
// offsets the accesses sum to <= nnz < 2^32, so the halves never carry into
// each other; with malformed ones the verdict keeps every later reader out.
__device__ __forceinline__ void csr_scan_tiles(uint64_t* __restrict__ part, uint64_t n_tiles, uint64_t cap_txn,
                                               uint64_t cap_nnz, uint64_t nnz_base, uint64_t* __restrict__ err_word,
                                               uint64_t* __restrict__ total) {
  __shared__ uint64_t s_w[SEL_NW];
  // thread t owns the consecutive tiles [t * chunk, (t + 1) * chunk): one
  // block scan whatever the tile count
  const uint64_t chunk = (n_tiles + SEL_T - 1) / SEL_T;
  const uint64_t q0 = min(n_tiles, threadIdx.x * chunk), q1 = min(n_tiles, q0 + chunk);
  uint64_t v = 0;
  for (uint64_t q = q0; q < q1; q++) v += part[q];
  uint64_t carry;
  uint64_t run = block_excl<PairOp>(v, s_w, SEL_NW, carry);
  for (uint64_t q = q0; q < q1; q++) {
    const uint64_t x = part[q];
    part[q] = run;
    run += x;
  }
  if (threadIdx.x == 0) {
    const uint64_t ns = carry & 0xFFFFFFFFull, ms = carry >> 32;
    *total = carry;
    if (ns > cap_txn || ms > cap_nnz || nnz_base + ms > 0xFFFFFFFFull) *err_word |= SEL_ERR_CAP;
  }
}

// The txn of tile-local output position p: the last t with s_start[t] <= p.
// Unselected and empty txns repeat their successor's start, so that t is the
// one whose accesses cover p.  cnt >= 1 txns, s_start[cnt] = the tile total.
__device__ inline uint32_t sel_find(const uint32_t* s_start, uint32_t cnt, uint32_t p) {
  uint32_t lo = 0, hi = cnt;  // s_start[lo] <= p < s_start[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (s_start[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

template <class Sel>
__device__ __forceinline__ void csr_scatter_tiles(const CsrMove& A, Sel S) {
  __shared__ uint64_t s_w[SEL_NW];
  __shared__ uint32_t s_start[SEL_T + 1];  // first output position of the txn within the tile
  __shared__ uint32_t s_src[SEL_T];        // its first access in the source
  if (*A.err) return;  // malformed offsets or no room: nothing is written
  if (blockIdx.x == 0 && threadIdx.x == 0) A.o_off[0] = (uint32_t)A.nnz_base;
  S.begin();
  for (uint64_t tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
    const uint64_t t = tile * SEL_T + threadIdx.x;
    const uint64_t left = A.n - tile * SEL_T;
    const uint32_t cnt = left < SEL_T ? (uint32_t)left : SEL_T;
    uint32_t a0 = 0, len = 0;
    uint64_t s = 0;
    bool sel = false;
    if (t < A.n) {
      s = S.src(t);
      a0 = A.off[s];
      len = A.off[s + 1] - a0;
      sel = S.take(t, s);
    }
    uint64_t tot;
    const uint64_t ex = block_excl_reuse<PairOp>(sel_pair(sel, len), s_w, SEL_NW, tot);
    const uint64_t base = A.part[tile];
    const uint64_t q0 = base & 0xFFFFFFFFull, x0 = base >> 32;  // the tile's first row / access
    const uint32_t st = (uint32_t)(ex >> 32), m = (uint32_t)(tot >> 32);
    s_start[threadIdx.x] = st;
    s_src[threadIdx.x] = a0;
    if (threadIdx.x == 0) s_start[cnt] = m;
    if (sel) {
      const uint64_t q = q0 + (ex & 0xFFFFFFFFull);
      A.o_off[q + 1] = (uint32_t)(A.nnz_base + x0 + st + len);
      S.row(q, t, s);
    }
    __syncthreads();
    // keys: one per lane, the whole tile's output range contiguous
    uint64_t* ok = A.o_keys + x0;
    for (uint32_t p0 = threadIdx.x; p0 < m; p0 += SEL_KU * SEL_T) {
      uint64_t k[SEL_KU];  // SEL_KU independent searches and loads in flight per lane
#pragma unroll
      for (uint32_t j = 0; j < SEL_KU; j++) {
        const uint32_t p = p0 + j * SEL_T;
        if (p < m) {
          const uint32_t tl = sel_find(s_start, cnt, p);
          k[j] = A.keys[(uint64_t)s_src[tl] + (p - s_start[tl])];
        }
      }
#pragma unroll
      for (uint32_t j = 0; j < SEL_KU; j++) {
        const uint32_t p = p0 + j * SEL_T;
        if (p < m) ok[p] = k[j];
      }
    }
    // access types: bytes up to the first 4-byte boundary of the output, then
    // four per lane as one u32 store (one u32 load where the four lie in one
    // txn and its source is aligned too), then the bytes left over
    uint8_t* oa = A.o_at + x0;
    const uint32_t head = min(m, (uint32_t)((4 - ((uintptr_t)oa & 3)) & 3));
    const uint32_t quads = (m - head) >> 2;
    if (threadIdx.x < m - 4 * quads) {  // at most 6 bytes
      const uint32_t p = threadIdx.x < head ? threadIdx.x : threadIdx.x + 4 * quads;
      const uint32_t tl = sel_find(s_start, cnt, p);
      oa[p] = A.at[(uint64_t)s_src[tl] + (p - s_start[tl])];
    }
    for (uint32_t g = threadIdx.x; g < quads; g += SEL_T) {
      const uint32_t p = head + 4 * g;
      uint32_t tl = sel_find(s_start, cnt, p);
      const uint8_t* sp = A.at + (uint64_t)s_src[tl] + (p - s_start[tl]);
      uint32_t w;
      if (p + 3 < s_start[tl + 1] && ((uintptr_t)sp & 3) == 0) {
        w = *(const uint32_t*)sp;
      } else {
        w = sp[0];
#pragma unroll
        for (uint32_t k = 1; k < 4; k++) {
          if (p + k >= s_start[tl + 1]) tl = sel_find(s_start, cnt, p + k);
          w |= (uint32_t)A.at[(uint64_t)s_src[tl] + (p + k - s_start[tl])] << (8 * k);
        }
      }
      *(uint32_t*)(oa + p) = w;
    }
    __syncthreads();  // the LDS arrays are rewritten by the next tile
  }
}

inline unsigned sel_grid(uint64_t tiles, unsigned max_grid) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(tiles, max_grid));
}

}  // namespace dcc
