// Basic timestamp ordering (CC_ALG TIMESTAMP) for a whole epoch
// (dcc_tso_validate_epoch), with the rows' wts / rts persistent in the
// context's row table (rowtab.h, probe policy ProbeMix).
//
// Reference: the txns of the batch run in index order, each one atomically:
// get_row for its accesses in list order (storage/row.cpp:239-282: WR sends
// P_REQ then R_REQ, RD / SCAN send R_REQ) against Row_ts::access
// (concurrency_control/row_ts.cpp:167-266), then cleanup (system/txn.cpp:
// 700-761, row.cpp:371-390): W_REQ per WR access of a committed txn, XP_REQ
// per WR access of an aborted one.  With one txn in flight no request is ever
// buffered, so only the comparisons are left:
//
//   R_REQ  abort iff ts < wts, else rts = max(rts, ts)          (:176, :188)
//   P_REQ  abort iff ts < rts or ts < wts                       (:193, :200)
//   W_REQ  wts = max(wts, ts)                                   (:237-239)
//   XP_REQ drops the prewrite; the rts bumps of the aborted txn stay
//
// Closed form per row K, over the accesses of K in index order: a WR access
// of txn i fails iff ts_i < max(rts0, wts0, ts_j of the executed non-XP
// accesses of txns j < i), a RD / SCAN access iff ts_i < max(wts0, ts_j of
// the committed txns j < i with a WR on K).  An access at position q of txn j
// is executed iff j did not abort at an ordinal <= q.  The maxima over the
// whole epoch are the row's new rts and wts.  (A txn's own earlier accesses
// add ts_i, which `ts_i < ts_i` never trips, so the prefix may hold them.)
//
// Whether an access is executed depends on the decisions, so the epoch is a
// fixed point.  The accesses are sorted stably by row (CSR order is index
// order, so every row's segment is in index order).  A txn is undecided with
// a progress p (accesses below p passed for certain), committed (p = its
// length) or aborted at p.  A round takes, per access, the exclusive segmented
// prefix maxima of ts in four flavours -- executed for certain / possibly
// executed, committed writer for certain / possibly -- and every undecided
// txn advances p while ts >= the possible bound, aborts at p if ts < the
// certain bound and stops otherwise.  The certain bound is below the true
// one and the possible bound above it, the certain sets only grow and the
// possible sets only shrink, and for the lowest undecided txn the two are
// equal, so it is decided in every round: the result is the replay's.
//
// Kernels:  k_ts_check    offsets / reserved keys / longest txn / varying key bits
//           k_ts_prep     packed sort keys, the record of every access, WR / read-only counts
//           k_ts_seg      sorted records (txn, position | type | head | last, ts), heads
//           k_ts_seed     a row-table slot per segment head (find or insert)
//           k_ts_scan     per 1,024-access tile: its aggregate (reduce) or,
//                         behind the scanned aggregates, the bounds of every
//                         access (apply); the final apply writes the rows
//           k_ts_aggscan  exclusive scan of the tile aggregates (one workgroup)
//           k_ts_advance  one round of decisions from the bounds
//           k_ts_rc       RC bytes, conflict ordinals, the commit count
// No workgroup waits on another: a round is reduce / scan of aggregates /
// apply / advance, four launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "dcc.h"
#include "dcc_ctx.h"
#include "dcc_device.h"
#include "dcc_scan.h"
#include "nowait_lanes.h"
#include "occ_kernels.h"
#include "radix_sort.h"
#include "rowtab.h"

using namespace dcc;

namespace {

constexpr uint32_t TS_T = 256;                    // threads per workgroup
constexpr uint32_t TS_ITEMS = 4;                  // consecutive sorted accesses per thread
constexpr uint32_t TS_TILE = TS_T * TS_ITEMS;     // accesses per scan tile
constexpr uint32_t TS_AGG_T = 1024;               // threads of the aggregate scan
constexpr uint32_t TS_RING = 64;                  // undecided-count ring (> the rounds of one host batch)
constexpr uint32_t TS_ERR_OFF = 1, TS_ERR_KEY = 2, TS_ERR_FULL = 4, TS_ERR_STATE = 8;
// counter words (ts_misc); KOR / KNOR are u64 at words 8 and 10
constexpr uint32_t TS_C_ERR = 0, TS_C_MAXLEN = 1, TS_C_NWR = 2, TS_C_RO = 3, TS_C_COMMIT = 4,
                   TS_C_HEADS = 5, TS_C_ROWS = 6, TS_C_KOR = 8, TS_C_KNOR = 10, TS_C_RING = 16,
                   TS_C_WORDS = TS_C_RING + TS_RING;
constexpr uint32_t TS_NONE = ROW_NONE;
// sorted record word: position | type << 8 | head << 16 | last << 17
constexpr uint32_t TS_I_HEAD = 1u << 16, TS_I_LAST = 1u << 17;
// txn word: state << 8 | progress
__device__ inline uint32_t st_state(uint32_t w) { return w >> 8; }
__device__ inline uint32_t st_prog(uint32_t w) { return w & 0xFFu; }

// The persistent rows: rowtab.h's slot {key, a, b} holds a row's wts / rts
// (tab[s].*WTS).
using TsProbe = ProbeMix;
constexpr auto WTS = &RowSlot::a, RTS = &RowSlot::b;

// ---------------------------------------------------------------- check
// The batch's validity before anything indexes with its offsets and before
// the row table changes; the key bits that vary (OR of the keys, OR of their
// complements) for the sort's KeyPack.
__global__ __launch_bounds__(TS_T) void k_ts_check(const uint32_t* __restrict__ off, uint64_t n,
                                                   const uint64_t* __restrict__ keys, uint64_t nnz,
                                                   uint32_t* __restrict__ cnt) {
  __shared__ uint64_t s_a[TS_T / 64], s_b[TS_T / 64];
  __shared__ uint32_t s_c[TS_T / 64], s_d[TS_T / 64];
  uint32_t len = 0, err = 0;
  uint64_t kor = 0, knor = 0;
  const uint64_t tid = (uint64_t)blockIdx.x * TS_T + threadIdx.x, stride = (uint64_t)gridDim.x * TS_T;
  for (uint64_t t = tid; t < n; t += stride) {
    const uint32_t a0 = off[t], b0 = off[t + 1];
    if (b0 < a0) err |= TS_ERR_OFF;
    else len = max(len, b0 - a0);
    if (t == 0 && a0 != 0) err |= TS_ERR_OFF;
    if (t == n - 1 && b0 != nnz) err |= TS_ERR_OFF;
  }
  for (uint64_t x = tid; x < nnz; x += stride) {
    const uint64_t k = keys[x];
    if (k == KEY_EMPTY) err |= TS_ERR_KEY;
    kor |= k;
    knor |= ~k;
  }
  kor = block_reduce<TS_T / 64, OrOp<uint64_t>>(kor, s_a);
  knor = block_reduce<TS_T / 64, OrOp<uint64_t>>(knor, s_b);
  len = block_reduce<TS_T / 64, MaxOp<uint32_t>>(len, s_c);
  err = block_reduce<TS_T / 64, OrOp<uint32_t>>(err, s_d);
  if (threadIdx.x == 0) {
    if (kor) atomicOr((unsigned long long*)&cnt[TS_C_KOR], (unsigned long long)kor);
    if (knor) atomicOr((unsigned long long*)&cnt[TS_C_KNOR], (unsigned long long)knor);
    if (len) atomicMax(&cnt[TS_C_MAXLEN], len);
    if (err) atomicOr(&cnt[TS_C_ERR], err);
  }
}

struct TsArgs {
  uint64_t n, m;
  const uint32_t* off;
  const uint64_t* keys;
  const uint8_t* at;
  const uint64_t* ts;
  uint32_t lp;      // log2 lanes per txn (k_ts_prep, k_ts_advance)
  uint4* arec;      // [m] {txn, position | type << 8, ts lo, ts hi} of every access
  uint32_t* stp;    // [n] state << 8 | progress
  ulonglong2* bnd;  // [m] (certain, possible) bound of every access, batch order
  uint32_t* cnt;
};

// P lanes per txn (nowait_lanes.h): the sort's packed key and value of every
// access and its record (what k_ts_seg needs of it, so that the sorted side
// takes one 16-byte gather per access); WR accesses and read-only txns
// counted; every txn undecided at progress 0, all n of them in the ring word
// round 1 reads.
__global__ __launch_bounds__(TS_T) void k_ts_prep(TsArgs A, KeyPack kp, uint64_t* __restrict__ ak,
                                                  uint32_t* __restrict__ av) {
  if (blockIdx.x == 0 && threadIdx.x == 0) A.cnt[TS_C_RING + 1] = (uint32_t)A.n;
  const Seg g = seg_of(A.lp);
  const uint32_t gpb = TS_T >> A.lp;
  uint32_t ro = 0, nwr = 0;
  for (uint64_t g0 = (uint64_t)blockIdx.x * gpb; g0 < A.n; g0 += (uint64_t)gridDim.x * gpb) {
    const uint64_t t = g0 + g.gl;
    const bool tv = t < A.n;
    uint32_t o0 = 0, len = 0;
    uint64_t tsv = 0;
    if (tv) {
      o0 = A.off[t];
      len = A.off[t + 1] - o0;
      tsv = A.ts[t];
    }
    const bool v = tv && g.a < len;
    const uint64_t x = (uint64_t)o0 + g.a;
    bool wr = false;
    if (v) {
      const uint32_t ty = A.at[x] & 3u;
      wr = ty == DCC_WR;
      ak[x] = keypack_apply(kp, A.keys[x]);
      av[x] = (uint32_t)x;
      A.arec[x] = make_uint4((uint32_t)t, g.a | (ty << 8), (uint32_t)tsv, (uint32_t)(tsv >> 32));
    }
    const uint64_t wb = ballot64(wr) & g.mask;
    if (tv && g.a == 0) {
      A.stp[t] = ST_UNDECIDED << 8;
      ro += wb ? 0u : 1u;
      nwr += (uint32_t)__popcll(wb);
    }
  }
  block_add<TS_T / 64>(ro, &A.cnt[TS_C_RO]);
  __syncthreads();  // block_add's LDS words are read before the next call writes them
  block_add<TS_T / 64>(nwr, &A.cnt[TS_C_NWR]);
}

// The sorted records: sk / sv are the sorted packed keys and access indices.
__global__ __launch_bounds__(TS_T) void k_ts_seg(TsArgs A, const uint64_t* __restrict__ sk,
                                                 const uint32_t* __restrict__ sv, uint32_t* __restrict__ s_txn,
                                                 uint32_t* __restrict__ s_info, uint64_t* __restrict__ s_ts) {
  uint32_t heads = 0;
  for (uint64_t s = (uint64_t)blockIdx.x * TS_T + threadIdx.x; s < A.m; s += (uint64_t)gridDim.x * TS_T) {
    const uint64_t k = sk[s];
    const bool head = s == 0 || sk[s - 1] != k, last = s + 1 == A.m || sk[s + 1] != k;
    const uint4 r = A.arec[sv[s]];
    s_txn[s] = r.x;
    s_info[s] = r.y | (head ? TS_I_HEAD : 0u) | (last ? TS_I_LAST : 0u);
    s_ts[s] = (uint64_t)r.z | ((uint64_t)r.w << 32);
    heads += head;
  }
  block_add<TS_T / 64>(heads, &A.cnt[TS_C_HEADS]);
}

// The row's slot, once per segment head (the table has room for every head).
__global__ __launch_bounds__(TS_T) void k_ts_seed(uint64_t m, const uint32_t* __restrict__ s_info,
                                                  const uint32_t* __restrict__ sv,
                                                  const uint64_t* __restrict__ keys, RowSlot* tab, uint32_t mask,
                                                  uint32_t* __restrict__ hslot, uint32_t* __restrict__ cnt) {
  uint32_t c = 0;
  for (uint64_t s = (uint64_t)blockIdx.x * TS_T + threadIdx.x; s < m; s += (uint64_t)gridDim.x * TS_T) {
    if (!(s_info[s] & TS_I_HEAD)) continue;
    bool ins;
    const uint32_t slot = probe_insert<TsProbe>(tab, mask, keys[sv[s]], ins);
    if (slot == TS_NONE) atomicOr(&cnt[TS_C_ERR], TS_ERR_FULL);
    hslot[s] = slot;
    c += ins;
  }
  block_add<TS_T / 64>(c, &cnt[TS_C_ROWS]);
}

// ----------------------------------------------------------------- scan
// The segmented maximum of four timestamps; f: the element is, or the run
// holds, a segment head (what lies before it does not reach past it).
struct Tq {
  uint64_t de, pe, dw, pw;  // executed: certain / possible; committed writer: certain / possible
  uint32_t f;
};
struct TqOp {
  using T = Tq;
  static constexpr bool has_inverse = false;
  __device__ static Tq identity() { return Tq{0, 0, 0, 0, 0}; }
  __device__ static Tq combine(const Tq& a, const Tq& b) {
    if (b.f) return b;
    return Tq{max(a.de, b.de), max(a.pe, b.pe), max(a.dw, b.dw), max(a.pw, b.pw), a.f};
  }
  __device__ static Tq shfl_up(const Tq& v, uint32_t d) {
    return Tq{(uint64_t)__shfl_up(v.de, d), (uint64_t)__shfl_up(v.pe, d), (uint64_t)__shfl_up(v.dw, d),
              (uint64_t)__shfl_up(v.pw, d), (uint32_t)__shfl_up(v.f, d)};
  }
};

struct ScanArgs {
  uint64_t m;
  const uint32_t* s_txn;
  const uint32_t* s_info;
  const uint64_t* s_ts;
  const uint32_t* sv;
  const uint32_t* hslot;
  const uint32_t* stp;
  RowSlot* tab;
  Tq* agg;          // [tiles] the tile aggregates
  Tq* pre;          // [tiles] their exclusive prefixes (k_ts_aggscan)
  uint8_t* tdone;   // [tiles] every access of the tile belongs to a decided txn
  ulonglong2* bnd;
  const uint32_t* left;  // txns undecided before this round: 0 = nothing to do
  uint32_t* err;
};

// The element an access contributes under the current decisions.  A segment
// head takes the row's state in: what a WR is checked against, max(rts0, wts0),
// and what a read is checked against, wts0.  FINAL (every txn decided, the
// possible values equal the certain ones): rts0 and wts0 apart, as the row
// keeps them, and the head's slot rides in `pe` to the segment's last element.
template <bool FINAL>
__device__ inline Tq ts_elem(uint32_t info, uint32_t st, uint64_t ts, uint32_t slot, const RowSlot* tab) {
  const uint32_t q = info & 0xFFu, ty = (info >> 8) & 3u;
  const uint32_t state = st_state(st), p = st_prog(st);
  const bool nx = ty != DCC_XP, wr = ty == DCC_WR;
  const bool dex = q < p, pex = state == ST_UNDECIDED || dex;
  Tq e;
  e.de = nx && dex ? ts : 0;
  e.pe = !FINAL && nx && pex ? ts : 0;
  e.dw = wr && state == ST_COMMIT ? ts : 0;
  e.pw = !FINAL && wr && state != ST_ABORT ? ts : 0;
  e.f = (info & TS_I_HEAD) ? 1u : 0u;
  if (FINAL && e.f) e.pe = slot;  // TS_NONE (a full table) is reported by the last element
  if (e.f && slot != TS_NONE) {
    const uint64_t w0 = tab[slot].*WTS, r0 = tab[slot].*RTS;
    if (FINAL) {
      e.de = max(e.de, r0);
      e.dw = max(e.dw, w0);
    } else {
      const uint64_t b = max(w0, r0);
      e.de = max(e.de, b);
      e.pe = max(e.pe, b);
      e.dw = max(e.dw, w0);
      e.pw = max(e.pw, w0);
    }
  }
  return e;
}

// One tile: thread t holds the sorted accesses 4t .. 4t + 3 of it.  !APPLY:
// the tile's aggregate.  Once every access of a tile belongs to a decided txn
// its aggregate is final and no access of it needs bounds: the rounds after
// that skip the tile (tdone).  APPLY: behind the tile's exclusive prefix, the
// bounds of every access of an undecided txn, in batch order; FINAL: the row's
// new (wts, rts) from the segment's last element, plain stores by one thread
// per row.
template <bool APPLY, bool FINAL>
__global__ __launch_bounds__(TS_T) void k_ts_scan(ScanArgs A) {
  __shared__ Tq s_w[TS_T / 64];
  if (!FINAL && (*A.left == 0 || A.tdone[blockIdx.x])) return;
  const uint64_t base = (uint64_t)blockIdx.x * TS_TILE + (uint64_t)threadIdx.x * TS_ITEMS;
  uint32_t info[TS_ITEMS], st[TS_ITEMS], x[TS_ITEMS];
  uint64_t ts[TS_ITEMS];
  Tq e[TS_ITEMS];
  if (base + TS_ITEMS <= A.m) {  // 16-B loads: the arrays are tile-aligned
    const uint4 i4 = *(const uint4*)(A.s_info + base), t4 = *(const uint4*)(A.s_txn + base);
    const ulonglong2 a = *(const ulonglong2*)(A.s_ts + base), b = *(const ulonglong2*)(A.s_ts + base + 2);
    info[0] = i4.x, info[1] = i4.y, info[2] = i4.z, info[3] = i4.w;
    st[0] = A.stp[t4.x], st[1] = A.stp[t4.y], st[2] = A.stp[t4.z], st[3] = A.stp[t4.w];
    ts[0] = a.x, ts[1] = a.y, ts[2] = b.x, ts[3] = b.y;
    if (APPLY && !FINAL) {
      const uint4 x4 = *(const uint4*)(A.sv + base);
      x[0] = x4.x, x[1] = x4.y, x[2] = x4.z, x[3] = x4.w;
    }
  } else {
#pragma unroll
    for (uint32_t k = 0; k < TS_ITEMS; k++) {
      const bool v = base + k < A.m;
      info[k] = v ? A.s_info[base + k] : 0u;  // past the end: an identity element
      st[k] = v ? A.stp[A.s_txn[base + k]] : (uint32_t)(ST_ABORT << 8);
      ts[k] = v ? A.s_ts[base + k] : 0;
      if (APPLY && !FINAL) x[k] = v ? A.sv[base + k] : 0u;
    }
  }
  Tq mine = TqOp::identity();
#pragma unroll
  for (uint32_t k = 0; k < TS_ITEMS; k++) {
    const uint32_t slot = (info[k] & TS_I_HEAD) ? A.hslot[base + k] : TS_NONE;
    e[k] = ts_elem<FINAL>(info[k], st[k], ts[k], slot, A.tab);
    mine = TqOp::combine(mine, e[k]);
  }
  Tq total;
  const Tq excl = block_excl<TS_T / 64, TqOp>(mine, s_w, total);
  if (!APPLY) {
    bool und = false;
#pragma unroll
    for (uint32_t k = 0; k < TS_ITEMS; k++) und |= st_state(st[k]) == ST_UNDECIDED;  // past the end: aborted
    const bool any = !FINAL && __syncthreads_or(und);
    if (threadIdx.x == 0) {
      A.agg[blockIdx.x] = total;
      if (!FINAL && !any) A.tdone[blockIdx.x] = 1;
    }
    return;
  }
  Tq run = TqOp::combine(A.pre[blockIdx.x], excl);
#pragma unroll
  for (uint32_t k = 0; k < TS_ITEMS; k++) {
    const bool v = base + k < A.m;
    if (!FINAL) {
      // the exclusive prefix of a head is the row's state, which its element
      // holds (next to its own ts, which never fails it: ts < ts is false)
      const uint32_t ty = (info[k] >> 8) & 3u;
      const Tq b = (info[k] & TS_I_HEAD) ? e[k] : run;
      if (v && ty != DCC_XP && st_state(st[k]) == ST_UNDECIDED) {
        const bool wr = ty == DCC_WR;
        A.bnd[x[k]] = make_ulonglong2(wr ? b.de : b.dw, wr ? b.pe : b.pw);
      }
    }
    run = TqOp::combine(run, e[k]);
    if (FINAL && v && (info[k] & TS_I_LAST)) {
      const uint32_t slot = (uint32_t)run.pe;
      if (slot == TS_NONE) {
        atomicOr(A.err, TS_ERR_STATE);
      } else {
        A.tab[slot].*WTS = run.dw;
        A.tab[slot].*RTS = run.de;
      }
    }
  }
}

// Exclusive scan of the tile aggregates, one workgroup; it also clears the
// ring word this round's k_ts_advance counts into.
__global__ __launch_bounds__(TS_AGG_T) void k_ts_aggscan(const Tq* __restrict__ agg, Tq* __restrict__ pre,
                                                         uint64_t tiles, const uint32_t* left,
                                                         uint32_t* left_out) {
  __shared__ Tq s_w[TS_AGG_T / 64];
  if (left_out && threadIdx.x == 0) *left_out = 0;
  if (left && *left == 0) return;
  Tq carry = TqOp::identity();
  for (uint64_t c0 = 0; c0 < tiles; c0 += TS_AGG_T) {
    const uint64_t i = c0 + threadIdx.x;
    const Tq v = i < tiles ? agg[i] : TqOp::identity();
    Tq total;
    const Tq ex = block_excl_reuse<TS_AGG_T / 64, TqOp>(v, s_w, total);
    if (i < tiles) pre[i] = TqOp::combine(carry, ex);
    carry = TqOp::combine(carry, total);
  }
}

// One round of decisions.  P lanes per txn, one access per lane: the first
// access at or past the progress that does not pass for certain is where the
// txn aborts (below the certain bound) or stops.  Counts the txns it leaves
// undecided.
__global__ __launch_bounds__(TS_T) void k_ts_advance(TsArgs A, const uint32_t* __restrict__ left,
                                                     uint32_t* left_out) {
  if (*left == 0) return;
  const Seg g = seg_of(A.lp);
  const uint32_t gpb = TS_T >> A.lp;
  uint32_t und_left = 0;
  for (uint64_t g0 = (uint64_t)blockIdx.x * gpb; g0 < A.n; g0 += (uint64_t)gridDim.x * gpb) {
    const uint64_t t = g0 + g.gl;
    const bool tv = t < A.n;
    const uint32_t st = tv ? A.stp[t] : (uint32_t)(ST_COMMIT << 8);
    const bool und = tv && st_state(st) == ST_UNDECIDED;
    if (!ballot64(und)) continue;  // the wave's txns are decided
    uint32_t o0 = 0, len = 0;
    uint64_t tsv = 0;
    if (und) {
      o0 = A.off[t];
      len = A.off[t + 1] - o0;
      tsv = A.ts[t];
    }
    const bool v = und && g.a < len && g.a >= st_prog(st);
    bool stop = false, fail = false;
    if (v) {
      const uint64_t x = (uint64_t)o0 + g.a;
      if (A.at[x] != DCC_XP) {
        const ulonglong2 b = A.bnd[x];
        stop = tsv < b.y;
        fail = tsv < b.x;
      }
    }
    const uint64_t sb = ballot64(stop) & g.mask, fb = ballot64(fail);
    if (und && g.a == 0) {
      uint32_t w;
      if (!sb) {
        w = (ST_COMMIT << 8) | len;
      } else {
        const uint32_t l = (uint32_t)__builtin_ctzll(sb);
        const bool ab = (fb >> l) & 1ull;
        w = ((ab ? ST_ABORT : ST_UNDECIDED) << 8) | (l - g.seg0);
        und_left += ab ? 0u : 1u;
      }
      A.stp[t] = w;
    }
  }
  block_add<TS_T / 64>(und_left, left_out);
}

__global__ __launch_bounds__(TS_T) void k_ts_rc(uint64_t n, const uint32_t* __restrict__ stp,
                                                uint8_t* __restrict__ rc, uint32_t* __restrict__ conflict,
                                                uint32_t* __restrict__ cnt) {
  uint32_t commits = 0, bad = 0;
  for (uint64_t t = (uint64_t)blockIdx.x * TS_T + threadIdx.x; t < n; t += (uint64_t)gridDim.x * TS_T) {
    const uint32_t st = stp[t];
    const bool ok = st_state(st) == ST_COMMIT;
    rc[t] = ok ? DCC_RC_RCOK : DCC_RC_ABORT;
    if (conflict) conflict[t] = ok ? DCC_ACCESS_NONE : st_prog(st);
    commits += ok;
    bad |= st_state(st) == ST_UNDECIDED;
  }
  if (bad) atomicOr(&cnt[TS_C_ERR], TS_ERR_STATE);
  block_add<TS_T / 64>(commits, &cnt[TS_C_COMMIT]);
}

unsigned ts_grid(uint64_t items, uint64_t per_block, unsigned max_grid) {
  const uint64_t b = (items + per_block - 1) / per_block;
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(b, max_grid));
}

}  // namespace

int dcc_ctx::tso_reserve(uint64_t n, uint64_t nnz, bool with_conflict) {
  const uint64_t nn = std::max<uint64_t>(n, 1), mm = std::max<uint64_t>(nnz, 1);
  const uint64_t mt = (mm + TS_TILE - 1) / TS_TILE * TS_TILE;  // whole tiles: 16-B loads
  CR(ts_misc.ensure(this, TS_C_WORDS * 4, "tso counters"));
  CR(ts_stp.ensure(this, nn * 4, "tso txn words"));
  CR(ts_arec.ensure(this, mm * 16, "tso access records"));
  for (int q = 0; q < 2; q++) {
    CR(ts_k[q].ensure(this, mt * 8, "tso sort keys"));
    CR(ts_v[q].ensure(this, mt * 4, "tso sort values"));
  }
  CR(ts_stxn.ensure(this, mt * 4, "tso sorted txns"));
  CR(ts_sinfo.ensure(this, mt * 4, "tso sorted records"));
  CR(ts_sts.ensure(this, mt * 8, "tso sorted timestamps"));
  CR(ts_hslot.ensure(this, mt * 4, "tso head slots"));
  CR(ts_bnd.ensure(this, mm * 16, "tso bounds"));
  CR(ts_agg.ensure(this, 2 * (mt / TS_TILE) * sizeof(Tq), "tso tile aggregates and prefixes"));
  CR(ts_tdone.ensure(this, mt / TS_TILE, "tso tile flags"));
  CR(cv_scratch.ensure(this, rs_scratch_words(mm) * 4 + 64, "radix scratch"));
  CR(rc.ensure(this, n + 16, "rc"));
  if (with_conflict) CR(ts_conf.ensure(this, nn * 4, "tso conflicts"));
  return DCC_OK;
}

int dcc_ctx::tso_epoch(const dcc_batch* b, const uint64_t* ts_in, uint8_t* out_rc, uint32_t* out_conflict,
                       dcc_stats* st) {
  dcc_ctx* ctx = this;
  EpochStats es;
  dcc_stats& S = es.S;
  if (!out_rc) return fail(DCC_EINVAL, "tso: null out_rc");
  if (!ts_in) return fail(DCC_EINVAL, "tso: null ts");
  CR(check_batch(b, false));  // the offsets are checked on the device (k_ts_check)
  if (comm_ranks() > 1) return fail(DCC_ENOTSUP, "tso: single-GPU engine");
  const bool dev = (b->flags & DCC_DEVICE_PTRS) != 0;
  if (b->n_txn == 0) {
    if (st) *st = S;
    return DCC_OK;
  }
  DevBatch d;
  CR(stage_batch(b, d));
  const uint64_t n = d.n, m = d.nnz;
  CR(tso_reserve(n, m, out_conflict != nullptr && !dev));
  const uint64_t* ts_dev;
  CR(stage(ts_stage, ts_in, n * 8, dev, "tso timestamps", ts_dev));
  uint32_t* cnt = (uint32_t*)ts_misc.p;
  uint32_t* ring = cnt + TS_C_RING;
  uint8_t* rc_dev = dev ? out_rc : (uint8_t*)rc.p;
  uint32_t* conf_dev = out_conflict ? (dev ? out_conflict : (uint32_t*)ts_conf.p) : nullptr;
  const unsigned max_grid = (unsigned)n_cu * 16;

  // reject a malformed batch before anything indexes with its offsets: the row
  // table is untouched by a rejected call
  CK(hipMemsetAsync(cnt, 0, TS_C_WORDS * 4, stream));
  k_ts_check<<<ts_grid(std::max(n, m), TS_T * 4, max_grid), TS_T, 0, stream>>>(d.off, n, d.keys, m, cnt);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(hmisc, cnt, TS_C_RING * 4, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  uint32_t maxlen = 0;
  uint64_t varying = 0;
  {
    const uint32_t* hc = (const uint32_t*)hmisc;
    if (hc[TS_C_ERR] & TS_ERR_OFF) return fail(DCC_EINVAL, "batch: malformed offsets");
    if (hc[TS_C_ERR] & TS_ERR_KEY) return fail(DCC_EINVAL, "batch: key equal to DCC_KEY_RESERVED");
    maxlen = hc[TS_C_MAXLEN];
    if (maxlen > MAX_TXN_LEN)
      return fail(DCC_EINVAL, "batch: a txn has %u accesses (> MAX_ROW_PER_TXN=%u)", maxlen, MAX_TXN_LEN);
    uint64_t kor, knor;
    memcpy(&kor, hc + TS_C_KOR, 8);
    memcpy(&knor, hc + TS_C_KNOR, 8);
    varying = m ? (kor & knor) : 0;  // a bit set in some key and clear in another
  }
  uint32_t lp = 0;
  while ((1u << lp) < maxlen) lp++;
  const uint64_t per_block = TS_T >> lp;  // txns per workgroup step
  const KeyPack kp = make_keypack(varying);
  const uint64_t tiles = (m + TS_TILE - 1) / TS_TILE;

  const bool prof = profiling;
  CK(hipEventRecord(ev0, stream));
  if (prof) CK(hipEventRecord(pev[0], stream));
  TsArgs A{n, m, d.off, d.keys, d.acctype, ts_dev, lp, (uint4*)ts_arec.p, (uint32_t*)ts_stp.p,
           (ulonglong2*)ts_bnd.p, cnt};
  uint64_t* kb[2] = {(uint64_t*)ts_k[0].p, (uint64_t*)ts_k[1].p};
  uint32_t* vb[2] = {(uint32_t*)ts_v[0].p, (uint32_t*)ts_v[1].p};
  k_ts_prep<<<ts_grid(n, per_block, max_grid), TS_T, 0, stream>>>(A, kp, kb[0], vb[0]);
  CK(hipGetLastError());
  ScanArgs SA{};
  uint64_t heads = 0;
  if (m) {
    const int cur = radix_sort_u64(kb, vb, m, kp.bits, (uint32_t*)cv_scratch.p, stream);
    k_ts_seg<<<ts_grid(m, TS_T, max_grid), TS_T, 0, stream>>>(A, kb[cur], vb[cur], (uint32_t*)ts_stxn.p,
                                                              (uint32_t*)ts_sinfo.p, (uint64_t*)ts_sts.p);
    CK(hipGetLastError());
    // the table gets room for every row of the epoch before any is entered
    CK(hipMemcpyAsync(hmisc, cnt, TS_C_RING * 4, hipMemcpyDeviceToHost, stream));
    CK(hipStreamSynchronize(stream));
    heads = ((const uint32_t*)hmisc)[TS_C_HEADS];
    CR(ts_rows.reserve<TsProbe>(this, ts_rows.rows + heads));
    k_ts_seed<<<ts_grid(m, TS_T, max_grid), TS_T, 0, stream>>>(m, (const uint32_t*)ts_sinfo.p, vb[cur], d.keys,
                                                               (RowSlot*)ts_rows.buf.p, ts_rows.mask(),
                                                               (uint32_t*)ts_hslot.p, cnt);
    CK(hipGetLastError());
    CK(hipMemsetAsync(ts_tdone.p, 0, tiles, stream));
    SA = ScanArgs{m,
                  (const uint32_t*)ts_stxn.p,
                  (const uint32_t*)ts_sinfo.p,
                  (const uint64_t*)ts_sts.p,
                  vb[cur],
                  (const uint32_t*)ts_hslot.p,
                  A.stp,
                  (RowSlot*)ts_rows.buf.p,
                  (Tq*)ts_agg.p,
                  (Tq*)ts_agg.p + tiles,
                  (uint8_t*)ts_tdone.p,
                  A.bnd,
                  nullptr,
                  &cnt[TS_C_ERR]};
  }
  if (prof) CK(hipEventRecord(pev[1], stream));

  // ---- rounds: round r reads the undecided count of round r - 1 from
  // ring[r % TS_RING] (nothing to do at 0) and counts into ring[(r + 1) %
  // TS_RING], which its k_ts_aggscan cleared.  Several rounds are enqueued
  // between host synchronisations; rounds past the fixed point return at once.
  uint32_t r = 1, rounds = 0;
  uint32_t batch = std::min<uint32_t>(2, batch_max);
  bool done = false;
  const unsigned agrid = ts_grid(n, per_block, max_grid);
  while (!done) {
    const uint32_t r0 = r;
    for (uint32_t q = 0; q < batch; q++, r++) {
      const uint32_t* left = &ring[r % TS_RING];
      uint32_t* left_out = &ring[(r + 1) % TS_RING];
      if (m) {
        SA.left = left;
        k_ts_scan<false, false><<<(unsigned)tiles, TS_T, 0, stream>>>(SA);
        k_ts_aggscan<<<1, TS_AGG_T, 0, stream>>>(SA.agg, SA.pre, tiles, left, left_out);
        k_ts_scan<true, false><<<(unsigned)tiles, TS_T, 0, stream>>>(SA);
      } else {
        k_ts_aggscan<<<1, TS_AGG_T, 0, stream>>>(nullptr, nullptr, 0, left, left_out);
      }
      k_ts_advance<<<agrid, TS_T, 0, stream>>>(A, left, left_out);
      if (prof && r == 1) CK(hipEventRecord(pev[2], stream));
    }
    CK(hipGetLastError());
    CK(hipMemcpyAsync(hmisc, ring, TS_RING * 4, hipMemcpyDeviceToHost, stream));
    CK(hipStreamSynchronize(stream));
    const uint32_t* hr = (const uint32_t*)hmisc;
    for (uint32_t q = r0; q < r; q++)
      if (hr[(q + 1) % TS_RING] == 0) {
        rounds = q;
        done = true;
        break;
      }
    if (!done && r > n + 2) return fail(DCC_EIO, "tso: fixed point did not converge");
    batch = std::min<uint32_t>(batch * 2, std::min<uint32_t>(batch_max, TS_RING / 2));
  }
  if (prof) CK(hipEventRecord(pev[3], stream));
  if (m) {  // every txn decided: the rows' new state from each segment's last element
    k_ts_scan<false, true><<<(unsigned)tiles, TS_T, 0, stream>>>(SA);
    k_ts_aggscan<<<1, TS_AGG_T, 0, stream>>>(SA.agg, SA.pre, tiles, nullptr, nullptr);
    k_ts_scan<true, true><<<(unsigned)tiles, TS_T, 0, stream>>>(SA);
  }
  k_ts_rc<<<ts_grid(n, TS_T, max_grid), TS_T, 0, stream>>>(n, A.stp, rc_dev, conf_dev, cnt);
  CK(hipGetLastError());
  if (prof) CK(hipEventRecord(pev[4], stream));
  CK(hipEventRecord(ev1, stream));
  if (!dev) {
    CK(hipMemcpyAsync(out_rc, rc_dev, n, hipMemcpyDeviceToHost, stream));
    if (out_conflict) CK(hipMemcpyAsync(out_conflict, conf_dev, n * 4, hipMemcpyDeviceToHost, stream));
  }
  CK(hipMemcpyAsync(hmisc, cnt, TS_C_RING * 4, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  const uint32_t* hc = (const uint32_t*)hmisc;
  ts_rows.rows += hc[TS_C_ROWS];  // rows entered stay in the table whatever follows
  if (hc[TS_C_ERR] & TS_ERR_FULL) return fail(DCC_EIO, "tso: row table full");
  if (hc[TS_C_ERR] & TS_ERR_STATE) return fail(DCC_EIO, "tso: inconsistent decisions");
  S.rounds = rounds;
  S.n_commit = hc[TS_C_COMMIT];
  S.n_abort = n - hc[TS_C_COMMIT];
  S.nnz_w = hc[TS_C_NWR];
  S.n_readonly = hc[TS_C_RO];
  S.alg_bytes = dcc_tso_alg_bytes(n, m, out_conflict != nullptr);
  CR(es.finish(this, 4));
  if (st) *st = S;
  return DCC_OK;
}

extern "C" uint64_t dcc_tso_alg_bytes(uint64_t n_txn, uint64_t nnz, int with_conflict) {
  // offsets, timestamp per txn, key + access type per access, one 24-B row
  // (key, wts, rts) per access, RC byte, conflict ordinal
  return 4 * (n_txn + 1) + 8 * n_txn + 9 * nnz + 24 * nnz + n_txn + (with_conflict ? 4 * n_txn : 0);
}

extern "C" int dcc_tso_validate_epoch(dcc_ctx* ctx, const dcc_batch* batch, const uint64_t* ts, uint8_t* out_rc,
                                      uint32_t* out_conflict, dcc_stats* out_stats) {
  if (!ctx || !batch || !out_rc || !ts) return DCC_EINVAL;
  dcc_pipe_drain(ctx);  // pipelined OCC epochs in flight complete first
  // a multi-GPU context: the whole epoch on rank 0 (the row table is one GPU's), no collective
  return dcc_on_device(ctx, true,
                       [&](dcc_ctx* s) { return s->tso_epoch(batch, ts, out_rc, out_conflict, out_stats); });
}

extern "C" int dcc_tso_rows_clear(dcc_ctx* ctx) {
  if (!ctx) return DCC_EINVAL;
  return dcc_on_device(ctx, false, [](dcc_ctx* s) { return s->ts_rows.clear(s); });
}

extern "C" int dcc_tso_rows_set(dcc_ctx* ctx, const uint64_t* keys, const uint64_t* wts, const uint64_t* rts,
                                uint64_t n) {
  if (!ctx || (n && (!keys || !wts || !rts))) return DCC_EINVAL;
  return dcc_on_device(ctx, false, [&](dcc_ctx* s) { return s->ts_rows.set<TsProbe>(s, keys, wts, rts, n); });
}

extern "C" int dcc_tso_rows_get(dcc_ctx* ctx, const uint64_t* keys, uint64_t* wts, uint64_t* rts, uint64_t n) {
  if (!ctx || (n && (!keys || !wts || !rts))) return DCC_EINVAL;
  return dcc_on_device(ctx, false, [&](dcc_ctx* s) { return s->ts_rows.get<TsProbe>(s, keys, wts, rts, n); });
}

extern "C" uint64_t dcc_tso_rows_size(const dcc_ctx* ctx) {
  if (ctx && ctx->multi) ctx = dcc_multi_sub((dcc_ctx*)ctx, 0);
  return ctx ? ctx->ts_rows.size() : 0;
}
