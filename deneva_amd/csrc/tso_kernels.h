// The timestamp-ordering epoch that TIMESTAMP (tso.hip) and MVCC (mvcc.hip)
// share: the sort by row, the sorted records, a round of the fixed point over
// segmented prefix maxima and the final pass (tso.hip's head comment has the
// algorithm; the batch check, the aggregate scan and the rounds loop are
// seg_rounds.h's).  What both engines run unchanged is written once
// here; what differs is an engine type E:
//
//   E::MVCC   false  TIMESTAMP: a RD / SCAN meets the committed-writer bound,
//                    the final apply stores the rows' new (wts, rts).
//             true   MVCC: a RD / SCAN never stops or fails its txn (it reads
//                    an older version); the final apply hands every access and
//                    every segment's last element to the engine
//                    (E::access_out, E::row_out) and writes no row itself.
//   E::Scan   k_ts_scan's argument: ScanArgs, or a struct derived from it
//   E::Out    what a thread of the final apply gathers over its accesses for
//             E::flush (MVCC: its late accesses; TIMESTAMP: empty)
//   E::name   the engine, for messages
//
// Included by the engine's .hip after it has defined its tile geometry
// (TS_T threads per workgroup, TS_ITEMS consecutive sorted accesses per
// thread): the kernels are per file, as rowtab.h's.
#pragma once
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
#include "seg_rounds.h"

namespace dcc {
namespace {

constexpr uint32_t TS_TILE = TS_T * TS_ITEMS;     // accesses per scan tile
// error bits next to CHK_ERR_*
constexpr uint32_t TS_ERR_FULL = 4, TS_ERR_STATE = 8, TS_ERR_TS = 16;
// counter words next to SEG_C_*; words 12 .. 15 are the engine's
constexpr uint32_t TS_C_NWR = 2, TS_C_RO = 3, TS_C_COMMIT = 4, TS_C_HEADS = 5, TS_C_ROWS = 6, TS_C_ENGINE = 12,
                   TS_C_RING = 16, TS_C_WORDS = TS_C_RING + SEG_RING;
static_assert(TS_TILE == SegWork::TILE && TS_C_WORDS <= SegWork::C_WORDS, "the shared workspace's sizes");
constexpr uint32_t TS_NONE = ROW_NONE;
// sorted record word: position | type << 8 | head << 16 | last << 17
constexpr uint32_t TS_I_HEAD = 1u << 16, TS_I_LAST = 1u << 17;
// txn word: state << 8 | progress
__device__ inline uint32_t st_state(uint32_t w) { return w >> 8; }
__device__ inline uint32_t st_prog(uint32_t w) { return w & 0xFFu; }

// The persistent rows: rowtab.h's slot {key, a, b} holds a row's wts / rts
// (tab[s].*WTS); MVCC's wts is the row's latest version.
using TsProbe = ProbeMix;
constexpr auto WTS = &RowSlot::a, RTS = &RowSlot::b;

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
    if (slot == TS_NONE) atomicOr(&cnt[SEG_C_ERR], TS_ERR_FULL);
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
static_assert(sizeof(Tq) == SegWork::AGG_BYTES, "the shared workspace's aggregate size");
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
  Tq* pre;          // [tiles] their exclusive prefixes (k_tile_aggscan)
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
// bounds of every access of an undecided txn, in batch order (MVCC: none for a
// RD / SCAN, which passes whatever came before); FINAL: the row's new (wts,
// rts) from the segment's last element, plain stores by one thread per row
// (MVCC: handed to the engine, with every access's exclusive committed-writer
// prefix, which is the newest version installed before it).
template <bool APPLY, bool FINAL, class E>
__global__ __launch_bounds__(TS_T) void k_ts_scan(typename E::Scan A) {
  __shared__ Tq s_w[TS_T / 64];
  constexpr bool NEED_X = APPLY && (!FINAL || E::MVCC);
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
    if (NEED_X) {
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
      if (NEED_X) x[k] = v ? A.sv[base + k] : 0u;
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
  typename E::Out out;  // what the engine gathers over the thread's accesses (MVCC)
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
        if constexpr (E::MVCC) A.bnd[x[k]] = make_ulonglong2(wr ? b.de : 0, wr ? b.pe : 0);
        else A.bnd[x[k]] = make_ulonglong2(wr ? b.de : b.dw, wr ? b.pe : b.pw);
      }
    }
    if constexpr (FINAL && E::MVCC) {
      // the newest version installed before this access: the prefix's, or for
      // a head the row's latest version (nothing writes the rows in this pass)
      uint64_t dw = run.dw;
      if (info[k] & TS_I_HEAD) {
        const uint32_t slot = (uint32_t)e[k].pe;
        dw = slot != TS_NONE ? A.tab[slot].*WTS : 0;
      }
      if (v) E::access_out(A, out, k, x[k], info[k], st[k], ts[k], dw);
    }
    run = TqOp::combine(run, e[k]);
    if (FINAL && v && (info[k] & TS_I_LAST)) {
      const uint32_t slot = (uint32_t)run.pe;
      if (slot == TS_NONE) {
        atomicOr(A.err, TS_ERR_STATE);
      } else if constexpr (E::MVCC) {
        E::row_out(A, base + k, slot, run.dw, run.de);
      } else {
        A.tab[slot].*WTS = run.dw;
        A.tab[slot].*RTS = run.de;
      }
    }
  }
  if constexpr (FINAL && E::MVCC) E::flush(A, out);
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
  if (bad) atomicOr(&cnt[SEG_C_ERR], TS_ERR_STATE);
  block_add<TS_T / 64>(commits, &cnt[TS_C_COMMIT]);
}

// ------------------------------------------------------------------ host
// One epoch's launch state: ts_build fills it, ts_rounds and the engine's
// final pass read it.
struct TsRun {
  uint64_t n = 0, m = 0, tiles = 0, per_block = 0, heads = 0;
  uint32_t lp = 0, rounds = 0, nnz_w = 0;
  unsigned max_grid = 1;
  uint32_t* cnt = nullptr;
  uint32_t* ring = nullptr;
  const uint32_t* sv = nullptr;  // sorted access indices
  TsArgs A{};
  ScanArgs SA{};
};

// The epoch up to the rounds: the batch checked (`more_checks(cnt)` enqueues
// the engine's own next to k_ts_check; a rejected batch ends here, before the
// row table or anything else is written), the accesses sorted by row, the
// sorted records, the row table grown for every head, `before_seed()` (the
// engine's last step that can fail for want of room), every row entered.
// ev0 / pev[0] are recorded behind the check, pev[1] at the end.
template <class E, class Checks, class BeforeSeed>
int ts_build(dcc_ctx* ctx, RowTab& rows, const DevBatch& d, const uint64_t* ts_dev, TsRun& R,
             Checks more_checks, BeforeSeed before_seed) {
  const uint64_t n = d.n, m = d.nnz;
  hipStream_t stream = ctx->stream;
  SegWork& W = ctx->seg;
  uint32_t* cnt = (uint32_t*)W.misc.p;
  R.n = n;
  R.m = m;
  R.cnt = cnt;
  R.ring = cnt + TS_C_RING;
  R.max_grid = (unsigned)ctx->n_cu * 16;

  // reject a malformed batch before anything indexes with its offsets: the row
  // table is untouched by a rejected call
  CK(hipMemsetAsync(cnt, 0, TS_C_WORDS * 4, stream));
  k_batch_check<true><<<launch_grid(std::max(n, m), CHK_T * 4, R.max_grid), CHK_T, 0, stream>>>(
      d.off, n, d.keys, m, cnt);
  CK(hipGetLastError());
  CR(more_checks(cnt));
  CK(hipMemcpyAsync(ctx->hmisc, cnt, TS_C_RING * 4, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  BatchShape shape;
  {
    const uint32_t* hc = (const uint32_t*)ctx->hmisc;
    // a bad timestamp is reported before an over-long txn, as the offsets and the keys are
    if (!(hc[SEG_C_ERR] & (CHK_ERR_OFF | CHK_ERR_KEY)) && (hc[SEG_C_ERR] & TS_ERR_TS))
      return ctx->fail(DCC_EINVAL, "%s: a timestamp is 0 or UINT64_MAX", E::name);
    CR(batch_checked(ctx, hc, m, true, shape));
  }
  const uint32_t lp = shape.lp;
  R.lp = lp;
  R.per_block = TS_T >> lp;  // txns per workgroup step
  const KeyPack kp = make_keypack(shape.varying);
  R.tiles = (m + TS_TILE - 1) / TS_TILE;

  const bool prof = ctx->profiling;
  CK(hipEventRecord(ctx->ev0, stream));
  if (prof) CK(hipEventRecord(ctx->pev[0], stream));
  R.A = TsArgs{n, m, d.off, d.keys, d.acctype, ts_dev, lp, (uint4*)W.arec.p, (uint32_t*)W.stp.p,
               (ulonglong2*)ctx->ts_bnd.p, cnt};
  uint64_t* kb[2] = {(uint64_t*)W.k[0].p, (uint64_t*)W.k[1].p};
  uint32_t* vb[2] = {(uint32_t*)W.v[0].p, (uint32_t*)W.v[1].p};
  k_ts_prep<<<launch_grid(n, R.per_block, R.max_grid), TS_T, 0, stream>>>(R.A, kp, kb[0], vb[0]);
  CK(hipGetLastError());
  R.SA = ScanArgs{};
  if (m) {
    const int cur = radix_sort_u64(kb, vb, m, kp.bits, (uint32_t*)ctx->cv_scratch.p, stream);
    R.sv = vb[cur];
    k_ts_seg<<<launch_grid(m, TS_T, R.max_grid), TS_T, 0, stream>>>(R.A, kb[cur], vb[cur], (uint32_t*)W.stxn.p,
                                                                    (uint32_t*)W.sinfo.p, (uint64_t*)W.sts.p);
    CK(hipGetLastError());
    // the table gets room for every row of the epoch before any is entered
    CK(hipMemcpyAsync(ctx->hmisc, cnt, TS_C_RING * 4, hipMemcpyDeviceToHost, stream));
    CK(hipStreamSynchronize(stream));
    R.heads = ((const uint32_t*)ctx->hmisc)[TS_C_HEADS];
    R.nnz_w = ((const uint32_t*)ctx->hmisc)[TS_C_NWR];
    CR(rows.reserve<TsProbe>(ctx, rows.rows + R.heads));
    CR(before_seed());
    k_ts_seed<<<launch_grid(m, TS_T, R.max_grid), TS_T, 0, stream>>>(m, (const uint32_t*)W.sinfo.p, vb[cur], d.keys,
                                                                     (RowSlot*)rows.buf.p, rows.mask(),
                                                                     (uint32_t*)ctx->ts_hslot.p, cnt);
    CK(hipGetLastError());
    CK(hipMemsetAsync(W.tdone.p, 0, R.tiles, stream));
    R.SA = ScanArgs{m,
                    (const uint32_t*)W.stxn.p,
                    (const uint32_t*)W.sinfo.p,
                    (const uint64_t*)W.sts.p,
                    vb[cur],
                    (const uint32_t*)ctx->ts_hslot.p,
                    R.A.stp,
                    (RowSlot*)rows.buf.p,
                    (Tq*)W.agg.p,
                    (Tq*)W.agg.p + R.tiles,
                    (uint8_t*)W.tdone.p,
                    R.A.bnd,
                    nullptr,
                    &cnt[SEG_C_ERR]};
  }
  if (prof) CK(hipEventRecord(ctx->pev[1], stream));
  return DCC_OK;
}

// The rounds (seg_rounds.h's loop): a round is reduce / scan of the tile
// aggregates, which clears the ring word the round counts into / apply /
// advance.  The lowest undecided txn is decided in every round: at most n of
// them.  `scan(SA)`: the engine's k_ts_scan argument for these launches.
template <class E, class MakeScan>
int ts_rounds(dcc_ctx* ctx, TsRun& R, MakeScan scan) {
  hipStream_t stream = ctx->stream;
  const uint64_t m = R.m, tiles = R.tiles;
  const unsigned agrid = launch_grid(R.n, R.per_block, R.max_grid);
  return rounds_loop(ctx, R.ring, R.n, R.n + 2, E::name, R.rounds,
                     [&](uint32_t, const uint32_t* left, uint32_t* left_out, uint64_t) {
                       if (m) {
                         R.SA.left = left;
                         k_ts_scan<false, false, E><<<(unsigned)tiles, TS_T, 0, stream>>>(scan(R.SA));
                         k_tile_aggscan<TqOp><<<1, SEG_AGG_T, 0, stream>>>(R.SA.agg, R.SA.pre, tiles, left, left_out);
                         k_ts_scan<true, false, E><<<(unsigned)tiles, TS_T, 0, stream>>>(scan(R.SA));
                       } else {
                         k_tile_aggscan<TqOp><<<1, SEG_AGG_T, 0, stream>>>(nullptr, nullptr, 0, left, left_out);
                       }
                       k_ts_advance<<<agrid, TS_T, 0, stream>>>(R.A, left, left_out);
                     });
}

}  // namespace
}  // namespace dcc
