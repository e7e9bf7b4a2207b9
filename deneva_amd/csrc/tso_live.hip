// TIMESTAMP (CC_ALG TIMESTAMP, concurrency_control/row_ts.cpp) with txns in
// flight, as two calls over a state the caller keeps in two per-txn arrays
// (include/dcc.h has the model; DESIGN.md §8t the arguments):
// dcc_tso_access_epoch only sends requests -- it decides pass, wait or abort
// for every access, nothing finishes inside it -- and dcc_tso_finish commits
// or aborts the txns the caller names and promotes buffered reads.  The rows'
// (wts, rts) are the context's TIMESTAMP row table (tso.hip).  It is the MVCC
// engine of mvcc_live.hip without the version store and with the wts
// comparisons.
//
// What the state holds per row: the pending prewrites (ts of every txn that is
// not GONE, once per WR access below its pos, and per WR access at the pos of a
// WAIT txn) and the buffered reads (a WAIT txn at its pos).  Row_ts::access
// (:167-208) is then
//
//   R_REQ  abort iff ts < wts; else wait iff ts > the least pending prewrite
//          ts of the row; else rts = max(rts, ts)
//   P_REQ  abort iff ts < rts or ts < wts; else the prewrite is pending
//
// Every test is strict: a txn's own accesses and ties never stop it.  No epoch
// changes wts, so "this access aborts on wts" is known once the rows are
// seeded: one segmented propagation of the head's wts leaves it as a bit of
// the sorted record (TI_WAB), which every round feeds into the flag byte as a
// certain and possible abort.
//
// Epoch.  The fixed point of mvcc_live.hip: the accesses sorted stably by (row,
// static before dynamic) -- static: the prewrites of the input state; dynamic:
// the accesses at or past pos of the RUN txns, in (txn, position) order -- and
// a round takes the exclusive segmented prefix of (largest executed read ts,
// least pending prewrite ts) in two flavours, the row's rts at the head:
//
//   certain read      a dynamic non-XP access below the stop of a decided txn
//                     (all of an RCOK one) or below an undecided one's progress
//   possible read     a certain one; one of an undecided txn below its cap
//   certain prewrite  a static one; a dynamic WR below the stop of a decided
//                     txn, at it for a WAIT one; below an undecided one's progress
//   possible prewrite a certain one; one of an undecided txn up to its cap
//
// The minimum travels as the maximum of the complements (tso_kernels.h's Tq):
// a prewrite at UINT64_MAX has complement 0, which is "none", and behaves as
// none in the reference too (min_pts is UINT64_MAX either way).  The lowest
// undecided txn sees certain == possible in what the others contribute, so it
// is decided in every round: at most n_txn + 1 rounds.  Behind the decisions
// one more scan leaves the rows' new rts.
//
// Finish.  The accesses sorted by (row, ts, txn): a buffered read of ts t is
// promoted iff no remaining prewrite below t precedes it, one exclusive
// segmented prefix; the same scan's maximum of the committing leavers' ts
// raises wts at the segment's end; a promoted read raises rts (an atomic
// maximum).  Rows, rc and pos are written by the last two kernels, which
// return at once if the error word is set.
//
// Kernels:  k_live_check / k_live_prep / k_live_advance / k_live_final /
//           k_live_gone  live_txn.h's, with TsLive below
//           k_tl_seg     sorted records, row heads and ends
//           k_ts_seed    (tso_kernels.h) the rows' slots
//           k_tl_scan    per 1,024-access tile: its aggregate, or behind the
//                        scanned aggregates: TI_WAB (once), four bits per
//                        dynamic access (a round), the rows' rts (final)
//           k_tl_fprep / k_tl_fkey / k_tl_fscan: the finish
// No workgroup waits on another.
#include <hip/hip_runtime.h>

#include "dcc.h"
#include "dcc_ctx.h"

using namespace dcc;

namespace dcc {
namespace {
constexpr uint32_t TS_T = 256;    // threads per workgroup
constexpr uint32_t TS_ITEMS = 4;  // consecutive sorted accesses per thread
}  // namespace
}  // namespace dcc

#include "live_txn.h"
#include "tso_kernels.h"

namespace {

// live_txn.h's error bits and counter words next to what k_ts_seed and the
// final scan leave in the same words
static_assert(LV_ERR_STATE == TS_ERR_STATE && LV_ERR_TS == TS_ERR_TS &&
                  !(TS_ERR_FULL & (LV_ERR_STATE | LV_ERR_TS | LV_ERR_RC | LV_ERR_POS | LV_ERR_LEAVE)),
              "the error bits of both headers in one word");
static_assert(lv_word_free(TS_C_HEADS) && lv_word_free(TS_C_ROWS) && LV_C_RING == TS_C_RING,
              "the shared workspace's counter words");
// record word: position | type << 8 | kind << 10 | TS_I_HEAD | TS_I_LAST |
// TI_WAB.  Epoch kinds: a static prewrite, a dynamic access.  Finish kinds are
// bits: a committing write, a remaining prewrite, a buffered read.
constexpr uint32_t TK_NONE = 0, TK_PRE = 1, TK_DYN = 2;
constexpr uint32_t FK_COMMIT = 1, FK_PRE = 2, FK_READ = 4;
constexpr uint32_t TI_WAB = 1u << 18;  // a dynamic non-XP access with ts < the row's wts
__device__ inline uint32_t ti_type(uint32_t info) { return (info >> 8) & 3u; }
__device__ inline uint32_t ti_kind(uint32_t info) { return (info >> 10) & 7u; }
// flag byte of a dynamic access: abort / wait under the certain sets, under the possible sets
constexpr uint32_t TF_CA = 1, TF_CW = 2, TF_PA = 4, TF_PW = 8;

// live_txn.h's engine type.  TS_RANGE is false: 0 is an ordinary timestamp, and
// a prewrite at UINT64_MAX behaves as no prewrite here as it does in Row_ts
struct TsLive {
  static constexpr uint32_t T = TS_T;
  static constexpr const char* name = "tso";
  static constexpr bool TS_RANGE = false, WAIT_STAYS = true, ROW_BIT = false, ABORT_POS = true;
  // dynamic from the pos of a RUN txn on; a prewrite: a WR below pos, or at
  // the pos of a WAIT txn; the WR requests are the counted ones
  __device__ static uint32_t record(uint8_t r, uint32_t p, uint32_t a, uint32_t ty, bool& dyn, bool& req) {
    const bool wr = ty == DCC_WR;
    uint32_t kind = TK_NONE;
    if (r == DCC_WD_RUN && a >= p) kind = TK_DYN;
    else if (r != DCC_WD_GONE && wr && (a < p || (r == DCC_RC_WAIT && a == p))) kind = TK_PRE;
    dyn = kind == TK_DYN;
    req = dyn && wr;
    return (ty << 8) | (kind << 10);
  }
  // a possible abort or wait stops; a certain abort aborts, a certain wait
  // without a possible abort waits
  static constexpr uint32_t STOP = TF_PA | TF_PW, CERTAIN = TF_CA | TF_CW;
  __device__ static uint32_t verdict(uint32_t f) {
    return (f & TF_CA) ? LS_ABORT : ((f & TF_CW) && !(f & TF_PA) ? LS_WAIT : LS_UND);
  }
};

// The sorted records: sk / sv are the sorted keys (the packed row above
// `shift` bits) and access indices; the rows counted.
__global__ __launch_bounds__(TS_T) void k_tl_seg(uint64_t m, uint32_t shift, const uint4* __restrict__ arec,
                                                 const uint64_t* __restrict__ sk, const uint32_t* __restrict__ sv,
                                                 uint32_t* __restrict__ s_txn, uint32_t* __restrict__ s_info,
                                                 uint64_t* __restrict__ s_ts, uint32_t* __restrict__ cnt) {
  uint32_t heads = 0;
  for (uint64_t s = (uint64_t)blockIdx.x * TS_T + threadIdx.x; s < m; s += (uint64_t)gridDim.x * TS_T) {
    const uint64_t k = sk[s] >> shift;
    const bool head = s == 0 || (sk[s - 1] >> shift) != k, last = s + 1 == m || (sk[s + 1] >> shift) != k;
    const uint4 r = arec[sv[s]];
    s_txn[s] = r.x;
    s_info[s] = r.y | (head ? TS_I_HEAD : 0u) | (last ? TS_I_LAST : 0u);
    s_ts[s] = (uint64_t)r.z | ((uint64_t)r.w << 32);
    heads += head;
  }
  block_add<TS_T / 64>(heads, &cnt[TS_C_HEADS]);
}

// ----------------------------------------------------------------- scan
struct TlScan {
  uint64_t m;
  const uint32_t* s_txn;
  uint32_t* s_info;  // written by the TL_WTS pass alone
  const uint64_t* s_ts;
  const uint32_t* sv;
  const uint32_t* hslot;
  const uint32_t* stp;
  RowSlot* tab;
  Tq* agg;          // [tiles] the tile aggregates
  Tq* pre;          // [tiles] their exclusive prefixes (k_tile_aggscan)
  uint8_t* tdone;   // [tiles] no access of the tile belongs to an undecided txn
  uint8_t* flg;
  const uint32_t* left;  // txns undecided before this round: 0 = nothing to do
  uint32_t* cnt;
};

// the scan's passes: the rows' wts to every access of the segment (once, behind
// the seed), a round, the rows' rts behind the decisions
enum : int { TL_WTS = 0, TL_ROUND = 1, TL_FINAL = 2 };

// The element an access contributes under the current decisions, in Tq's
// fields: de / pe the executed read's ts (certain / possible), dw / pw the
// complement of the pending prewrite's ts (certain / possible; 0: none).  A
// segment head takes the row's rts in.  TL_FINAL (every txn decided): de
// alone, the head's slot in pe, which the maximum carries to the segment's
// end.  TL_WTS: the head's wts in dw and nothing else.
template <int PASS>
__device__ inline Tq tl_elem(uint32_t info, uint32_t st, uint64_t ts, uint32_t slot, const RowSlot* tab) {
  Tq e{0, 0, 0, 0, (info & TS_I_HEAD) ? 1u : 0u};
  if (PASS == TL_WTS) {
    if (e.f && slot != TS_NONE) e.dw = tab[slot].*WTS;
    return e;
  }
  const uint32_t q = info & 0xFFu, ty = ti_type(info), kind = ti_kind(info);
  const uint32_t state = ls_state(st), p = ls_prog(st), cap = ls_cap(st);
  const bool dyn = kind == TK_DYN, nx = ty != DCC_XP, wr = ty == DCC_WR, und = state == LS_UND;
  const bool cex = dyn && nx && (state == LS_OK || q < p);
  const bool cpr = kind == TK_PRE || (dyn && wr && (state == LS_OK || q < p || (state == LS_WAIT && q == p)));
  const bool pex = cex || (dyn && und && nx && q < cap);
  const bool ppr = cpr || (dyn && und && wr && q <= cap);
  constexpr bool FINAL = PASS == TL_FINAL;
  e.de = cex ? ts : 0;
  e.pe = !FINAL && pex ? ts : 0;
  e.dw = !FINAL && cpr ? ~ts : 0;
  e.pw = !FINAL && ppr ? ~ts : 0;
  if (FINAL && e.f) e.pe = slot;
  if (e.f && slot != TS_NONE) {
    const uint64_t r0 = tab[slot].*RTS;
    e.de = max(e.de, r0);
    if (!FINAL) e.pe = max(e.pe, r0);
  }
  return e;
}

// One tile: thread t holds the sorted accesses 4t .. 4t + 3 of it.  !APPLY:
// the tile's aggregate; in a round a tile none of whose accesses belongs to an
// undecided txn keeps its aggregate and is skipped from then on (tdone).
// APPLY, TL_WTS: TI_WAB of every dynamic non-XP access, from the row's wts in
// its prefix.  APPLY, TL_ROUND: behind the tile's exclusive prefix, the four
// bits of every dynamic access of an undecided txn at or past its progress, in
// batch order.  APPLY, TL_FINAL (nothing if the error word is set): from a
// segment's last element the row's new rts, a plain store by one thread per
// row -- a head that another tile reads meanwhile gives that tile a value
// which only this row's end, not in that tile, would use.
template <bool APPLY, int PASS>
__global__ __launch_bounds__(TS_T) void k_tl_scan(TlScan A) {
  __shared__ Tq s_w[TS_T / 64];
  if (PASS == TL_ROUND && (*A.left == 0 || A.tdone[blockIdx.x])) return;
  if (PASS == TL_FINAL && A.cnt[SEG_C_ERR]) return;
  const uint64_t base = (uint64_t)blockIdx.x * TS_TILE + (uint64_t)threadIdx.x * TS_ITEMS;
  uint32_t info[TS_ITEMS], st[TS_ITEMS];
  uint64_t ts[TS_ITEMS];
  Tq e[TS_ITEMS];
#pragma unroll
  for (uint32_t k = 0; k < TS_ITEMS; k++) {
    const bool v = base + k < A.m;
    info[k] = v ? A.s_info[base + k] : 0u;  // past the end: an identity element
    st[k] = v && PASS != TL_WTS ? A.stp[A.s_txn[base + k]] : ls_word(LS_STATIC, 0, 0);
    ts[k] = v ? A.s_ts[base + k] : 0;
  }
  Tq mine = TqOp::identity();
#pragma unroll
  for (uint32_t k = 0; k < TS_ITEMS; k++) {
    const uint32_t slot = (info[k] & TS_I_HEAD) ? A.hslot[base + k] : TS_NONE;
    e[k] = tl_elem<PASS>(info[k], st[k], ts[k], slot, A.tab);
    mine = TqOp::combine(mine, e[k]);
  }
  Tq total;
  const Tq excl = block_excl<TS_T / 64, TqOp>(mine, s_w, total);
  if (!APPLY) {
    bool und = false;
#pragma unroll
    for (uint32_t k = 0; k < TS_ITEMS; k++) und |= ls_state(st[k]) == LS_UND;
    const bool any = PASS == TL_ROUND && __syncthreads_or(und);
    if (threadIdx.x == 0) {
      A.agg[blockIdx.x] = total;
      if (PASS == TL_ROUND && !any) A.tdone[blockIdx.x] = 1;
    }
    return;
  }
  Tq run = TqOp::combine(A.pre[blockIdx.x], excl);
#pragma unroll
  for (uint32_t k = 0; k < TS_ITEMS; k++) {
    const bool v = base + k < A.m;
    const uint32_t q = info[k] & 0xFFu, ty = ti_type(info[k]);
    const bool dyn = ti_kind(info[k]) == TK_DYN, nx = ty != DCC_XP, wr = ty == DCC_WR;
    // the exclusive prefix of a head is the row's state, which its element
    // holds next to its own ts, which never stops it: every test is strict
    const Tq b = (info[k] & TS_I_HEAD) ? e[k] : run;
    const uint64_t t = ts[k];
    if (PASS == TL_WTS) {
      if (v && dyn && nx && t < b.dw) A.s_info[base + k] = info[k] | TI_WAB;
    } else if (PASS == TL_ROUND) {
      if (v && dyn && ls_state(st[k]) == LS_UND && q >= ls_prog(st[k])) {
        const bool wab = (info[k] & TI_WAB) != 0;
        A.flg[A.sv[base + k]] =
            (uint8_t)((wab || (wr && t < b.de) ? TF_CA : 0u) | (nx && b.dw > ~t ? TF_CW : 0u) |
                      (wab || (wr && t < b.pe) ? TF_PA : 0u) | (nx && b.pw > ~t ? TF_PW : 0u));
      }
    }
    run = TqOp::combine(run, e[k]);
    if (PASS == TL_FINAL && v && (info[k] & TS_I_LAST)) {
      const uint32_t slot = (uint32_t)run.pe;
      if (slot == TS_NONE) atomicOr(&A.cnt[SEG_C_ERR], TS_ERR_STATE);
      else A.tab[slot].*RTS = run.de;
    }
  }
}

// --------------------------------------------------------------- finish
// P lanes per txn: the first sort's key of every access, its txn's packed ts
// (ascending; input order is txn index order, which the stable sorts keep),
// and its record: the WR accesses of a committing leaver raise wts; a staying
// txn's prewrites remain, and so does its buffered read.
__global__ __launch_bounds__(TS_T) void k_tl_fprep(LiveArgs A, const uint8_t* __restrict__ leave, KeyPack tp,
                                                   uint64_t* __restrict__ ak, uint32_t* __restrict__ av) {
  const Seg g = seg_of(A.lp);
  const uint32_t gpb = TS_T >> A.lp;
  for (uint64_t g0 = (uint64_t)blockIdx.x * gpb; g0 < A.n; g0 += (uint64_t)gridDim.x * gpb) {
    const uint64_t t = g0 + g.gl;
    if (t >= A.n) continue;
    const uint32_t o0 = A.off[t], len = A.off[t + 1] - o0;
    if (g.a >= len) continue;
    const uint8_t r = A.rc[t];
    const uint32_t p = A.pos[t];
    const bool lv = leave[t] != 0, stays = r != DCC_WD_GONE && !lv;
    const uint64_t x = (uint64_t)o0 + g.a, tsv = A.ts[t];
    const uint32_t ty = A.at[x] & 3u;
    const bool wr = ty == DCC_WR, atp = r == DCC_RC_WAIT && g.a == p;
    uint32_t kind = 0;
    if (lv && r == DCC_RC_RCOK && wr) kind = FK_COMMIT;
    if (stays && wr && (g.a < p || atp)) kind |= FK_PRE;
    if (stays && atp) kind |= FK_READ;
    ak[x] = keypack_apply(tp, tsv);
    av[x] = (uint32_t)x;
    A.arec[x] = make_uint4((uint32_t)t, g.a | (ty << 8) | (kind << 10), (uint32_t)tsv, (uint32_t)(tsv >> 32));
  }
}

// The second sort's key, in the order the first sort left: the packed row.
__global__ __launch_bounds__(TS_T) void k_tl_fkey(uint64_t m, const uint64_t* __restrict__ keys, KeyPack kp,
                                                  const uint32_t* __restrict__ sv, uint64_t* __restrict__ sk) {
  for (uint64_t s = (uint64_t)blockIdx.x * TS_T + threadIdx.x; s < m; s += (uint64_t)gridDim.x * TS_T)
    sk[s] = keypack_apply(kp, keys[sv[s]]);
}

struct TlFin {
  uint64_t m;
  const uint32_t* s_txn;
  const uint32_t* s_info;
  const uint64_t* s_ts;
  const uint32_t* hslot;
  RowSlot* tab;
  Tq* agg;
  Tq* pre;
  uint8_t* rc;
  uint32_t* pos;
  uint32_t* cnt;
};

// The finish's element: the complement of a remaining prewrite's ts in dw, a
// committing write's ts in pw, the head's slot in pe.
__device__ inline Tq tf_elem(uint32_t info, uint64_t ts, uint32_t slot) {
  const uint32_t kind = ti_kind(info);
  Tq e;
  e.de = 0;
  e.pe = (info & TS_I_HEAD) ? slot : 0;
  e.dw = (kind & FK_PRE) ? ~ts : 0;
  e.pw = (kind & FK_COMMIT) ? ts : 0;
  e.f = (info & TS_I_HEAD) ? 1u : 0u;
  return e;
}

// !APPLY: the tile's aggregate.  APPLY (nothing if the error word is set):
// every buffered read decided from its exclusive prefix -- within a row the
// records are in ts order, so every prewrite below its ts precedes it; a
// promoted one raises the row's rts (an atomic maximum: several reads of a row
// may be promoted) and becomes (RUN, pos + 1).  A segment's last element
// raises the row's wts to the largest committing write.
template <bool APPLY>
__global__ __launch_bounds__(TS_T) void k_tl_fscan(TlFin A) {
  __shared__ Tq s_w[TS_T / 64];
  if (APPLY && A.cnt[SEG_C_ERR]) return;
  const uint64_t base = (uint64_t)blockIdx.x * TS_TILE + (uint64_t)threadIdx.x * TS_ITEMS;
  uint32_t info[TS_ITEMS];
  uint64_t ts[TS_ITEMS];
  Tq e[TS_ITEMS];
  Tq mine = TqOp::identity();
#pragma unroll
  for (uint32_t k = 0; k < TS_ITEMS; k++) {
    const bool v = base + k < A.m;
    info[k] = v ? A.s_info[base + k] : 0u;
    ts[k] = v ? A.s_ts[base + k] : 0;
    e[k] = tf_elem(info[k], ts[k], (info[k] & TS_I_HEAD) ? A.hslot[base + k] : TS_NONE);
    mine = TqOp::combine(mine, e[k]);
  }
  Tq total;
  const Tq excl = block_excl<TS_T / 64, TqOp>(mine, s_w, total);
  if (!APPLY) {
    if (threadIdx.x == 0) A.agg[blockIdx.x] = total;
    return;
  }
  Tq run = TqOp::combine(A.pre[blockIdx.x], excl);
  uint32_t prom = 0;
#pragma unroll
  for (uint32_t k = 0; k < TS_ITEMS; k++) {
    const bool v = base + k < A.m;
    const Tq b = (info[k] & TS_I_HEAD) ? e[k] : run;
    const uint64_t t = ts[k];
    run = TqOp::combine(run, e[k]);
    const uint32_t slot = (uint32_t)run.pe;
    if (v && slot == TS_NONE) {
      atomicOr(&A.cnt[SEG_C_ERR], TS_ERR_STATE);
      continue;
    }
    if (v && (ti_kind(info[k]) & FK_READ) && !(b.dw > ~t)) {
      const uint32_t i = A.s_txn[base + k];
      atomicMax((unsigned long long*)&(A.tab[slot].*RTS), (unsigned long long)t);
      A.rc[i] = DCC_WD_RUN;
      A.pos[i] += 1;
      prom++;
    }
    if (v && (info[k] & TS_I_LAST) && run.pw) {
      RowSlot* r = &A.tab[slot];
      r->*WTS = max(r->*WTS, run.pw);
    }
  }
  block_add<TS_T / 64>(prom, &A.cnt[LV_C_PROM]);
}

// live_txn.h's open, and behind it the head slots' room.
int tl_open(dcc_ctx* ctx, const dcc_batch* b, const uint64_t* ts_in, uint8_t* rc_io, uint32_t* pos_io, bool finish,
            const uint8_t* leave_in, uint64_t* out_left, uint64_t* out_promoted, LiveOpen& O) {
  CR(live_open<TsLive>(ctx, b, ts_in, rc_io, pos_io, finish, leave_in, out_left, out_promoted, O));
  if (O.A.n == 0) return DCC_OK;
  // live_open has made live_reserve's part with the same sizes, so that part
  // allocates nothing here and the pointers in O.A stay valid
  return ctx->tso_live_reserve(O.A.n, O.A.m, !O.dev);
}

// The rows of the sorted records entered into the table, which gets room for
// every one of them first (`heads`, read back by the caller).
int tl_seed(dcc_ctx* ctx, const LiveOpen& O, uint32_t heads, const uint32_t* sv) {
  hipStream_t stream = ctx->stream;
  RowTab& rows = ctx->ts_rows;
  CR(rows.reserve<TsProbe>(ctx, rows.rows + heads));
  k_ts_seed<<<launch_grid(O.A.m, TS_T, O.max_grid), TS_T, 0, stream>>>(
      O.A.m, (const uint32_t*)ctx->seg.sinfo.p, sv, O.A.keys, (RowSlot*)rows.buf.p, rows.mask(),
      (uint32_t*)ctx->ts_hslot.p, O.A.cnt);
  CK(hipGetLastError());
  return DCC_OK;
}

}  // namespace

int dcc_ctx::tso_live_reserve(uint64_t n, uint64_t nnz, bool host_arrays) {
  const uint64_t mm = std::max<uint64_t>(nnz, 1);
  const uint64_t mt = (mm + TS_TILE - 1) / TS_TILE * TS_TILE;
  CR(live_reserve(n, nnz, host_arrays));  // `seg`, the flag bytes, the state arrays of a host call
  CR(ts_hslot.ensure(this, mt * 4, "tso head slots"));
  return DCC_OK;
}

int dcc_ctx::tso_access_epoch(const dcc_batch* b, const uint64_t* ts_in, uint8_t* rc_io, uint32_t* pos_io,
                              uint32_t* out_conflict, dcc_stats* st) {
  dcc_ctx* ctx = this;
  LiveOpen O;
  dcc_stats& S = O.es.S;
  CR(tl_open(this, b, ts_in, rc_io, pos_io, false, nullptr, nullptr, nullptr, O));
  if (O.A.n == 0) {
    if (st) *st = S;
    return DCC_OK;
  }
  const uint64_t n = O.A.n, m = O.A.m, tiles = O.tiles;
  const bool dev = O.dev, prof = profiling;
  const unsigned max_grid = O.max_grid;
  const KeyPack kp = O.kp;
  const LiveArgs& A = O.A;
  uint32_t* conf_dev = out_conflict ? (dev ? out_conflict : (uint32_t*)lv_conf.p) : nullptr;
  SegWork& W = seg;
  uint32_t* cnt = A.cnt;

  CK(hipEventRecord(ev0, stream));
  if (prof) CK(hipEventRecord(pev[0], stream));
  uint64_t* kb[2] = {(uint64_t*)W.k[0].p, (uint64_t*)W.k[1].p};
  uint32_t* vb[2] = {(uint32_t*)W.v[0].p, (uint32_t*)W.v[1].p};
  const unsigned agrid = launch_grid(n, O.per_block, max_grid);
  k_live_prep<TsLive><<<agrid, TS_T, 0, stream>>>(A, kp, kb[0], vb[0]);
  CK(hipGetLastError());
  TlScan SA{};
  if (m) {
    const int cur = radix_sort_u64(kb, vb, m, kp.bits + 1, (uint32_t*)cv_scratch.p, stream);
    k_tl_seg<<<launch_grid(m, TS_T, max_grid), TS_T, 0, stream>>>(m, 1, A.arec, kb[cur], vb[cur], (uint32_t*)W.stxn.p,
                                                                  (uint32_t*)W.sinfo.p, (uint64_t*)W.sts.p, cnt);
    CK(hipGetLastError());
    // the table gets room for every row of the epoch before any is entered
    CK(hipMemcpyAsync(hmisc, cnt, LV_C_RING * 4, hipMemcpyDeviceToHost, stream));
    CK(hipStreamSynchronize(stream));
    CR(tl_seed(this, O, ((const uint32_t*)hmisc)[TS_C_HEADS], vb[cur]));
    CK(hipMemsetAsync(W.tdone.p, 0, tiles, stream));
    SA = TlScan{m,
                (const uint32_t*)W.stxn.p,
                (uint32_t*)W.sinfo.p,
                (const uint64_t*)W.sts.p,
                vb[cur],
                (const uint32_t*)ts_hslot.p,
                A.stp,
                (RowSlot*)ts_rows.buf.p,
                (Tq*)W.agg.p,
                (Tq*)W.agg.p + tiles,
                (uint8_t*)W.tdone.p,
                A.flg,
                nullptr,
                cnt};
    // no epoch changes wts: which accesses abort on it is decided here, once
    k_tl_scan<false, TL_WTS><<<(unsigned)tiles, TS_T, 0, stream>>>(SA);
    k_tile_aggscan<TqOp><<<1, SEG_AGG_T, 0, stream>>>(SA.agg, SA.pre, tiles, nullptr, nullptr);
    k_tl_scan<true, TL_WTS><<<(unsigned)tiles, TS_T, 0, stream>>>(SA);
    CK(hipGetLastError());
  }
  if (prof) CK(hipEventRecord(pev[1], stream));

  // The rounds (seg_rounds.h's loop): reduce / scan of the tile aggregates,
  // which clears the ring word the round counts into / apply / advance.  The
  // lowest undecided txn is decided in every round.
  uint32_t rounds = 0;
  CR(rounds_loop(this, cnt + LV_C_RING, n, n + m + 2, TsLive::name, rounds,
                 [&](uint32_t, const uint32_t* left, uint32_t* left_out, uint64_t) {
                   if (m) {
                     SA.left = left;
                     k_tl_scan<false, TL_ROUND><<<(unsigned)tiles, TS_T, 0, stream>>>(SA);
                     k_tile_aggscan<TqOp><<<1, SEG_AGG_T, 0, stream>>>(SA.agg, SA.pre, tiles, left, left_out);
                     k_tl_scan<true, TL_ROUND><<<(unsigned)tiles, TS_T, 0, stream>>>(SA);
                   } else {
                     k_tile_aggscan<TqOp><<<1, SEG_AGG_T, 0, stream>>>(nullptr, nullptr, 0, left, left_out);
                   }
                   k_live_advance<TsLive><<<agrid, TS_T, 0, stream>>>(A, left, left_out);
                 }));

  // rc / pos of a host call stay as they were unless the decisions are sound:
  // the final pass writes the staged copies.  The rows' rts come behind it and
  // its error word.
  k_live_final<TsLive><<<launch_grid(n, TS_T, max_grid), TS_T, 0, stream>>>(n, A.stp, A.rc, A.pos, conf_dev, cnt);
  if (m) {
    k_tl_scan<false, TL_FINAL><<<(unsigned)tiles, TS_T, 0, stream>>>(SA);
    k_tile_aggscan<TqOp><<<1, SEG_AGG_T, 0, stream>>>(SA.agg, SA.pre, tiles, nullptr, nullptr);
    k_tl_scan<true, TL_FINAL><<<(unsigned)tiles, TS_T, 0, stream>>>(SA);
  }
  CK(hipGetLastError());
  if (prof) CK(hipEventRecord(pev[4], stream));
  CK(hipEventRecord(ev1, stream));
  CK(hipMemcpyAsync(hmisc, cnt, LV_C_WORDS * 4, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  const uint32_t* hc = (const uint32_t*)hmisc;
  ts_rows.rows += hc[TS_C_ROWS];  // rows entered stay in the table whatever follows
  if (hc[SEG_C_ERR] & TS_ERR_FULL) return fail(DCC_EIO, "tso: row table full");
  if (hc[SEG_C_ERR] & TS_ERR_STATE) return fail(DCC_EIO, "tso: inconsistent decisions");
  S.rounds = rounds;
  S.n_commit = hc[LV_C_OK];
  S.n_abort = hc[LV_C_ABORT];
  S.n_survivors = hc[LV_C_WAIT];
  S.nnz_w = hc[LV_C_NREQ];
  S.n_readonly = hc[LV_C_RO];
  if (!dev) {
    CR(live_copy_back(this, O, rc_io, pos_io, out_conflict));
    CK(hipStreamSynchronize(stream));
  }
  S.alg_bytes = dcc_tso_access_alg_bytes(n, m, out_conflict != nullptr);
  CR(O.es.finish(this, 4));
  if (st) *st = S;
  return DCC_OK;
}

int dcc_ctx::tso_finish(const dcc_batch* b, const uint64_t* ts_in, uint8_t* rc_io, uint32_t* pos_io,
                        const uint8_t* leave_in, uint64_t* out_left, uint64_t* out_promoted, dcc_stats* st) {
  dcc_ctx* ctx = this;
  LiveOpen O;
  dcc_stats& S = O.es.S;
  CR(tl_open(this, b, ts_in, rc_io, pos_io, true, leave_in, out_left, out_promoted, O));
  if (O.A.n == 0) {
    if (st) *st = S;
    return DCC_OK;
  }
  const uint64_t n = O.A.n, m = O.A.m, tiles = O.tiles;
  const unsigned max_grid = O.max_grid;
  const KeyPack kp = O.kp, tp = make_keypack(O.tvar);
  const LiveArgs& A = O.A;
  SegWork& W = seg;
  uint32_t* cnt = A.cnt;

  CK(hipEventRecord(ev0, stream));
  if (m) {
    const unsigned mgrid = launch_grid(m, TS_T, max_grid);
    const uint64_t* sk;
    const uint32_t* sv;
    // the records hold what the passes below need of rc / pos / leave: the
    // state is only written behind them (the checked offsets cover every
    // access, so k_tl_fprep writes every key and record)
    CR(live_sort_ts_row(
        this, m, tp.bits, kp.bits,
        [&](uint64_t* ak, uint32_t* av) {
          k_tl_fprep<<<launch_grid(n, O.per_block, max_grid), TS_T, 0, stream>>>(A, O.leave_dev, tp, ak, av);
        },
        [&](const uint32_t* v, uint64_t* k) { k_tl_fkey<<<mgrid, TS_T, 0, stream>>>(m, A.keys, kp, v, k); }, sk, sv));
    k_tl_seg<<<mgrid, TS_T, 0, stream>>>(m, 0, A.arec, sk, sv, (uint32_t*)W.stxn.p, (uint32_t*)W.sinfo.p,
                                         (uint64_t*)W.sts.p, cnt);
    CK(hipGetLastError());
    // room in the row table for every row before anything is kept
    CK(hipMemcpyAsync(hmisc, cnt, LV_C_RING * 4, hipMemcpyDeviceToHost, stream));
    CK(hipStreamSynchronize(stream));
    CR(tl_seed(this, O, ((const uint32_t*)hmisc)[TS_C_HEADS], sv));
    const TlFin F{m,
                  (const uint32_t*)W.stxn.p,
                  (const uint32_t*)W.sinfo.p,
                  (const uint64_t*)W.sts.p,
                  (const uint32_t*)ts_hslot.p,
                  (RowSlot*)ts_rows.buf.p,
                  (Tq*)W.agg.p,
                  (Tq*)W.agg.p + tiles,
                  A.rc,
                  A.pos,
                  cnt};
    k_tl_fscan<false><<<(unsigned)tiles, TS_T, 0, stream>>>(F);
    k_tile_aggscan<TqOp><<<1, SEG_AGG_T, 0, stream>>>(F.agg, F.pre, tiles, nullptr, nullptr);
    k_tl_fscan<true><<<(unsigned)tiles, TS_T, 0, stream>>>(F);
    CK(hipGetLastError());
  }
  k_live_gone<TsLive><<<launch_grid(n, TS_T, max_grid), TS_T, 0, stream>>>(n, O.leave_dev, A.rc, &cnt[SEG_C_ERR]);
  CK(hipGetLastError());
  CK(hipEventRecord(ev1, stream));
  CK(hipMemcpyAsync(hmisc, cnt, LV_C_WORDS * 4, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  const uint32_t* hc = (const uint32_t*)hmisc;
  ts_rows.rows += hc[TS_C_ROWS];
  if (hc[SEG_C_ERR] & TS_ERR_FULL) return fail(DCC_EIO, "tso: row table full");
  if (hc[SEG_C_ERR] & TS_ERR_STATE) return fail(DCC_EIO, "tso: inconsistent finish");
  if (!O.dev) {
    CR(live_copy_back(this, O, rc_io, pos_io));
    CK(hipStreamSynchronize(stream));
  }
  S.n_commit = O.count;
  S.n_survivors = hc[LV_C_PROM];
  if (out_left) *out_left = S.n_commit;
  if (out_promoted) *out_promoted = S.n_survivors;
  CR(O.es.finish(this, 0));
  if (st) *st = S;
  return DCC_OK;
}

extern "C" uint64_t dcc_tso_access_alg_bytes(uint64_t n_txn, uint64_t nnz, int with_conflict) {
  // offsets; ts, rc and pos per txn in; key + access type per access; one
  // 24-B row aggregate (rts, least pending prewrite, wts) per access; rc and
  // pos per txn out; conflict ordinal
  return 4 * (n_txn + 1) + 13 * n_txn + 9 * nnz + 24 * nnz + 5 * n_txn + (with_conflict ? 4 * n_txn : 0);
}

extern "C" int dcc_tso_access_epoch(dcc_ctx* ctx, const dcc_batch* batch, const uint64_t* ts, uint8_t* rc,
                                    uint32_t* pos, uint32_t* out_conflict, dcc_stats* out_stats) {
  if (!ctx || !batch) return DCC_EINVAL;
  if (!ts || !rc || !pos) return ctx->fail(DCC_EINVAL, "tso: null ts / rc / pos");
  dcc_pipe_drain(ctx);  // pipelined OCC epochs in flight complete first
  // a multi-GPU context: the whole epoch on rank 0 (the row table is one GPU's), no collective
  return dcc_on_device(ctx, true,
                       [&](dcc_ctx* s) { return s->tso_access_epoch(batch, ts, rc, pos, out_conflict, out_stats); });
}

extern "C" int dcc_tso_finish(dcc_ctx* ctx, const dcc_batch* batch, const uint64_t* ts, uint8_t* rc, uint32_t* pos,
                              const uint8_t* leave, uint64_t* out_left, uint64_t* out_promoted,
                              dcc_stats* out_stats) {
  if (!ctx || !batch) return DCC_EINVAL;
  if (!ts || !rc || !pos || !leave) return ctx->fail(DCC_EINVAL, "tso: null ts / rc / pos / leave");
  dcc_pipe_drain(ctx);
  return dcc_on_device(ctx, true, [&](dcc_ctx* s) {
    return s->tso_finish(batch, ts, rc, pos, leave, out_left, out_promoted, out_stats);
  });
}
