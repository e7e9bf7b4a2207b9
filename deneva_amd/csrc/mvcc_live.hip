// MVCC (CC_ALG MVCC, concurrency_control/row_mvcc.cpp) with txns in flight, as
// two calls over a state the caller keeps in two per-txn arrays (include/dcc.h
// has the model; DESIGN.md §8r the arguments): dcc_mvcc_access_epoch only
// sends requests -- it decides pass, wait or abort for every access, nothing
// finishes inside it -- and dcc_mvcc_finish commits or aborts the txns the
// caller names and promotes buffered reads.  Rows (latest version, rts) and
// the version store are the context's (mvcc.hip).
//
// What the state holds per row: the pending prewrites (ts of every txn that is
// not GONE, once per WR access below its pos, and per WR access at the pos of a
// WAIT txn) and the buffered reads (a WAIT txn at its pos).  Every pending
// prewrite is at or above the row's latest version, so Row_mvcc::conflict
// (:198-240) reduces to
//
//   P_REQ  abort iff ts < rts
//   R_REQ  wait  iff ts > the least pending prewrite ts of the row
//
// and a read that does not wait returns the largest version <= ts and raises
// rts to ts.  Both tests are strict: a txn's own accesses and ties never stop
// it.
//
// Epoch.  The fixed point of waitdie.hip: the accesses sorted stably by (row,
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
// (cap: the txn's first access at or past its progress with a certain stop,
// which stays one.)  An undecided txn walks from its progress over the
// accesses without a possible stop; at the first other access it aborts
// (certain abort), waits (certain wait, no possible abort) or stays undecided
// with its progress there.  The lowest undecided txn sees certain == possible
// in what the others contribute, and its own accesses never stop it, so it is
// decided in every round: at most n_txn + 1 rounds.  The minimum travels as
// the maximum of the complements, which makes the aggregate tso_kernels.h's
// Tq.  Behind the decisions one more scan gives every executed read the row's
// latest version (the fast path: ts >= it) or a search of the store, which no
// epoch changes, and the rows' new rts.
//
// Finish.  The accesses sorted by (row, ts, txn): a buffered read of ts t is
// promoted iff no remaining prewrite below t precedes it, one exclusive
// segmented prefix.  The committing leavers' (key, ts) pairs, compacted in
// that order, are merged into the store's other buffer (mvcc_store.h); a
// promoted read searches the merged store.  Rows, rc, pos and the versions
// out are written by the last two kernels, which return at once if the error
// word is set; the host swaps the store's buffers only if it is clear.
//
// Kernels:  k_live_check / k_live_prep / k_live_advance / k_live_final /
//           k_live_gone  live_txn.h's, with MlLive below: the
//                        check, sort keys / records / txn words, one round of
//                        decisions, rc / pos / conflict ordinals, the leavers
//           k_ml_seg     sorted records, row heads and ends
//           k_ts_seed    (tso_kernels.h) the rows' slots
//           k_ml_scan    per 1,024-access tile: its aggregate, or behind the
//                        scanned aggregates four bits per dynamic access;
//                        final: versions and rts
//           k_ml_fprep / k_ml_fkey / k_ml_inst / k_mv_merge / k_ml_fscan: the
//           finish
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
#include "mvcc_store.h"
#include "tso_kernels.h"

namespace {

static_assert(TS_T == MVS_T, "the store kernels' workgroup");
// live_txn.h's error bits and counter words next to what k_ts_seed and the
// final scan leave in the same words; the engine's own: the versions installed
// (u64), the versions to install, the late reads
static_assert(LV_ERR_STATE == TS_ERR_STATE && LV_ERR_TS == TS_ERR_TS &&
                  !(TS_ERR_FULL & (LV_ERR_STATE | LV_ERR_TS | LV_ERR_RC | LV_ERR_POS | LV_ERR_LEAVE)),
              "the error bits of both headers in one word");
constexpr uint32_t ML_C_NC = TS_C_ENGINE, ML_C_NINST = LV_C_ENGINE, ML_C_LATE = 80;
constexpr uint32_t ML_C_WORDS = SegWork::C_WORDS;
static_assert(lv_word_free(TS_C_HEADS) && lv_word_free(TS_C_ROWS) && lv_word_free(ML_C_NC) &&
                  lv_word_free(ML_C_NC + 1) && LV_C_RING == TS_C_RING && LV_C_WORDS <= ML_C_LATE &&
                  ML_C_LATE < ML_C_WORDS,
              "the shared workspace's counter words");
// record word: position | type << 8 | kind << 10 | TS_I_HEAD | TS_I_LAST.
// Epoch kinds: a static prewrite, a dynamic access.  Finish kinds are bits: a
// version to install, a remaining prewrite, a buffered read.
constexpr uint32_t MK_NONE = 0, MK_PRE = 1, MK_DYN = 2;
constexpr uint32_t FK_INST = 1, FK_PRE = 2, FK_READ = 4;
__device__ inline uint32_t mi_type(uint32_t info) { return (info >> 8) & 3u; }
__device__ inline uint32_t mi_kind(uint32_t info) { return (info >> 10) & 7u; }
// flag byte of a dynamic access: abort / wait under the certain sets, under the possible sets
constexpr uint32_t MF_CA = 1, MF_CW = 2, MF_PA = 4, MF_PW = 8;

// live_txn.h's engine type
struct MlLive {
  static constexpr uint32_t T = TS_T;
  static constexpr const char* name = "mvcc";
  static constexpr bool TS_RANGE = true, WAIT_STAYS = true, ROW_BIT = false, ABORT_POS = true;
  // dynamic from the pos of a RUN txn on; a prewrite: a WR below pos, or at
  // the pos of a WAIT txn; the WR requests are the counted ones
  __device__ static uint32_t record(uint8_t r, uint32_t p, uint32_t a, uint32_t ty, bool& dyn, bool& req) {
    const bool wr = ty == DCC_WR;
    uint32_t kind = MK_NONE;
    if (r == DCC_WD_RUN && a >= p) kind = MK_DYN;
    else if (r != DCC_WD_GONE && wr && (a < p || (r == DCC_RC_WAIT && a == p))) kind = MK_PRE;
    dyn = kind == MK_DYN;
    req = dyn && wr;
    return (ty << 8) | (kind << 10);
  }
  // a possible abort or wait stops; a certain abort aborts, a certain wait
  // without a possible abort waits
  static constexpr uint32_t STOP = MF_PA | MF_PW, CERTAIN = MF_CA | MF_CW;
  __device__ static uint32_t verdict(uint32_t f) {
    return (f & MF_CA) ? LS_ABORT : ((f & MF_CW) && !(f & MF_PA) ? LS_WAIT : LS_UND);
  }
};

// The sorted records: sk / sv are the sorted keys (the packed row above
// `shift` bits) and access indices; the rows counted.
__global__ __launch_bounds__(TS_T) void k_ml_seg(uint64_t m, uint32_t shift, const uint4* __restrict__ arec,
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
struct MlScan {
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
  uint8_t* tdone;   // [tiles] no access of the tile belongs to an undecided txn
  uint8_t* flg;
  const uint32_t* left;  // txns undecided before this round: 0 = nothing to do
  uint32_t* cnt;
  // the final pass: the batch's keys, the store, the versions out (null: not wanted)
  const uint64_t* keys;
  MvStore store;
  uint64_t* vts;
};

// The element an access contributes under the current decisions, in Tq's
// fields: de / pe the executed read's ts (certain / possible), dw / pw the
// complement of the pending prewrite's ts (certain / possible; 0: none).  A
// segment head takes the row's rts in.  FINAL (every txn decided): de alone,
// the head's slot in pe and the row's latest version in dw, which the maximum
// carries to every access of the segment.
template <bool FINAL>
__device__ inline Tq ml_elem(uint32_t info, uint32_t st, uint64_t ts, uint32_t slot, const RowSlot* tab) {
  const uint32_t q = info & 0xFFu, ty = mi_type(info), kind = mi_kind(info);
  const uint32_t state = ls_state(st), p = ls_prog(st), cap = ls_cap(st);
  const bool dyn = kind == MK_DYN, nx = ty != DCC_XP, wr = ty == DCC_WR, und = state == LS_UND;
  const bool cex = dyn && nx && (state == LS_OK || q < p);
  const bool cpr = kind == MK_PRE || (dyn && wr && (state == LS_OK || q < p || (state == LS_WAIT && q == p)));
  const bool pex = cex || (dyn && und && nx && q < cap);
  const bool ppr = cpr || (dyn && und && wr && q <= cap);
  Tq e;
  e.de = cex ? ts : 0;
  e.pe = !FINAL && pex ? ts : 0;
  e.dw = !FINAL && cpr ? ~ts : 0;
  e.pw = !FINAL && ppr ? ~ts : 0;
  e.f = (info & TS_I_HEAD) ? 1u : 0u;
  if (FINAL && e.f) e.pe = slot;
  if (e.f && slot != TS_NONE) {
    const uint64_t r0 = tab[slot].*RTS;
    e.de = max(e.de, r0);
    if (FINAL) e.dw = tab[slot].*WTS;
    else e.pe = max(e.pe, r0);
  }
  return e;
}

// One tile: thread t holds the sorted accesses 4t .. 4t + 3 of it.  !APPLY:
// the tile's aggregate; a tile none of whose accesses belongs to an undecided
// txn keeps its aggregate and is skipped from then on (tdone).  APPLY: behind
// the tile's exclusive prefix, the four bits of every dynamic access of an
// undecided txn at or past its progress, in batch order.  FINAL APPLY (nothing
// if the error word is set): the version of every executed read, and from a
// segment's last element the row's new rts, a plain store by one thread per
// row -- a head that another tile reads meanwhile gives that tile a value
// which only this row's end, not in that tile, would use.
template <bool APPLY, bool FINAL>
__global__ __launch_bounds__(TS_T) void k_ml_scan(MlScan A) {
  __shared__ Tq s_w[TS_T / 64];
  if (!FINAL && (*A.left == 0 || A.tdone[blockIdx.x])) return;
  if (FINAL && APPLY && A.cnt[SEG_C_ERR]) return;
  const uint64_t base = (uint64_t)blockIdx.x * TS_TILE + (uint64_t)threadIdx.x * TS_ITEMS;
  uint32_t info[TS_ITEMS], st[TS_ITEMS];
  uint64_t ts[TS_ITEMS];
  Tq e[TS_ITEMS];
#pragma unroll
  for (uint32_t k = 0; k < TS_ITEMS; k++) {
    const bool v = base + k < A.m;
    info[k] = v ? A.s_info[base + k] : 0u;  // past the end: an identity element
    st[k] = v ? A.stp[A.s_txn[base + k]] : ls_word(LS_STATIC, 0, 0);
    ts[k] = v ? A.s_ts[base + k] : 0;
  }
  Tq mine = TqOp::identity();
#pragma unroll
  for (uint32_t k = 0; k < TS_ITEMS; k++) {
    const uint32_t slot = (info[k] & TS_I_HEAD) ? A.hslot[base + k] : TS_NONE;
    e[k] = ml_elem<FINAL>(info[k], st[k], ts[k], slot, A.tab);
    mine = TqOp::combine(mine, e[k]);
  }
  Tq total;
  const Tq excl = block_excl<TS_T / 64, TqOp>(mine, s_w, total);
  if (!APPLY) {
    bool und = false;
#pragma unroll
    for (uint32_t k = 0; k < TS_ITEMS; k++) und |= ls_state(st[k]) == LS_UND;
    const bool any = !FINAL && __syncthreads_or(und);
    if (threadIdx.x == 0) {
      A.agg[blockIdx.x] = total;
      if (!FINAL && !any) A.tdone[blockIdx.x] = 1;
    }
    return;
  }
  Tq run = TqOp::combine(A.pre[blockIdx.x], excl);
  uint32_t late = 0;
#pragma unroll
  for (uint32_t k = 0; k < TS_ITEMS; k++) {
    const bool v = base + k < A.m;
    const uint32_t q = info[k] & 0xFFu, ty = mi_type(info[k]);
    const bool dyn = mi_kind(info[k]) == MK_DYN, nx = ty != DCC_XP, wr = ty == DCC_WR;
    // the exclusive prefix of a head is the row's state, which its element
    // holds next to its own ts, which never stops it: both tests are strict
    const Tq b = (info[k] & TS_I_HEAD) ? e[k] : run;
    const uint64_t t = ts[k];
    if (!FINAL) {
      if (v && dyn && ls_state(st[k]) == LS_UND && q >= ls_prog(st[k])) {
        A.flg[A.sv[base + k]] = (uint8_t)((wr && t < b.de ? MF_CA : 0u) | (nx && b.dw > ~t ? MF_CW : 0u) |
                                          (wr && t < b.pe ? MF_PA : 0u) | (nx && b.pw > ~t ? MF_PW : 0u));
      }
    } else if (v && dyn && nx && A.vts && (ls_state(st[k]) == LS_OK || q < ls_prog(st[k]))) {
      const uint32_t x = A.sv[base + k];
      uint64_t ver = b.dw;  // the row's latest version
      if (t < ver) {
        const uint64_t K = A.keys[x], p = mv_upper(A.store.k, A.store.t, A.store.n, K, t);
        ver = p && A.store.k[p - 1] == K ? A.store.t[p - 1] : DCC_VTS_BASE;
        late++;
      }
      A.vts[x] = ver;
    }
    run = TqOp::combine(run, e[k]);
    if (FINAL && v && (info[k] & TS_I_LAST)) {
      const uint32_t slot = (uint32_t)run.pe;
      if (slot == TS_NONE) atomicOr(&A.cnt[SEG_C_ERR], TS_ERR_STATE);
      else A.tab[slot].*RTS = run.de;
    }
  }
  if (FINAL) block_add<TS_T / 64>(late, &A.cnt[ML_C_LATE]);
}

// --------------------------------------------------------------- finish
// P lanes per txn: the first sort's key of every access, its txn's packed ts
// (ascending; input order is txn index order, which the stable sorts keep),
// and its record: the WR accesses of a committing leaver install a version;
// a staying txn's prewrites remain, and so does its buffered read.  The
// versions to install counted.
__global__ __launch_bounds__(TS_T) void k_ml_fprep(LiveArgs A, const uint8_t* __restrict__ leave, KeyPack tp,
                                                   uint64_t* __restrict__ ak, uint32_t* __restrict__ av) {
  const Seg g = seg_of(A.lp);
  const uint32_t gpb = TS_T >> A.lp;
  uint32_t ninst = 0;
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
    if (lv && r == DCC_RC_RCOK && wr) kind = FK_INST;
    if (stays && wr && (g.a < p || atp)) kind |= FK_PRE;
    if (stays && atp) kind |= FK_READ;
    ninst += kind == FK_INST;
    ak[x] = keypack_apply(tp, tsv);
    av[x] = (uint32_t)x;
    A.arec[x] = make_uint4((uint32_t)t, g.a | (ty << 8) | (kind << 10), (uint32_t)tsv, (uint32_t)(tsv >> 32));
  }
  block_add<TS_T / 64>(ninst, &A.cnt[ML_C_NINST]);
}

// The second sort's key, in the order the first sort left: the packed row.
__global__ __launch_bounds__(TS_T) void k_ml_fkey(uint64_t m, const uint64_t* __restrict__ keys, KeyPack kp,
                                                  const uint32_t* __restrict__ sv, uint64_t* __restrict__ sk) {
  for (uint64_t s = (uint64_t)blockIdx.x * TS_T + threadIdx.x; s < m; s += (uint64_t)gridDim.x * TS_T)
    sk[s] = keypack_apply(kp, keys[sv[s]]);
}

// One tile of the sorted records per workgroup.  !SCATTER: the tile's number
// of versions to install into toff.  SCATTER: behind the tile's offset (toff
// after k_mv_offsets) those versions in order: (raw key, ts), which is (key,
// ts) order.
template <bool SCATTER>
__global__ __launch_bounds__(TS_T) void k_ml_inst(uint64_t m, const uint32_t* __restrict__ s_info,
                                                  const uint64_t* __restrict__ s_ts,
                                                  const uint32_t* __restrict__ sv,
                                                  const uint64_t* __restrict__ keys, uint64_t* toff,
                                                  uint64_t* __restrict__ ek, uint64_t* __restrict__ et) {
  __shared__ uint32_t s_w[TS_T / 64];
  const uint64_t base = (uint64_t)blockIdx.x * TS_TILE + (uint64_t)threadIdx.x * TS_ITEMS;
  uint32_t mask = 0;
#pragma unroll
  for (uint32_t k = 0; k < TS_ITEMS; k++)
    if (base + k < m && (mi_kind(s_info[base + k]) & FK_INST)) mask |= 1u << k;
  uint32_t total;
  const uint32_t excl = block_excl<TS_T / 64, AddOp<uint32_t>>((uint32_t)__popc(mask), s_w, total);
  if (!SCATTER) {
    if (threadIdx.x == 0) toff[blockIdx.x] = total;
    return;
  }
  uint64_t pos = toff[blockIdx.x] + excl;
#pragma unroll
  for (uint32_t k = 0; k < TS_ITEMS; k++)
    if ((mask >> k) & 1u) {
      ek[pos] = keys[sv[base + k]];
      et[pos] = s_ts[base + k];
      pos++;
    }
}

struct MlFin {
  uint64_t m;
  const uint32_t* s_txn;
  const uint32_t* s_info;
  const uint64_t* s_ts;
  const uint32_t* sv;
  const uint32_t* hslot;
  RowSlot* tab;
  Tq* agg;
  Tq* pre;
  const uint64_t* keys;
  MvStore store;  // the store behind the installs
  uint64_t* vts;  // may be null
  uint8_t* rc;
  uint32_t* pos;
  uint32_t* cnt;
};

// The finish's element: the complement of a remaining prewrite's ts in dw, an
// installed version in pw, the head's slot in pe.
__device__ inline Tq mf_elem(uint32_t info, uint64_t ts, uint32_t slot) {
  const uint32_t kind = mi_kind(info);
  Tq e;
  e.de = 0;
  e.pe = (info & TS_I_HEAD) ? slot : 0;
  e.dw = (kind & FK_PRE) ? ~ts : 0;
  e.pw = (kind & FK_INST) ? ts : 0;
  e.f = (info & TS_I_HEAD) ? 1u : 0u;
  return e;
}

// !APPLY: the tile's aggregate.  APPLY (nothing if the error word is set):
// every buffered read decided from its exclusive prefix -- within a row the
// records are in ts order, so every prewrite below its ts precedes it; a
// promoted one reads the largest version <= its ts, raises the row's rts (an
// atomic maximum: several reads of a row may be promoted) and becomes (RUN,
// pos + 1).  A segment's last element leaves the row's latest version.
template <bool APPLY>
__global__ __launch_bounds__(TS_T) void k_ml_fscan(MlFin A) {
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
    e[k] = mf_elem(info[k], ts[k], (info[k] & TS_I_HEAD) ? A.hslot[base + k] : TS_NONE);
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
    if (v && (mi_kind(info[k]) & FK_READ) && !(b.dw > ~t)) {
      const uint32_t x = A.sv[base + k], i = A.s_txn[base + k];
      if (A.vts && mi_type(info[k]) != DCC_XP) {
        const uint64_t K = A.keys[x], p = mv_upper(A.store.k, A.store.t, A.store.n, K, t);
        A.vts[x] = p && A.store.k[p - 1] == K ? A.store.t[p - 1] : DCC_VTS_BASE;
      }
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

// live_txn.h's open, and behind it what MVCC adds: its own workspaces and the
// versions of a host call on the device (a call writes some entries and leaves
// the others alone).
int ml_open(dcc_ctx* ctx, const dcc_batch* b, const uint64_t* ts_in, uint8_t* rc_io, uint32_t* pos_io, bool finish,
            const uint8_t* leave_in, uint64_t* vts_io, uint64_t* out_left, uint64_t* out_promoted, LiveOpen& O,
            uint64_t*& vts_dev) {
  CR(live_open<MlLive>(ctx, b, ts_in, rc_io, pos_io, finish, leave_in, out_left, out_promoted, O));
  vts_dev = vts_io;
  if (O.A.n == 0) return DCC_OK;
  // live_open has made live_reserve's part with the same sizes, so that part
  // allocates nothing here and the pointers in O.A stay valid
  CR(ctx->mvcc_live_reserve(O.A.n, O.A.m, !O.dev));
  if (vts_io && !O.dev) {
    vts_dev = (uint64_t*)ctx->mv_vts.p;
    if (O.A.m) CK(hipMemcpyAsync(vts_dev, vts_io, O.A.m * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  return DCC_OK;
}

// The rows of the sorted records entered into the table, which gets room for
// every one of them first (`heads`, read back by the caller).
int ml_seed(dcc_ctx* ctx, const LiveOpen& O, uint32_t heads, const uint32_t* sv) {
  hipStream_t stream = ctx->stream;
  RowTab& rows = ctx->mv_rows;
  CR(rows.reserve<TsProbe>(ctx, rows.rows + heads));
  k_ts_seed<<<launch_grid(O.A.m, TS_T, O.max_grid), TS_T, 0, stream>>>(
      O.A.m, (const uint32_t*)ctx->seg.sinfo.p, sv, O.A.keys, (RowSlot*)rows.buf.p, rows.mask(),
      (uint32_t*)ctx->ts_hslot.p, O.A.cnt);
  CK(hipGetLastError());
  return DCC_OK;
}

}  // namespace

int dcc_ctx::mvcc_live_reserve(uint64_t n, uint64_t nnz, bool host_arrays) {
  const uint64_t mm = std::max<uint64_t>(nnz, 1);
  const uint64_t mt = (mm + TS_TILE - 1) / TS_TILE * TS_TILE;
  CR(live_reserve(n, nnz, host_arrays));  // `seg`, the flag bytes, the state arrays of a host call
  CR(ts_hslot.ensure(this, mt * 4, "mvcc head slots"));
  CR(mv_ek.ensure(this, mt * 8, "mvcc epoch version keys"));
  CR(mv_et.ensure(this, mt * 8, "mvcc epoch version timestamps"));
  CR(mv_toff.ensure(this, (mt / TS_TILE + 1) * 8, "mvcc tile offsets"));
  if (host_arrays) CR(mv_vts.ensure(this, mm * 8, "mvcc versions out"));
  return DCC_OK;
}

int dcc_ctx::mvcc_access_epoch(const dcc_batch* b, const uint64_t* ts_in, uint8_t* rc_io, uint32_t* pos_io,
                               uint64_t* vts_io, uint32_t* out_conflict, dcc_stats* st) {
  dcc_ctx* ctx = this;
  LiveOpen O;
  dcc_stats& S = O.es.S;
  uint64_t* vts_dev;
  CR(ml_open(this, b, ts_in, rc_io, pos_io, false, nullptr, vts_io, nullptr, nullptr, O, vts_dev));
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
  k_live_prep<MlLive><<<agrid, TS_T, 0, stream>>>(A, kp, kb[0], vb[0]);
  CK(hipGetLastError());
  MlScan SA{};
  if (m) {
    const int cur = radix_sort_u64(kb, vb, m, kp.bits + 1, (uint32_t*)cv_scratch.p, stream);
    k_ml_seg<<<launch_grid(m, TS_T, max_grid), TS_T, 0, stream>>>(m, 1, A.arec, kb[cur], vb[cur], (uint32_t*)W.stxn.p,
                                                                  (uint32_t*)W.sinfo.p, (uint64_t*)W.sts.p, cnt);
    CK(hipGetLastError());
    // the table gets room for every row of the epoch before any is entered
    CK(hipMemcpyAsync(hmisc, cnt, LV_C_RING * 4, hipMemcpyDeviceToHost, stream));
    CK(hipStreamSynchronize(stream));
    CR(ml_seed(this, O, ((const uint32_t*)hmisc)[TS_C_HEADS], vb[cur]));
    CK(hipMemsetAsync(W.tdone.p, 0, tiles, stream));
    SA = MlScan{m,
                (const uint32_t*)W.stxn.p,
                (const uint32_t*)W.sinfo.p,
                (const uint64_t*)W.sts.p,
                vb[cur],
                (const uint32_t*)ts_hslot.p,
                A.stp,
                (RowSlot*)mv_rows.buf.p,
                (Tq*)W.agg.p,
                (Tq*)W.agg.p + tiles,
                (uint8_t*)W.tdone.p,
                A.flg,
                nullptr,
                cnt,
                A.keys,
                MvStore{(const uint64_t*)mv_sk[mv_cur].p, (const uint64_t*)mv_st[mv_cur].p, mv_n},
                vts_dev};
  }
  if (prof) CK(hipEventRecord(pev[1], stream));

  // The rounds (seg_rounds.h's loop): reduce / scan of the tile aggregates,
  // which clears the ring word the round counts into / apply / advance.  The
  // lowest undecided txn is decided in every round.
  uint32_t rounds = 0;
  CR(rounds_loop(this, cnt + LV_C_RING, n, n + m + 2, MlLive::name, rounds,
                 [&](uint32_t, const uint32_t* left, uint32_t* left_out, uint64_t) {
                   if (m) {
                     SA.left = left;
                     k_ml_scan<false, false><<<(unsigned)tiles, TS_T, 0, stream>>>(SA);
                     k_tile_aggscan<TqOp><<<1, SEG_AGG_T, 0, stream>>>(SA.agg, SA.pre, tiles, left, left_out);
                     k_ml_scan<true, false><<<(unsigned)tiles, TS_T, 0, stream>>>(SA);
                   } else {
                     k_tile_aggscan<TqOp><<<1, SEG_AGG_T, 0, stream>>>(nullptr, nullptr, 0, left, left_out);
                   }
                   k_live_advance<MlLive><<<agrid, TS_T, 0, stream>>>(A, left, left_out);
                 }));

  // rc / pos of a host call stay as they were unless the decisions are sound:
  // the final pass writes the staged copies.  Versions and the rows' rts come
  // behind it and its error word.
  k_live_final<MlLive><<<launch_grid(n, TS_T, max_grid), TS_T, 0, stream>>>(n, A.stp, A.rc, A.pos, conf_dev, cnt);
  if (m) {
    k_ml_scan<false, true><<<(unsigned)tiles, TS_T, 0, stream>>>(SA);
    k_tile_aggscan<TqOp><<<1, SEG_AGG_T, 0, stream>>>(SA.agg, SA.pre, tiles, nullptr, nullptr);
    k_ml_scan<true, true><<<(unsigned)tiles, TS_T, 0, stream>>>(SA);
  }
  CK(hipGetLastError());
  if (prof) CK(hipEventRecord(pev[4], stream));
  CK(hipEventRecord(ev1, stream));
  CK(hipMemcpyAsync(hmisc, cnt, ML_C_WORDS * 4, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  const uint32_t* hc = (const uint32_t*)hmisc;
  mv_rows.rows += hc[TS_C_ROWS];  // rows entered stay in the table whatever follows
  if (hc[SEG_C_ERR] & TS_ERR_FULL) return fail(DCC_EIO, "mvcc: row table full");
  if (hc[SEG_C_ERR] & TS_ERR_STATE) return fail(DCC_EIO, "mvcc: inconsistent decisions");
  S.rounds = rounds;
  S.n_commit = hc[LV_C_OK];
  S.n_abort = hc[LV_C_ABORT];
  S.n_survivors = hc[LV_C_WAIT];
  S.nnz_w = hc[LV_C_NREQ];
  S.n_readonly = hc[LV_C_RO];
  if (!dev) {
    CR(live_copy_back(this, O, rc_io, pos_io, out_conflict));
    if (vts_io && m) CK(hipMemcpyAsync(vts_io, vts_dev, m * 8, hipMemcpyDeviceToHost, stream));
    CK(hipStreamSynchronize(stream));
  }
  S.alg_bytes = dcc_mvcc_access_alg_bytes(n, m, out_conflict != nullptr, vts_io != nullptr);
  CR(O.es.finish(this, 4));
  if (st) *st = S;
  return DCC_OK;
}

int dcc_ctx::mvcc_finish(const dcc_batch* b, const uint64_t* ts_in, uint8_t* rc_io, uint32_t* pos_io,
                         const uint8_t* leave_in, uint64_t* vts_io, uint64_t* out_left, uint64_t* out_promoted,
                         dcc_stats* st) {
  dcc_ctx* ctx = this;
  LiveOpen O;
  dcc_stats& S = O.es.S;
  uint64_t* vts_dev;
  CR(ml_open(this, b, ts_in, rc_io, pos_io, true, leave_in, vts_io, out_left, out_promoted, O, vts_dev));
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
  uint64_t ninst = 0;

  CK(hipEventRecord(ev0, stream));
  if (m) {
    const unsigned mgrid = launch_grid(m, TS_T, max_grid);
    const uint64_t* sk;
    const uint32_t* sv;
    // the records hold what the passes below need of rc / pos / leave: the
    // state is only written behind them (the checked offsets cover every
    // access, so k_ml_fprep writes every key and record)
    CR(live_sort_ts_row(
        this, m, tp.bits, kp.bits,
        [&](uint64_t* ak, uint32_t* av) {
          k_ml_fprep<<<launch_grid(n, O.per_block, max_grid), TS_T, 0, stream>>>(A, O.leave_dev, tp, ak, av);
        },
        [&](const uint32_t* v, uint64_t* k) { k_ml_fkey<<<mgrid, TS_T, 0, stream>>>(m, A.keys, kp, v, k); }, sk, sv));
    k_ml_seg<<<mgrid, TS_T, 0, stream>>>(m, 0, A.arec, sk, sv, (uint32_t*)W.stxn.p, (uint32_t*)W.sinfo.p,
                                         (uint64_t*)W.sts.p, cnt);
    CK(hipGetLastError());
    // room in the row table for every row and in the store's other buffer for
    // every version before anything is kept
    CK(hipMemcpyAsync(hmisc, cnt, ML_C_WORDS * 4, hipMemcpyDeviceToHost, stream));
    CK(hipStreamSynchronize(stream));
    ninst = ((const uint32_t*)hmisc)[ML_C_NINST];
    const uint32_t heads = ((const uint32_t*)hmisc)[TS_C_HEADS];
    if (ninst) CR(mvcc_store_room(mv_n + ninst));
    CR(ml_seed(this, O, heads, sv));
    const uint32_t* s_info = (const uint32_t*)W.sinfo.p;
    const uint64_t* s_ts = (const uint64_t*)W.sts.p;
    MvStore store{(const uint64_t*)mv_sk[mv_cur].p, (const uint64_t*)mv_st[mv_cur].p, mv_n};
    if (ninst) {
      uint64_t* toff = (uint64_t*)mv_toff.p;
      uint64_t* ek = (uint64_t*)mv_ek.p;
      uint64_t* et = (uint64_t*)mv_et.p;
      uint64_t* nc_dev = (uint64_t*)&cnt[ML_C_NC];
      uint64_t* dk = (uint64_t*)mv_sk[mv_cur ^ 1].p;
      uint64_t* dt = (uint64_t*)mv_st[mv_cur ^ 1].p;
      k_ml_inst<false><<<(unsigned)tiles, TS_T, 0, stream>>>(m, s_info, s_ts, sv, A.keys, toff, ek, et);
      k_mv_offsets<<<1, MVS_OFF_T, 0, stream>>>(toff, tiles, nc_dev);
      k_ml_inst<true><<<(unsigned)tiles, TS_T, 0, stream>>>(m, s_info, s_ts, sv, A.keys, toff, ek, et);
      k_mv_merge<<<launch_grid(mv_n + ninst, MVS_T, max_grid), MVS_T, 0, stream>>>(store, ek, et, nc_dev, dk, dt);
      CK(hipGetLastError());
      store = MvStore{dk, dt, mv_n + ninst};
    }
    const MlFin F{m,     (const uint32_t*)W.stxn.p, s_info,  s_ts, sv,    (const uint32_t*)ts_hslot.p,
                  (RowSlot*)mv_rows.buf.p, (Tq*)W.agg.p, (Tq*)W.agg.p + tiles, A.keys, store, vts_dev,
                  A.rc,  A.pos, cnt};
    k_ml_fscan<false><<<(unsigned)tiles, TS_T, 0, stream>>>(F);
    k_tile_aggscan<TqOp><<<1, SEG_AGG_T, 0, stream>>>(F.agg, F.pre, tiles, nullptr, nullptr);
    k_ml_fscan<true><<<(unsigned)tiles, TS_T, 0, stream>>>(F);
    CK(hipGetLastError());
  }
  k_live_gone<MlLive><<<launch_grid(n, TS_T, max_grid), TS_T, 0, stream>>>(n, O.leave_dev, A.rc, &cnt[SEG_C_ERR]);
  CK(hipGetLastError());
  CK(hipEventRecord(ev1, stream));
  CK(hipMemcpyAsync(hmisc, cnt, ML_C_WORDS * 4, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  const uint32_t* hc = (const uint32_t*)hmisc;
  mv_rows.rows += hc[TS_C_ROWS];
  if (hc[SEG_C_ERR] & TS_ERR_FULL) return fail(DCC_EIO, "mvcc: row table full");
  if (hc[SEG_C_ERR] & TS_ERR_STATE) return fail(DCC_EIO, "mvcc: inconsistent finish");
  uint64_t nc;
  memcpy(&nc, hc + ML_C_NC, 8);
  if (nc != ninst) return fail(DCC_EIO, "mvcc: the versions installed do not match their count");
  if (nc) {  // the merged store is the store
    mv_cur ^= 1;
    mv_n += nc;
  }
  if (!O.dev) {
    CR(live_copy_back(this, O, rc_io, pos_io));
    if (vts_io && m) CK(hipMemcpyAsync(vts_io, vts_dev, m * 8, hipMemcpyDeviceToHost, stream));
    CK(hipStreamSynchronize(stream));
  }
  S.n_commit = O.count;
  S.n_survivors = hc[LV_C_PROM];
  S.nnz_w = nc;
  if (out_left) *out_left = S.n_commit;
  if (out_promoted) *out_promoted = S.n_survivors;
  CR(O.es.finish(this, 0));
  if (st) *st = S;
  return DCC_OK;
}

extern "C" uint64_t dcc_mvcc_access_alg_bytes(uint64_t n_txn, uint64_t nnz, int with_conflict, int with_vts) {
  // offsets; ts, rc and pos per txn in; key + access type per access; one
  // 24-B row aggregate (rts, least pending prewrite, latest version) per
  // access; rc and pos per txn out; conflict ordinal; versions out
  return 4 * (n_txn + 1) + 13 * n_txn + 9 * nnz + 24 * nnz + 5 * n_txn + (with_conflict ? 4 * n_txn : 0) +
         (with_vts ? 8 * nnz : 0);
}

extern "C" int dcc_mvcc_access_epoch(dcc_ctx* ctx, const dcc_batch* batch, const uint64_t* ts, uint8_t* rc,
                                     uint32_t* pos, uint64_t* vts, uint32_t* out_conflict, dcc_stats* out_stats) {
  if (!ctx || !batch) return DCC_EINVAL;
  if (!ts || !rc || !pos) return ctx->fail(DCC_EINVAL, "mvcc: null ts / rc / pos");
  dcc_pipe_drain(ctx);  // pipelined OCC epochs in flight complete first
  // a multi-GPU context: the whole epoch on rank 0 (rows and versions are one GPU's), no collective
  return dcc_on_device(ctx, true, [&](dcc_ctx* s) {
    return s->mvcc_access_epoch(batch, ts, rc, pos, vts, out_conflict, out_stats);
  });
}

extern "C" int dcc_mvcc_finish(dcc_ctx* ctx, const dcc_batch* batch, const uint64_t* ts, uint8_t* rc, uint32_t* pos,
                               const uint8_t* leave, uint64_t* vts, uint64_t* out_left, uint64_t* out_promoted,
                               dcc_stats* out_stats) {
  if (!ctx || !batch) return DCC_EINVAL;
  if (!ts || !rc || !pos || !leave) return ctx->fail(DCC_EINVAL, "mvcc: null ts / rc / pos / leave");
  dcc_pipe_drain(ctx);
  return dcc_on_device(ctx, true, [&](dcc_ctx* s) {
    return s->mvcc_finish(batch, ts, rc, pos, leave, vts, out_left, out_promoted, out_stats);
  });
}
