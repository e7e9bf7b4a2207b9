// WAIT_DIE (CC_ALG WAIT_DIE, concurrency_control/row_lock.cpp) as two calls
// over a lock state the caller keeps in two per-txn arrays (include/dcc.h has
// the model): dcc_waitdie_lock_epoch only acquires, dcc_waitdie_release
// removes the txns the caller names and promotes waiters.
//
// Epoch.  Per row, a request of txn i of type t meets four aggregates of the
// entries before it: any owner, any EX owner, the least owner ts, the largest
// waiter ts (row_lock.cpp:69-77, :103-118):
//
//   conflict  an EX owner, or t is EX and any owner, or ts_i < the largest waiter ts
//   die       ts_i > the least owner ts
//
// no conflict: granted; conflict and die: the txn dies, and what it gained in
// this epoch leaves no trace; conflict and no die: it waits there.  Which
// entries exist depends on the decisions of the txns before, so the epoch is
// the fixed point of tso.hip: the accesses are sorted stably by (row, static
// before dynamic) -- static: the owned prefixes and the waiter accesses of the
// input state; dynamic: the accesses at or past pos of the RUN txns, which
// stay in (txn, position) order -- and a round takes the exclusive segmented
// prefix of the aggregates in two flavours:
//
//   certain owner    a static owner; a dynamic access below the stop of a txn
//                    decided RCOK or WAIT
//   possible owner   a certain one; a dynamic access of an undecided txn below
//                    its cap
//   certain waiter   a static waiter; the stop access of a txn decided WAIT
//   possible waiter  a certain one; a dynamic access of an undecided txn from
//                    its progress up to its cap
//
// (cap: the txn's first access with a certain conflict, once one is known --
// a certain conflict stays one, so the txn never owns that access or a later
// one; without it a txn that is sure to stop on a hot row would keep every
// later txn of its other rows undecided)
//
// plus, for the txn itself only, its own dynamic accesses below its progress
// as certain owners (it holds them when it reaches a later access; for the
// others they are only possible until it is decided).  They sit right before
// the access in the sorted order, so they are a second segmented prefix over
// the runs of one txn within a row.  An undecided txn walks from its progress
// over the accesses without a possible conflict; at the first other access it
// dies (certain conflict and certain die), waits (certain conflict, no possible
// die) or stops undecided with its progress there.  Conflict and die are
// monotone in the sets and certain <= true <= possible; for the lowest
// undecided txn only its own accesses between progress and stop are possible
// and not certain, so in every round it is decided or its progress grows: at
// most n_txn + nnz rounds.
//
// Release.  The staying static accesses sorted by (row, owners before waiters,
// descending ts, txn index); one exclusive segmented scan carries (waiters so
// far, any owner, an EX owner, a waiter so far is EX): the waiter is promoted
// iff no EX owner remains and it is the head of a row without owners or every
// waiter up to it, itself included, is SH (row_lock.cpp:317-357).
//
// Kernels:  k_live_check / k_live_prep / k_live_advance / k_live_final /
//           k_live_gone   live_txn.h's, with WdLive below: the
//                         check, sort keys / records / txn words, one round of
//                         decisions, rc / pos / conflict ordinals, the leavers
//           k_wd_seg      sorted records, row heads, own-run heads
//           k_wd_scan     per 1,024-access tile: its aggregate, or behind the
//                         scanned aggregates four bits per dynamic access
//           k_wd_rprep / k_wd_rkey / k_wd_rseg / k_wd_rscan: the release
// No workgroup waits on another.  The offsets' and keys' rules of the check,
// k_tile_aggscan, the rounds loop and the workspaces are seg_rounds.h's
// (DESIGN.md §8n).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "dcc.h"
#include "dcc_ctx.h"
#include "dcc_device.h"
#include "dcc_scan.h"
#include "live_txn.h"
#include "nowait_lanes.h"
#include "occ_kernels.h"
#include "radix_sort.h"
#include "seg_rounds.h"

using namespace dcc;

namespace {

constexpr uint32_t WD_T = 256;      // threads per workgroup
constexpr uint32_t WD_ITEMS = 4;    // consecutive sorted accesses per thread
constexpr uint32_t WD_TILE = WD_T * WD_ITEMS;  // accesses per scan tile
// the rounds loop's ring, SEG_RING of seg_rounds.h, restated as a number here,
// where the tests that size their chains past it read the geometry
constexpr uint32_t WD_RING = 64;
static_assert(WD_RING == SEG_RING, "the ring is seg_rounds.h's");
static_assert(WD_TILE == SegWork::TILE, "the shared workspace's tile");
// record word: position | EX << 8 | kind << 9 | row head << 16 | own-run head << 17
constexpr uint32_t WK_NONE = 0, WK_OWN = 1, WK_WAITER = 2, WK_DYN = 3;
constexpr uint32_t WI_EX = 1u << 8, WI_HEAD = 1u << 16, WI_OHEAD = 1u << 17;
__device__ inline uint32_t wi_kind(uint32_t info) { return (info >> 9) & 3u; }
// flag byte of a dynamic access: conflict / die under the certain sets, under the possible sets
constexpr uint32_t WF_CC = 1, WF_CD = 2, WF_PC = 4, WF_PD = 8;

// live_txn.h's engine type
struct WdLive {
  static constexpr uint32_t T = WD_T;
  static constexpr const char* name = "waitdie";
  static constexpr bool TS_RANGE = false, WAIT_STAYS = false, ROW_BIT = true, ABORT_POS = false;
  // owned below pos, waited at at the pos of a WAIT txn, dynamic from the pos
  // of a RUN txn on; the EX requests are the counted ones
  __device__ static uint32_t record(uint8_t r, uint32_t p, uint32_t a, uint32_t ty, bool& dyn, bool& req) {
    const uint32_t ex = is_ex(ty);
    uint32_t kind = WK_NONE;
    if (r != DCC_WD_GONE) {
      if (a < p) kind = WK_OWN;
      else if (r == DCC_RC_WAIT && a == p) kind = WK_WAITER;
      else if (r == DCC_WD_RUN) kind = WK_DYN;
    }
    dyn = kind == WK_DYN;
    req = dyn && ex;
    return (ex ? WI_EX : 0u) | (kind << 9);
  }
  // a possible conflict stops; on a certain one the txn dies if it dies for
  // certain and waits if it cannot die
  static constexpr uint32_t STOP = WF_PC, CERTAIN = WF_CC;
  __device__ static uint32_t verdict(uint32_t f) {
    return (f & WF_CC) && (f & WF_CD) ? LS_ABORT : ((f & WF_CC) && !(f & WF_PD) ? LS_WAIT : LS_UND);
  }
};

// The sorted records: sk / sv are the sorted keys and access indices.  A row
// head is where the packed row changes; an own-run head is every access that
// does not follow a dynamic access of the same txn in the same row.
__global__ __launch_bounds__(WD_T) void k_wd_seg(uint64_t m, const uint4* __restrict__ arec,
                                                 const uint64_t* __restrict__ sk, const uint32_t* __restrict__ sv,
                                                 uint32_t* __restrict__ s_txn, uint32_t* __restrict__ s_info,
                                                 uint64_t* __restrict__ s_ts) {
  for (uint64_t s = (uint64_t)blockIdx.x * WD_T + threadIdx.x; s < m; s += (uint64_t)gridDim.x * WD_T) {
    const uint64_t k = sk[s] >> 1;
    const bool head = s == 0 || (sk[s - 1] >> 1) != k;
    const uint4 r = arec[sv[s]];
    bool ohead = true;
    if (!head && wi_kind(r.y) == WK_DYN) {
      const uint4 q = arec[sv[s - 1]];
      ohead = wi_kind(q.y) != WK_DYN || q.x != r.x;
    }
    s_txn[s] = r.x;
    s_info[s] = r.y | (head ? WI_HEAD : 0u) | (ohead ? WI_OHEAD : 0u);
    s_ts[s] = (uint64_t)r.z | ((uint64_t)r.w << 32);
  }
}

// ----------------------------------------------------------------- scan
// The segmented aggregates: least owner ts and largest waiter ts, certain and
// possible; in `bits` the row-head flag, any / EX owner (certain, possible),
// the own-run head flag and any / EX own access below the progress.
constexpr uint32_t WB_F = 1, WB_CANY = 2, WB_CEX = 4, WB_PANY = 8, WB_PEX = 16, WB_OF = 32, WB_OANY = 64,
                   WB_OEX = 128;
constexpr uint32_t WB_ROW = WB_CANY | WB_CEX | WB_PANY | WB_PEX, WB_OWN = WB_OF | WB_OANY | WB_OEX;
struct Wq {
  uint64_t cmin, pmin, cw, pw;
  uint32_t bits;
};
static_assert(sizeof(Wq) == SegWork::AGG_BYTES, "the shared workspace's aggregate size");
struct WqOp {
  using T = Wq;
  static constexpr bool has_inverse = false;
  __device__ static Wq identity() { return Wq{~0ull, ~0ull, 0, 0, 0}; }
  __device__ static Wq combine(const Wq& a, const Wq& b) {
    if (b.bits & WB_F) return b;  // a row head is an own-run head too
    const uint32_t row = ((a.bits | b.bits) & WB_ROW) | (a.bits & WB_F);
    const uint32_t own = (b.bits & WB_OF) ? (b.bits & WB_OWN) : ((a.bits | b.bits) & WB_OWN);
    return Wq{min(a.cmin, b.cmin), min(a.pmin, b.pmin), max(a.cw, b.cw), max(a.pw, b.pw), row | own};
  }
  __device__ static Wq shfl_up(const Wq& v, uint32_t d) {
    return Wq{(uint64_t)__shfl_up(v.cmin, d), (uint64_t)__shfl_up(v.pmin, d), (uint64_t)__shfl_up(v.cw, d),
              (uint64_t)__shfl_up(v.pw, d), (uint32_t)__shfl_up(v.bits, d)};
  }
};

struct WdScan {
  uint64_t m;
  const uint32_t* s_txn;
  const uint32_t* s_info;
  const uint64_t* s_ts;
  const uint32_t* sv;
  const uint32_t* stp;
  Wq* agg;          // [tiles] the tile aggregates
  Wq* pre;          // [tiles] their exclusive prefixes (k_tile_aggscan)
  uint8_t* tdone;   // [tiles] no access of the tile belongs to an undecided txn
  uint8_t* flg;
  const uint32_t* left;  // txns undecided before this round: 0 = nothing to do
};

// The element an access contributes under the current decisions.
__device__ inline Wq wd_elem(uint32_t info, uint32_t st, uint64_t ts) {
  const uint32_t q = info & 0xFFu, kind = wi_kind(info), state = ls_state(st), p = ls_prog(st), cap = ls_cap(st);
  const bool dyn = kind == WK_DYN, ex = (info & WI_EX) != 0;
  const bool cown = kind == WK_OWN || (dyn && (state == LS_OK || (state == LS_WAIT && q < p)));
  const bool pown = cown || (dyn && state == LS_UND && q < cap);
  const bool cwait = kind == WK_WAITER || (dyn && state == LS_WAIT && q == p);
  const bool pwait = cwait || (dyn && state == LS_UND && q >= p && q <= cap);
  const bool own = dyn && state == LS_UND && q < p;
  Wq e;
  e.cmin = cown ? ts : ~0ull;
  e.pmin = pown ? ts : ~0ull;
  e.cw = cwait ? ts : 0;
  e.pw = pwait ? ts : 0;
  e.bits = ((info & WI_HEAD) ? WB_F : 0u) | ((info & WI_OHEAD) ? WB_OF : 0u) | (cown ? WB_CANY : 0u) |
           (cown && ex ? WB_CEX : 0u) | (pown ? WB_PANY : 0u) | (pown && ex ? WB_PEX : 0u) |
           (own ? WB_OANY : 0u) | (own && ex ? WB_OEX : 0u);
  return e;
}

// One tile: thread t holds the sorted accesses 4t .. 4t + 3 of it.  !APPLY:
// the tile's aggregate; a tile none of whose accesses belongs to an undecided
// txn keeps its aggregate and is skipped from then on (tdone).  APPLY: behind
// the tile's exclusive prefix, the four bits of every dynamic access of an
// undecided txn at or past its progress, in batch order.
template <bool APPLY>
__global__ __launch_bounds__(WD_T) void k_wd_scan(WdScan A) {
  __shared__ Wq s_w[WD_T / 64];
  if (*A.left == 0 || A.tdone[blockIdx.x]) return;
  const uint64_t base = (uint64_t)blockIdx.x * WD_TILE + (uint64_t)threadIdx.x * WD_ITEMS;
  uint32_t info[WD_ITEMS], st[WD_ITEMS];
  uint64_t ts[WD_ITEMS];
  Wq e[WD_ITEMS];
#pragma unroll
  for (uint32_t k = 0; k < WD_ITEMS; k++) {
    const bool v = base + k < A.m;
    info[k] = v ? A.s_info[base + k] : 0u;  // past the end: an identity element
    st[k] = v ? A.stp[A.s_txn[base + k]] : ls_word(LS_STATIC, 0, 0);
    ts[k] = v ? A.s_ts[base + k] : 0;
  }
  Wq mine = WqOp::identity();
#pragma unroll
  for (uint32_t k = 0; k < WD_ITEMS; k++) {
    e[k] = wd_elem(info[k], st[k], ts[k]);
    mine = WqOp::combine(mine, e[k]);
  }
  Wq total;
  const Wq excl = block_excl<WD_T / 64, WqOp>(mine, s_w, total);
  if (!APPLY) {
    bool und = false;
#pragma unroll
    for (uint32_t k = 0; k < WD_ITEMS; k++) und |= ls_state(st[k]) == LS_UND;
    const bool any = __syncthreads_or(und);
    if (threadIdx.x == 0) {
      A.agg[blockIdx.x] = total;
      if (!any) A.tdone[blockIdx.x] = 1;
    }
    return;
  }
  Wq run = WqOp::combine(A.pre[blockIdx.x], excl);
#pragma unroll
  for (uint32_t k = 0; k < WD_ITEMS; k++) {
    const bool v = base + k < A.m;
    if (v && wi_kind(info[k]) == WK_DYN && ls_state(st[k]) == LS_UND && (info[k] & 0xFFu) >= ls_prog(st[k])) {
      const Wq b = (info[k] & WI_HEAD) ? WqOp::identity() : run;
      const uint32_t ob = (info[k] & WI_OHEAD) ? 0u : b.bits;
      const bool ex = (info[k] & WI_EX) != 0;
      const uint64_t t = ts[k];
      const bool cc = (b.bits & WB_CEX) || (ex && (b.bits & WB_CANY)) || t < b.cw || (ob & WB_OEX) ||
                      (ex && (ob & WB_OANY));
      const bool pc = (b.bits & WB_PEX) || (ex && (b.bits & WB_PANY)) || t < b.pw;
      A.flg[A.sv[base + k]] =
          (uint8_t)((cc ? WF_CC : 0u) | (t > b.cmin ? WF_CD : 0u) | (pc ? WF_PC : 0u) | (t > b.pmin ? WF_PD : 0u));
    }
    run = WqOp::combine(run, e[k]);
  }
}

// -------------------------------------------------------------- release
// P lanes per txn: the first sort's key of every access, the complement of
// its txn's packed ts (descending ts; input order is txn index order, which
// the stable sorts keep), and its record.  Only the accesses a staying txn
// owns or waits at take part; the others become identity elements.
__global__ __launch_bounds__(WD_T) void k_wd_rprep(LiveArgs A, const uint8_t* __restrict__ leave, KeyPack tp,
                                                   uint64_t* __restrict__ ak, uint32_t* __restrict__ av) {
  const Seg g = seg_of(A.lp);
  const uint32_t gpb = WD_T >> A.lp;
  const uint64_t tmask = tp.bits >= 64 ? ~0ull : ((1ull << tp.bits) - 1ull);
  for (uint64_t g0 = (uint64_t)blockIdx.x * gpb; g0 < A.n; g0 += (uint64_t)gridDim.x * gpb) {
    const uint64_t t = g0 + g.gl;
    if (t >= A.n) continue;
    const uint32_t o0 = A.off[t], len = A.off[t + 1] - o0;
    if (g.a >= len) continue;
    const uint8_t r = A.rc[t];
    const uint32_t p = A.pos[t];
    const bool stays = r != DCC_WD_GONE && leave[t] == 0;
    const uint64_t x = (uint64_t)o0 + g.a;
    uint32_t kind = WK_NONE;
    if (stays && g.a < p) kind = WK_OWN;
    else if (stays && r == DCC_RC_WAIT && g.a == p) kind = WK_WAITER;
    const uint32_t ex = is_ex(A.at[x] & 3u);
    ak[x] = ~keypack_apply(tp, A.ts[t]) & tmask;
    av[x] = (uint32_t)x;
    A.arec[x] = make_uint4((uint32_t)t, g.a | (ex ? WI_EX : 0u) | (kind << 9), 0u, 0u);
  }
}

// The second sort's key, in the order the first sort left: (packed row,
// waiter).
__global__ __launch_bounds__(WD_T) void k_wd_rkey(uint64_t m, const uint4* __restrict__ arec,
                                                  const uint64_t* __restrict__ keys, KeyPack kp,
                                                  const uint32_t* __restrict__ sv, uint64_t* __restrict__ sk) {
  for (uint64_t s = (uint64_t)blockIdx.x * WD_T + threadIdx.x; s < m; s += (uint64_t)gridDim.x * WD_T) {
    const uint32_t x = sv[s];
    sk[s] = (keypack_apply(kp, keys[x]) << 1) | (wi_kind(arec[x].y) == WK_WAITER ? 1ull : 0ull);
  }
}

__global__ __launch_bounds__(WD_T) void k_wd_rseg(uint64_t m, const uint4* __restrict__ arec,
                                                  const uint64_t* __restrict__ sk, const uint32_t* __restrict__ sv,
                                                  uint32_t* __restrict__ s_txn, uint32_t* __restrict__ s_info) {
  for (uint64_t s = (uint64_t)blockIdx.x * WD_T + threadIdx.x; s < m; s += (uint64_t)gridDim.x * WD_T) {
    const bool head = s == 0 || (sk[s - 1] >> 1) != (sk[s] >> 1);
    const uint4 r = arec[sv[s]];
    s_txn[s] = r.x;
    s_info[s] = r.y | (head ? WI_HEAD : 0u);
  }
}

// The release's segmented sum: waiters so far in the low word; above it any
// owner, an EX owner, a waiter that is EX; the row-head flag on top.
constexpr uint64_t RB_ANY = 1ull << 32, RB_EX = 1ull << 33, RB_WEX = 1ull << 34, RB_F = 1ull << 63;
struct RqOp {
  using T = uint64_t;
  static constexpr bool has_inverse = false;
  __device__ static uint64_t identity() { return 0; }
  __device__ static uint64_t combine(uint64_t a, uint64_t b) {
    if (b & RB_F) return b;
    return (((a & 0xFFFFFFFFull) + (b & 0xFFFFFFFFull)) & 0xFFFFFFFFull) | ((a | b) & (RB_ANY | RB_EX | RB_WEX)) |
           (a & RB_F);
  }
  __device__ static uint64_t shfl_up(uint64_t v, uint32_t d) { return (uint64_t)__shfl_up(v, d); }
};

struct WdRel {
  uint64_t m;
  const uint32_t* s_txn;
  const uint32_t* s_info;
  uint64_t* agg;
  uint64_t* pre;
  uint8_t* rc;
  uint32_t* pos;
  uint32_t* cnt;
};

// !APPLY: the tile's aggregate.  APPLY: every staying waiter decided from its
// exclusive prefix; a promoted one becomes (RUN, pos + 1).
template <bool APPLY>
__global__ __launch_bounds__(WD_T) void k_wd_rscan(WdRel A) {
  __shared__ uint64_t s_w[WD_T / 64];
  const uint64_t base = (uint64_t)blockIdx.x * WD_TILE + (uint64_t)threadIdx.x * WD_ITEMS;
  uint32_t info[WD_ITEMS];
  uint64_t e[WD_ITEMS];
  uint64_t mine = RqOp::identity();
#pragma unroll
  for (uint32_t k = 0; k < WD_ITEMS; k++) {
    info[k] = base + k < A.m ? A.s_info[base + k] : 0u;
    const uint32_t kind = wi_kind(info[k]);
    const bool ex = (info[k] & WI_EX) != 0;
    e[k] = ((info[k] & WI_HEAD) ? RB_F : 0ull) | (kind == WK_OWN ? RB_ANY | (ex ? RB_EX : 0ull) : 0ull) |
           (kind == WK_WAITER ? 1ull | (ex ? RB_WEX : 0ull) : 0ull);
    mine = RqOp::combine(mine, e[k]);
  }
  uint64_t total;
  const uint64_t excl = block_excl<WD_T / 64, RqOp>(mine, s_w, total);
  if (!APPLY) {
    if (threadIdx.x == 0) A.agg[blockIdx.x] = total;
    return;
  }
  uint64_t run = RqOp::combine(A.pre[blockIdx.x], excl);
  uint32_t prom = 0;
#pragma unroll
  for (uint32_t k = 0; k < WD_ITEMS; k++) {
    if (base + k < A.m && wi_kind(info[k]) == WK_WAITER) {
      const uint64_t b = (info[k] & WI_HEAD) ? 0ull : run;
      const bool ex = (info[k] & WI_EX) != 0;
      const bool head_free = (b & 0xFFFFFFFFull) == 0 && !(b & RB_ANY);
      if (!(b & RB_EX) && (head_free || (!(b & RB_WEX) && !ex))) {
        const uint32_t t = A.s_txn[base + k];
        A.rc[t] = DCC_WD_RUN;
        A.pos[t] += 1;
        prom++;
      }
    }
    run = RqOp::combine(run, e[k]);
  }
  block_add<WD_T / 64>(prom, &A.cnt[LV_C_PROM]);
}

}  // namespace

int dcc_ctx::live_reserve(uint64_t n, uint64_t nnz, bool host_arrays) {
  const uint64_t nn = std::max<uint64_t>(n, 1), mm = std::max<uint64_t>(nnz, 1);
  CR(seg.reserve(this, n, nnz));
  CR(lv_flg.ensure(this, mm, "waitdie access flags"));
  CR(cv_scratch.ensure(this, rs_scratch_words(mm) * 4 + 64, "radix scratch"));
  if (host_arrays) {
    CR(lv_hts.ensure(this, nn * 8, "waitdie timestamps"));
    CR(lv_hrc.ensure(this, nn, "waitdie rc"));
    CR(lv_hpos.ensure(this, nn * 4, "waitdie pos"));
    CR(lv_hleave.ensure(this, nn, "waitdie leave"));
    CR(lv_conf.ensure(this, nn * 4, "waitdie conflicts"));
  }
  return DCC_OK;
}

// The arrays of a call on the device: a host call's are copied into the
// context's staging buffers (and rc / pos copied back by the caller once the
// call has succeeded).
int dcc_ctx::live_stage(uint64_t n, bool dev, const uint64_t* ts, uint8_t* rc, uint32_t* pos,
                           const uint8_t* leave, const uint64_t*& ts_d, uint8_t*& rc_d, uint32_t*& pos_d,
                           const uint8_t*& leave_d) {
  dcc_ctx* ctx = this;
  ts_d = ts;
  rc_d = rc;
  pos_d = pos;
  leave_d = leave;
  if (dev) return DCC_OK;
  CK(hipMemcpyAsync(lv_hts.p, ts, n * 8, hipMemcpyHostToDevice, stream));
  CK(hipMemcpyAsync(lv_hrc.p, rc, n, hipMemcpyHostToDevice, stream));
  CK(hipMemcpyAsync(lv_hpos.p, pos, n * 4, hipMemcpyHostToDevice, stream));
  if (leave) CK(hipMemcpyAsync(lv_hleave.p, leave, n, hipMemcpyHostToDevice, stream));
  ts_d = (const uint64_t*)lv_hts.p;
  rc_d = (uint8_t*)lv_hrc.p;
  pos_d = (uint32_t*)lv_hpos.p;
  leave_d = leave ? (const uint8_t*)lv_hleave.p : nullptr;
  return DCC_OK;
}

int dcc_ctx::waitdie_epoch(const dcc_batch* b, const uint64_t* ts_in, uint8_t* rc_io, uint32_t* pos_io,
                           uint32_t* out_conflict, dcc_stats* st) {
  dcc_ctx* ctx = this;
  LiveOpen O;
  dcc_stats& S = O.es.S;
  CR(live_open<WdLive>(this, b, ts_in, rc_io, pos_io, false, nullptr, nullptr, nullptr, O));
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
  k_live_prep<WdLive><<<agrid, WD_T, 0, stream>>>(A, kp, kb[0], vb[0]);
  CK(hipGetLastError());
  WdScan SA{};
  if (m) {
    const int cur = radix_sort_u64(kb, vb, m, kp.bits + 1, (uint32_t*)cv_scratch.p, stream);
    k_wd_seg<<<launch_grid(m, WD_T, max_grid), WD_T, 0, stream>>>(m, A.arec, kb[cur], vb[cur], (uint32_t*)W.stxn.p,
                                                                  (uint32_t*)W.sinfo.p, (uint64_t*)W.sts.p);
    CK(hipGetLastError());
    CK(hipMemsetAsync(W.tdone.p, 0, tiles, stream));
    SA = WdScan{m,      (const uint32_t*)W.stxn.p, (const uint32_t*)W.sinfo.p, (const uint64_t*)W.sts.p,
                vb[cur], A.stp,                     (Wq*)W.agg.p,               (Wq*)W.agg.p + tiles,
                (uint8_t*)W.tdone.p, A.flg,        nullptr};
  }
  if (prof) CK(hipEventRecord(pev[1], stream));

  // The rounds (seg_rounds.h's loop): reduce / scan of the tile aggregates,
  // which clears the ring word the round counts into / apply / advance.  The
  // lowest undecided txn is decided or moves its progress in every round.
  uint32_t rounds = 0;
  CR(rounds_loop(this, cnt + LV_C_RING, n, n + m + 2, WdLive::name, rounds,
                 [&](uint32_t, const uint32_t* left, uint32_t* left_out, uint64_t) {
                   if (m) {
                     SA.left = left;
                     k_wd_scan<false><<<(unsigned)tiles, WD_T, 0, stream>>>(SA);
                     k_tile_aggscan<WqOp><<<1, SEG_AGG_T, 0, stream>>>(SA.agg, SA.pre, tiles, left, left_out);
                     k_wd_scan<true><<<(unsigned)tiles, WD_T, 0, stream>>>(SA);
                   } else {
                     k_tile_aggscan<WqOp><<<1, SEG_AGG_T, 0, stream>>>(nullptr, nullptr, 0, left, left_out);
                   }
                   k_live_advance<WdLive><<<agrid, WD_T, 0, stream>>>(A, left, left_out);
                 }));

  // rc / pos of a host call stay as they were unless the decisions are sound:
  // the final pass writes the staged copies
  k_live_final<WdLive><<<launch_grid(n, WD_T, max_grid), WD_T, 0, stream>>>(n, A.stp, A.rc, A.pos, conf_dev, cnt);
  CK(hipGetLastError());
  if (prof) CK(hipEventRecord(pev[4], stream));
  CK(hipEventRecord(ev1, stream));
  CK(hipMemcpyAsync(hmisc, cnt, LV_C_RING * 4, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  const uint32_t* hc = (const uint32_t*)hmisc;
  if (hc[SEG_C_ERR] & LV_ERR_STATE) return fail(DCC_EIO, "waitdie: inconsistent decisions");
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
  S.alg_bytes = dcc_waitdie_alg_bytes(n, m, out_conflict != nullptr);
  CR(O.es.finish(this, 4));
  if (st) *st = S;
  return DCC_OK;
}

int dcc_ctx::waitdie_release(const dcc_batch* b, const uint64_t* ts_in, uint8_t* rc_io, uint32_t* pos_io,
                             const uint8_t* leave_in, uint64_t* out_left, uint64_t* out_promoted,
                             dcc_stats* st) {
  dcc_ctx* ctx = this;
  LiveOpen O;
  dcc_stats& S = O.es.S;
  CR(live_open<WdLive>(this, b, ts_in, rc_io, pos_io, true, leave_in, out_left, out_promoted, O));
  if (O.A.n == 0) {
    if (st) *st = S;
    return DCC_OK;
  }
  const uint64_t n = O.A.n, m = O.A.m, tiles = O.tiles;
  const unsigned max_grid = O.max_grid;
  const KeyPack kp = O.kp, tp = make_keypack(O.tvar);
  const LiveArgs& A = O.A;
  SegWork& W = seg;

  CK(hipEventRecord(ev0, stream));
  if (m) {
    const unsigned mgrid = launch_grid(m, WD_T, max_grid);
    const uint64_t* sk;
    const uint32_t* sv;
    // the records hold what the passes below need of rc / pos / leave: the
    // state is only written behind them (the checked offsets cover every
    // access, so k_wd_rprep writes every key and record)
    CR(live_sort_ts_row(
        this, m, tp.bits, kp.bits + 1,
        [&](uint64_t* ak, uint32_t* av) {
          k_wd_rprep<<<launch_grid(n, O.per_block, max_grid), WD_T, 0, stream>>>(A, O.leave_dev, tp, ak, av);
        },
        [&](const uint32_t* v, uint64_t* k) { k_wd_rkey<<<mgrid, WD_T, 0, stream>>>(m, A.arec, A.keys, kp, v, k); },
        sk, sv));
    k_wd_rseg<<<mgrid, WD_T, 0, stream>>>(m, A.arec, sk, sv, (uint32_t*)W.stxn.p, (uint32_t*)W.sinfo.p);
    CK(hipGetLastError());
    const WdRel R{m,       (const uint32_t*)W.stxn.p, (const uint32_t*)W.sinfo.p, (uint64_t*)W.agg.p,
                  (uint64_t*)W.agg.p + tiles, A.rc,   A.pos,                       A.cnt};
    k_wd_rscan<false><<<(unsigned)tiles, WD_T, 0, stream>>>(R);
    k_tile_aggscan<RqOp><<<1, SEG_AGG_T, 0, stream>>>(R.agg, R.pre, tiles, nullptr, nullptr);
    k_wd_rscan<true><<<(unsigned)tiles, WD_T, 0, stream>>>(R);
    CK(hipGetLastError());
  }
  k_live_gone<WdLive><<<launch_grid(n, WD_T, max_grid), WD_T, 0, stream>>>(n, O.leave_dev, A.rc, nullptr);
  CK(hipGetLastError());
  CK(hipEventRecord(ev1, stream));
  CK(hipMemcpyAsync(hmisc, A.cnt, (LV_C_PROM + 1) * 4, hipMemcpyDeviceToHost, stream));
  CR(live_copy_back(this, O, rc_io, pos_io));
  CK(hipStreamSynchronize(stream));
  const uint32_t* hc = (const uint32_t*)hmisc;
  S.n_commit = O.count;
  S.n_survivors = hc[LV_C_PROM];
  if (out_left) *out_left = S.n_commit;
  if (out_promoted) *out_promoted = S.n_survivors;
  CR(O.es.finish(this, 0));
  if (st) *st = S;
  return DCC_OK;
}

extern "C" uint64_t dcc_waitdie_alg_bytes(uint64_t n_txn, uint64_t nnz, int with_conflict) {
  // offsets; ts, rc and pos per txn in; key + access type per access; one
  // 24-B row aggregate (any / EX owner, least owner ts, largest waiter ts) per
  // access; rc and pos per txn out; conflict ordinal
  return 4 * (n_txn + 1) + 13 * n_txn + 9 * nnz + 24 * nnz + 5 * n_txn + (with_conflict ? 4 * n_txn : 0);
}

extern "C" int dcc_waitdie_lock_epoch(dcc_ctx* ctx, const dcc_batch* batch, const uint64_t* ts, uint8_t* rc,
                                      uint32_t* pos, uint32_t* out_conflict, dcc_stats* out_stats) {
  if (!ctx || !batch || !ts || !rc || !pos) return DCC_EINVAL;
  // a read released inside the epoch would promote waiters mid-epoch: SERIALIZABLE only
  if (batch->flags & (DCC_ISO_READ_COMMITTED | DCC_ISO_READ_UNCOMMITTED))
    return ctx->fail(DCC_ENOTSUP, "waitdie: an isolation level below SERIALIZABLE");
  dcc_pipe_drain(ctx);  // pipelined OCC epochs in flight complete first
  // a multi-GPU context: the whole epoch on rank 0, no collective
  return dcc_on_device(ctx, true,
                       [&](dcc_ctx* s) { return s->waitdie_epoch(batch, ts, rc, pos, out_conflict, out_stats); });
}

extern "C" int dcc_waitdie_release(dcc_ctx* ctx, const dcc_batch* batch, const uint64_t* ts, uint8_t* rc,
                                   uint32_t* pos, const uint8_t* leave, uint64_t* out_left,
                                   uint64_t* out_promoted, dcc_stats* out_stats) {
  if (!ctx || !batch || !ts || !rc || !pos || !leave) return DCC_EINVAL;
  if (batch->flags & (DCC_ISO_READ_COMMITTED | DCC_ISO_READ_UNCOMMITTED))
    return ctx->fail(DCC_ENOTSUP, "waitdie: an isolation level below SERIALIZABLE");
  dcc_pipe_drain(ctx);
  return dcc_on_device(ctx, true, [&](dcc_ctx* s) {
    return s->waitdie_release(batch, ts, rc, pos, leave, out_left, out_promoted, out_stats);
  });
}
