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
// Kernels:  k_wd_check    offsets / keys / longest txn / the (rc, pos) state /
//                         varying bits of the keys and the timestamps
//           k_wd_prep     sort keys, access records, txn words, request counts
//           k_wd_seg      sorted records, row heads, own-run heads
//           k_wd_scan     per 1,024-access tile: its aggregate, or behind the
//                         scanned aggregates four bits per dynamic access
//           k_wd_advance  one round of decisions
//           k_wd_final    rc, pos, conflict ordinals, counts
//           k_wd_rprep / k_wd_rkey / k_wd_rseg / k_wd_rscan / k_wd_rgone: the release
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
// error bits next to CHK_ERR_*
constexpr uint32_t WD_ERR_RC = 4, WD_ERR_POS = 8, WD_ERR_STATE = 16;
// counter words next to SEG_C_*; TOR / TNOR are u64 at words 12, 14
constexpr uint32_t WD_C_NEX = 2, WD_C_RO = 3, WD_C_OK = 4, WD_C_DIE = 5, WD_C_WAIT = 6, WD_C_LEFT = 7,
                   WD_C_TOR = 12, WD_C_TNOR = 14, WD_C_PROM = 16, WD_C_RING = 20,
                   WD_C_WORDS = WD_C_RING + SEG_RING;
static_assert(WD_TILE == SegWork::TILE && WD_C_WORDS <= SegWork::C_WORDS, "the shared workspace's sizes");
// txn word: state << 16 | cap << 8 | progress.  cap: the first access at or
// past the progress of an undecided txn with a certain conflict (WS_NOCAP: none
// known): it owns nothing from there on and waits there at the latest
constexpr uint32_t WS_UND = 0, WS_OK = 1, WS_WAIT = 2, WS_DIE = 3, WS_STATIC = 4, WS_NOCAP = 0xFFu;
__host__ __device__ constexpr uint32_t ws_word(uint32_t state, uint32_t cap, uint32_t prog) {
  return (state << 16) | (cap << 8) | prog;
}
__device__ inline uint32_t ws_state(uint32_t w) { return w >> 16; }
__device__ inline uint32_t ws_cap(uint32_t w) { return (w >> 8) & 0xFFu; }
__device__ inline uint32_t ws_prog(uint32_t w) { return w & 0xFFu; }
// record word: position | EX << 8 | kind << 9 | row head << 16 | own-run head << 17
constexpr uint32_t WK_NONE = 0, WK_OWN = 1, WK_WAITER = 2, WK_DYN = 3;
constexpr uint32_t WI_EX = 1u << 8, WI_HEAD = 1u << 16, WI_OHEAD = 1u << 17;
__device__ inline uint32_t wi_kind(uint32_t info) { return (info >> 9) & 3u; }
// flag byte of a dynamic access: conflict / die under the certain sets, under the possible sets
constexpr uint32_t WF_CC = 1, WF_CD = 2, WF_PC = 4, WF_PD = 8;

__device__ inline bool wd_state_ok(uint8_t rc) {
  return rc == DCC_WD_RUN || rc == DCC_RC_RCOK || rc == DCC_RC_WAIT || rc == DCC_RC_ABORT || rc == DCC_WD_GONE;
}

// ---------------------------------------------------------------- check
// The batch's and the state's validity before anything indexes with them and
// before anything is written; the key bits and timestamp bits that vary; the
// RUN txns (epoch, `leave` null: the ring word round 1 reads) or the leavers
// that were not GONE (release).
__global__ __launch_bounds__(WD_T) void k_wd_check(const uint32_t* __restrict__ off, uint64_t n,
                                                   const uint64_t* __restrict__ keys, uint64_t nnz,
                                                   const uint64_t* __restrict__ ts,
                                                   const uint8_t* __restrict__ rc,
                                                   const uint32_t* __restrict__ pos,
                                                   const uint8_t* __restrict__ leave, uint32_t* __restrict__ cnt) {
  __shared__ uint64_t s_a[WD_T / 64], s_b[WD_T / 64], s_e[WD_T / 64], s_f[WD_T / 64];
  __shared__ uint32_t s_c[WD_T / 64], s_d[WD_T / 64];
  uint32_t len = 0, err = 0, count = 0;
  uint64_t kor = 0, knor = 0, tor = 0, tnor = 0;
  const uint64_t tid = (uint64_t)blockIdx.x * WD_T + threadIdx.x, stride = (uint64_t)gridDim.x * WD_T;
  for (uint64_t t = tid; t < n; t += stride) {
    uint32_t l;
    if (!check_span(off, t, n, nnz, err, len, l)) continue;
    const uint8_t r = rc[t];
    const uint32_t p = pos[t];
    if (!wd_state_ok(r)) err |= WD_ERR_RC;
    else if (r != DCC_WD_GONE && (p > l || (r == DCC_RC_RCOK && p != l) || (r == DCC_RC_WAIT && p >= l)))
      err |= WD_ERR_POS;
    const uint64_t v = ts[t];
    tor |= v;
    tnor |= ~v;
    count += leave ? (leave[t] != 0 && r != DCC_WD_GONE) : (r == DCC_WD_RUN);
  }
  for (uint64_t x = tid; x < nnz; x += stride) check_key(keys[x], err, kor, knor);
  kor = block_reduce<WD_T / 64, OrOp<uint64_t>>(kor, s_a);
  knor = block_reduce<WD_T / 64, OrOp<uint64_t>>(knor, s_b);
  tor = block_reduce<WD_T / 64, OrOp<uint64_t>>(tor, s_e);
  tnor = block_reduce<WD_T / 64, OrOp<uint64_t>>(tnor, s_f);
  len = block_reduce<WD_T / 64, MaxOp<uint32_t>>(len, s_c);
  err = block_reduce<WD_T / 64, OrOp<uint32_t>>(err, s_d);
  if (threadIdx.x == 0) {
    if (kor) atomicOr((unsigned long long*)&cnt[SEG_C_KOR], (unsigned long long)kor);
    if (knor) atomicOr((unsigned long long*)&cnt[SEG_C_KNOR], (unsigned long long)knor);
    if (tor) atomicOr((unsigned long long*)&cnt[WD_C_TOR], (unsigned long long)tor);
    if (tnor) atomicOr((unsigned long long*)&cnt[WD_C_TNOR], (unsigned long long)tnor);
    if (len) atomicMax(&cnt[SEG_C_MAXLEN], len);
    if (err) atomicOr(&cnt[SEG_C_ERR], err);
  }
  block_add<WD_T / 64>(count, leave ? &cnt[WD_C_LEFT] : &cnt[WD_C_RING + 1]);
}

struct WdArgs {
  uint64_t n, m;
  const uint32_t* off;
  const uint64_t* keys;
  const uint8_t* at;
  const uint64_t* ts;
  uint8_t* rc;       // the state, updated in place by the final pass
  uint32_t* pos;
  uint32_t lp;       // log2 lanes per txn
  uint4* arec;       // [m] {txn, record word, ts lo, ts hi} of every access
  uint32_t* stp;     // [n] state << 8 | progress
  uint8_t* flg;      // [m] WF_* of every dynamic access, batch order
  uint32_t* cnt;
};

// P lanes per txn (nowait_lanes.h).  Epoch: the sort key (packed row, dynamic)
// and the record of every access; a RUN txn undecided at progress pos; the EX
// requests and the RUN txns without one counted.
__global__ __launch_bounds__(WD_T) void k_wd_prep(WdArgs A, KeyPack kp, uint64_t* __restrict__ ak,
                                                  uint32_t* __restrict__ av) {
  const Seg g = seg_of(A.lp);
  const uint32_t gpb = WD_T >> A.lp;
  uint32_t ro = 0, nex = 0;
  for (uint64_t g0 = (uint64_t)blockIdx.x * gpb; g0 < A.n; g0 += (uint64_t)gridDim.x * gpb) {
    const uint64_t t = g0 + g.gl;
    const bool tv = t < A.n;
    uint32_t o0 = 0, len = 0, p = 0;
    uint8_t r = DCC_WD_GONE;
    uint64_t tsv = 0;
    if (tv) {
      o0 = A.off[t];
      len = A.off[t + 1] - o0;
      tsv = A.ts[t];
      r = A.rc[t];
      p = A.pos[t];
    }
    const bool v = tv && g.a < len, run = r == DCC_WD_RUN;
    const uint64_t x = (uint64_t)o0 + g.a;
    bool exreq = false;
    if (v) {
      const uint32_t ex = is_ex(A.at[x] & 3u);
      uint32_t kind = WK_NONE;
      if (r != DCC_WD_GONE) {
        if (g.a < p) kind = WK_OWN;
        else if (r == DCC_RC_WAIT && g.a == p) kind = WK_WAITER;
        else if (run) kind = WK_DYN;
      }
      exreq = kind == WK_DYN && ex;
      ak[x] = (keypack_apply(kp, A.keys[x]) << 1) | (kind == WK_DYN ? 1ull : 0ull);
      av[x] = (uint32_t)x;
      A.arec[x] = make_uint4((uint32_t)t, g.a | (ex ? WI_EX : 0u) | (kind << 9), (uint32_t)tsv,
                             (uint32_t)(tsv >> 32));
    }
    const uint64_t xb = ballot64(exreq) & g.mask;
    if (tv && g.a == 0) {
      A.stp[t] = run ? ws_word(WS_UND, WS_NOCAP, p) : ws_word(WS_STATIC, 0, 0);
      if (run) {
        ro += xb ? 0u : 1u;
        nex += (uint32_t)__popcll(xb);
      }
    }
  }
  block_add<WD_T / 64>(ro, &A.cnt[WD_C_RO]);
  __syncthreads();  // block_add's LDS words are read before the next call writes them
  block_add<WD_T / 64>(nex, &A.cnt[WD_C_NEX]);
}

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
  const uint32_t q = info & 0xFFu, kind = wi_kind(info), state = ws_state(st), p = ws_prog(st), cap = ws_cap(st);
  const bool dyn = kind == WK_DYN, ex = (info & WI_EX) != 0;
  const bool cown = kind == WK_OWN || (dyn && (state == WS_OK || (state == WS_WAIT && q < p)));
  const bool pown = cown || (dyn && state == WS_UND && q < cap);
  const bool cwait = kind == WK_WAITER || (dyn && state == WS_WAIT && q == p);
  const bool pwait = cwait || (dyn && state == WS_UND && q >= p && q <= cap);
  const bool own = dyn && state == WS_UND && q < p;
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
    st[k] = v ? A.stp[A.s_txn[base + k]] : ws_word(WS_STATIC, 0, 0);
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
    for (uint32_t k = 0; k < WD_ITEMS; k++) und |= ws_state(st[k]) == WS_UND;
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
    if (v && wi_kind(info[k]) == WK_DYN && ws_state(st[k]) == WS_UND && (info[k] & 0xFFu) >= ws_prog(st[k])) {
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

// One round of decisions.  P lanes per txn, one access per lane: the first
// access at or past the progress with a possible conflict is where the txn
// dies, waits or stops.  Counts the txns it leaves undecided.
__global__ __launch_bounds__(WD_T) void k_wd_advance(WdArgs A, const uint32_t* __restrict__ left,
                                                     uint32_t* left_out) {
  if (*left == 0) return;
  const Seg g = seg_of(A.lp);
  const uint32_t gpb = WD_T >> A.lp;
  uint32_t und_left = 0;
  for (uint64_t g0 = (uint64_t)blockIdx.x * gpb; g0 < A.n; g0 += (uint64_t)gridDim.x * gpb) {
    const uint64_t t = g0 + g.gl;
    const bool tv = t < A.n;
    const uint32_t st = tv ? A.stp[t] : ws_word(WS_STATIC, 0, 0);
    const bool und = tv && ws_state(st) == WS_UND;
    if (!ballot64(und)) continue;  // the wave's txns are decided
    uint32_t o0 = 0, len = 0;
    if (und) {
      o0 = A.off[t];
      len = A.off[t + 1] - o0;
    }
    const bool v = und && g.a < len && g.a >= ws_prog(st);
    const uint32_t f = v ? A.flg[(uint64_t)o0 + g.a] : 0u;
    const uint64_t sb = ballot64((f & WF_PC) != 0) & g.mask;
    const uint64_t ccb = ballot64((f & WF_CC) != 0), cdb = ballot64((f & WF_CD) != 0),
                   pdb = ballot64((f & WF_PD) != 0);
    if (und && g.a == 0) {
      uint32_t w;
      if (!sb) {
        w = ws_word(WS_OK, 0, len);
      } else {
        const uint32_t l = (uint32_t)__builtin_ctzll(sb);
        const bool cc = (ccb >> l) & 1ull, cd = (cdb >> l) & 1ull, pd = (pdb >> l) & 1ull;
        const uint32_t s = cc && cd ? WS_DIE : (cc && !pd ? WS_WAIT : WS_UND);
        const uint64_t cf = ccb & g.mask;  // certain conflicts at or past the progress: they stay certain
        w = ws_word(s, cf ? (uint32_t)__builtin_ctzll(cf) - g.seg0 : WS_NOCAP, l - g.seg0);
        und_left += s == WS_UND ? 1u : 0u;
      }
      A.stp[t] = w;
    }
  }
  block_add<WD_T / 64>(und_left, left_out);
}

// The new state of the RUN txns: (RCOK, len), (WAIT, stop) or (ABORT, the
// input pos); the conflict ordinals; the counts.
__global__ __launch_bounds__(WD_T) void k_wd_final(uint64_t n, const uint32_t* __restrict__ stp,
                                                   uint8_t* __restrict__ rc, uint32_t* __restrict__ pos,
                                                   uint32_t* __restrict__ conflict, uint32_t* __restrict__ cnt) {
  uint32_t ok = 0, die = 0, wait = 0, bad = 0;
  for (uint64_t t = (uint64_t)blockIdx.x * WD_T + threadIdx.x; t < n; t += (uint64_t)gridDim.x * WD_T) {
    const uint32_t st = stp[t], s = ws_state(st), p = ws_prog(st);
    uint32_t c = DCC_ACCESS_NONE;
    if (s == WS_OK) {
      rc[t] = DCC_RC_RCOK;
      pos[t] = p;
      ok++;
    } else if (s == WS_WAIT) {
      rc[t] = DCC_RC_WAIT;
      pos[t] = p;
      c = p;
      wait++;
    } else if (s == WS_DIE) {
      rc[t] = DCC_RC_ABORT;
      c = p;
      die++;
    } else if (s == WS_UND) {
      bad = 1;
    }
    if (conflict) conflict[t] = c;
  }
  if (bad) atomicOr(&cnt[SEG_C_ERR], WD_ERR_STATE);
  block_add<WD_T / 64>(ok, &cnt[WD_C_OK]);
  __syncthreads();
  block_add<WD_T / 64>(die, &cnt[WD_C_DIE]);
  __syncthreads();
  block_add<WD_T / 64>(wait, &cnt[WD_C_WAIT]);
}

// -------------------------------------------------------------- release
// P lanes per txn: the first sort's key of every access, the complement of
// its txn's packed ts (descending ts; input order is txn index order, which
// the stable sorts keep), and its record.  Only the accesses a staying txn
// owns or waits at take part; the others become identity elements.
__global__ __launch_bounds__(WD_T) void k_wd_rprep(WdArgs A, const uint8_t* __restrict__ leave, KeyPack tp,
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
  block_add<WD_T / 64>(prom, &A.cnt[WD_C_PROM]);
}

__global__ __launch_bounds__(WD_T) void k_wd_rgone(uint64_t n, const uint8_t* __restrict__ leave,
                                                   uint8_t* __restrict__ rc) {
  for (uint64_t t = (uint64_t)blockIdx.x * WD_T + threadIdx.x; t < n; t += (uint64_t)gridDim.x * WD_T)
    if (leave[t]) rc[t] = DCC_WD_GONE;
}

// What the check left in the pinned mirror: the rejection, or the batch's
// shape, the timestamp bits that vary and the RUN txns / leavers.
struct WdChecked : BatchShape {
  uint32_t count = 0;
  uint64_t tvar = 0;
};
int wd_checked(dcc_ctx* ctx, const uint32_t* hc, uint64_t n, uint64_t m, bool release, WdChecked& c) {
  const uint32_t err = hc[SEG_C_ERR];
  CR(batch_checked(ctx, hc, m, true, c));
  if (err & WD_ERR_RC) return ctx->fail(DCC_EINVAL, "waitdie: an rc byte is none of the five states");
  if (err & WD_ERR_POS)
    return ctx->fail(DCC_EINVAL, "waitdie: a pos does not fit its state (pos > len, RCOK below len, WAIT at len)");
  uint64_t a, b;
  memcpy(&a, hc + WD_C_TOR, 8);
  memcpy(&b, hc + WD_C_TNOR, 8);
  c.tvar = n ? (a & b) : 0;
  c.count = release ? hc[WD_C_LEFT] : hc[WD_C_RING + 1];
  return DCC_OK;
}

// What a lock epoch and a release share up to ev0: the call's arguments
// checked, the batch and the state arrays on the device, the check, the key
// pack and the lanes' geometry.  A.n == 0 behind a DCC_OK: the empty batch.
struct WdOpen {
  uint64_t per_block = 0, tiles = 0;
  bool dev = false;
  const uint8_t* leave_dev = nullptr;
  unsigned max_grid = 1;
  WdChecked c;
  KeyPack kp{};
  WdArgs A{};  // rc, pos, cnt: the state and the counters on the device
};
int wd_open(dcc_ctx* ctx, const dcc_batch* b, const uint64_t* ts_in, uint8_t* rc_io, uint32_t* pos_io, bool release,
            const uint8_t* leave_in, uint64_t* out_left, uint64_t* out_promoted, WdOpen& O) {
  hipStream_t stream = ctx->stream;
  if (!ts_in || !rc_io || !pos_io) return ctx->fail(DCC_EINVAL, "waitdie: null ts / rc / pos");
  if (release && !leave_in) return ctx->fail(DCC_EINVAL, "waitdie: null leave");
  CR(ctx->check_batch(b, false));  // the offsets are checked on the device (k_wd_check)
  if (ctx->comm_ranks() > 1) return ctx->fail(DCC_ENOTSUP, "waitdie: single-GPU engine");
  O.dev = (b->flags & DCC_DEVICE_PTRS) != 0;
  if (out_left) *out_left = 0;
  if (out_promoted) *out_promoted = 0;
  if (b->n_txn == 0) return DCC_OK;
  DevBatch d;
  CR(ctx->stage_batch(b, d));
  const uint64_t n = d.n, m = d.nnz;
  CR(ctx->waitdie_reserve(n, m, !O.dev));
  const uint64_t* ts_dev;
  uint8_t* rc_dev;
  uint32_t* pos_dev;
  CR(ctx->waitdie_stage(n, O.dev, ts_in, rc_io, pos_io, leave_in, ts_dev, rc_dev, pos_dev, O.leave_dev));
  SegWork& W = ctx->seg;
  uint32_t* cnt = (uint32_t*)W.misc.p;
  O.max_grid = (unsigned)ctx->n_cu * 16;

  // reject a malformed batch or state before anything indexes with it: rc,
  // pos and the outputs are untouched by a rejected call
  CK(hipMemsetAsync(cnt, 0, WD_C_WORDS * 4, stream));
  k_wd_check<<<launch_grid(std::max(n, m), WD_T * 4, O.max_grid), WD_T, 0, stream>>>(
      d.off, n, d.keys, m, ts_dev, rc_dev, pos_dev, O.leave_dev, cnt);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(ctx->hmisc, cnt, WD_C_WORDS * 4, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  CR(wd_checked(ctx, (const uint32_t*)ctx->hmisc, n, m, release, O.c));
  O.kp = make_keypack(O.c.varying);
  if (O.kp.bits > 63) return ctx->fail(DCC_ENOTSUP, "waitdie: the keys vary in all 64 bits");
  O.per_block = WD_T >> O.c.lp;
  O.tiles = (m + WD_TILE - 1) / WD_TILE;
  O.A = WdArgs{n,      m,  d.off, d.keys, d.acctype, ts_dev, rc_dev, pos_dev,
               O.c.lp, (uint4*)W.arec.p, (uint32_t*)W.stp.p, (uint8_t*)ctx->wd_flg.p, cnt};
  return DCC_OK;
}

}  // namespace

int dcc_ctx::waitdie_reserve(uint64_t n, uint64_t nnz, bool host_arrays) {
  const uint64_t nn = std::max<uint64_t>(n, 1), mm = std::max<uint64_t>(nnz, 1);
  CR(seg.reserve(this, n, nnz));
  CR(wd_flg.ensure(this, mm, "waitdie access flags"));
  CR(cv_scratch.ensure(this, rs_scratch_words(mm) * 4 + 64, "radix scratch"));
  if (host_arrays) {
    CR(wd_hts.ensure(this, nn * 8, "waitdie timestamps"));
    CR(wd_hrc.ensure(this, nn, "waitdie rc"));
    CR(wd_hpos.ensure(this, nn * 4, "waitdie pos"));
    CR(wd_hleave.ensure(this, nn, "waitdie leave"));
    CR(wd_conf.ensure(this, nn * 4, "waitdie conflicts"));
  }
  return DCC_OK;
}

// The arrays of a call on the device: a host call's are copied into the
// context's staging buffers (and rc / pos copied back by the caller once the
// call has succeeded).
int dcc_ctx::waitdie_stage(uint64_t n, bool dev, const uint64_t* ts, uint8_t* rc, uint32_t* pos,
                           const uint8_t* leave, const uint64_t*& ts_d, uint8_t*& rc_d, uint32_t*& pos_d,
                           const uint8_t*& leave_d) {
  dcc_ctx* ctx = this;
  ts_d = ts;
  rc_d = rc;
  pos_d = pos;
  leave_d = leave;
  if (dev) return DCC_OK;
  CK(hipMemcpyAsync(wd_hts.p, ts, n * 8, hipMemcpyHostToDevice, stream));
  CK(hipMemcpyAsync(wd_hrc.p, rc, n, hipMemcpyHostToDevice, stream));
  CK(hipMemcpyAsync(wd_hpos.p, pos, n * 4, hipMemcpyHostToDevice, stream));
  if (leave) CK(hipMemcpyAsync(wd_hleave.p, leave, n, hipMemcpyHostToDevice, stream));
  ts_d = (const uint64_t*)wd_hts.p;
  rc_d = (uint8_t*)wd_hrc.p;
  pos_d = (uint32_t*)wd_hpos.p;
  leave_d = leave ? (const uint8_t*)wd_hleave.p : nullptr;
  return DCC_OK;
}

int dcc_ctx::waitdie_epoch(const dcc_batch* b, const uint64_t* ts_in, uint8_t* rc_io, uint32_t* pos_io,
                           uint32_t* out_conflict, dcc_stats* st) {
  dcc_ctx* ctx = this;
  EpochStats es;
  dcc_stats& S = es.S;
  WdOpen O;
  CR(wd_open(this, b, ts_in, rc_io, pos_io, false, nullptr, nullptr, nullptr, O));
  if (O.A.n == 0) {
    if (st) *st = S;
    return DCC_OK;
  }
  const uint64_t n = O.A.n, m = O.A.m, tiles = O.tiles;
  const bool dev = O.dev, prof = profiling;
  const unsigned max_grid = O.max_grid;
  const KeyPack kp = O.kp;
  const WdArgs& A = O.A;
  uint32_t* conf_dev = out_conflict ? (dev ? out_conflict : (uint32_t*)wd_conf.p) : nullptr;
  SegWork& W = seg;
  uint32_t* cnt = A.cnt;

  CK(hipEventRecord(ev0, stream));
  if (prof) CK(hipEventRecord(pev[0], stream));
  uint64_t* kb[2] = {(uint64_t*)W.k[0].p, (uint64_t*)W.k[1].p};
  uint32_t* vb[2] = {(uint32_t*)W.v[0].p, (uint32_t*)W.v[1].p};
  const unsigned agrid = launch_grid(n, O.per_block, max_grid);
  k_wd_prep<<<agrid, WD_T, 0, stream>>>(A, kp, kb[0], vb[0]);
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
  CR(rounds_loop(this, cnt + WD_C_RING, n, n + m + 2, "waitdie", rounds,
                 [&](uint32_t, const uint32_t* left, uint32_t* left_out, uint64_t) {
                   if (m) {
                     SA.left = left;
                     k_wd_scan<false><<<(unsigned)tiles, WD_T, 0, stream>>>(SA);
                     k_tile_aggscan<WqOp><<<1, SEG_AGG_T, 0, stream>>>(SA.agg, SA.pre, tiles, left, left_out);
                     k_wd_scan<true><<<(unsigned)tiles, WD_T, 0, stream>>>(SA);
                   } else {
                     k_tile_aggscan<WqOp><<<1, SEG_AGG_T, 0, stream>>>(nullptr, nullptr, 0, left, left_out);
                   }
                   k_wd_advance<<<agrid, WD_T, 0, stream>>>(A, left, left_out);
                 }));

  // rc / pos of a host call stay as they were unless the decisions are sound:
  // the final pass writes the staged copies
  k_wd_final<<<launch_grid(n, WD_T, max_grid), WD_T, 0, stream>>>(n, A.stp, A.rc, A.pos, conf_dev, cnt);
  CK(hipGetLastError());
  if (prof) CK(hipEventRecord(pev[4], stream));
  CK(hipEventRecord(ev1, stream));
  CK(hipMemcpyAsync(hmisc, cnt, WD_C_RING * 4, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  const uint32_t* hc = (const uint32_t*)hmisc;
  if (hc[SEG_C_ERR] & WD_ERR_STATE) return fail(DCC_EIO, "waitdie: inconsistent decisions");
  S.rounds = rounds;
  S.n_commit = hc[WD_C_OK];
  S.n_abort = hc[WD_C_DIE];
  S.n_survivors = hc[WD_C_WAIT];
  S.nnz_w = hc[WD_C_NEX];
  S.n_readonly = hc[WD_C_RO];
  if (!dev) {
    CK(hipMemcpyAsync(rc_io, A.rc, n, hipMemcpyDeviceToHost, stream));
    CK(hipMemcpyAsync(pos_io, A.pos, n * 4, hipMemcpyDeviceToHost, stream));
    if (out_conflict) CK(hipMemcpyAsync(out_conflict, conf_dev, n * 4, hipMemcpyDeviceToHost, stream));
    CK(hipStreamSynchronize(stream));
  }
  S.alg_bytes = dcc_waitdie_alg_bytes(n, m, out_conflict != nullptr);
  CR(es.finish(this, 4));
  if (st) *st = S;
  return DCC_OK;
}

int dcc_ctx::waitdie_release(const dcc_batch* b, const uint64_t* ts_in, uint8_t* rc_io, uint32_t* pos_io,
                             const uint8_t* leave_in, uint64_t* out_left, uint64_t* out_promoted,
                             dcc_stats* st) {
  dcc_ctx* ctx = this;
  EpochStats es;
  dcc_stats& S = es.S;
  WdOpen O;
  CR(wd_open(this, b, ts_in, rc_io, pos_io, true, leave_in, out_left, out_promoted, O));
  if (O.A.n == 0) {
    if (st) *st = S;
    return DCC_OK;
  }
  const uint64_t n = O.A.n, m = O.A.m, tiles = O.tiles;
  const unsigned max_grid = O.max_grid;
  const KeyPack kp = O.kp, tp = make_keypack(O.c.tvar);
  const WdArgs& A = O.A;
  SegWork& W = seg;

  CK(hipEventRecord(ev0, stream));
  if (m) {
    uint64_t* kb[2] = {(uint64_t*)W.k[0].p, (uint64_t*)W.k[1].p};
    uint32_t* vb[2] = {(uint32_t*)W.v[0].p, (uint32_t*)W.v[1].p};
    const unsigned mgrid = launch_grid(m, WD_T, max_grid);
    // the records hold what the passes below need of rc / pos / leave: the
    // state is only written behind them (the checked offsets cover every
    // access, so k_wd_rprep writes every key and record)
    k_wd_rprep<<<launch_grid(n, O.per_block, max_grid), WD_T, 0, stream>>>(A, O.leave_dev, tp, kb[0], vb[0]);
    CK(hipGetLastError());
    const int c1 = radix_sort_u64(kb, vb, m, tp.bits, (uint32_t*)cv_scratch.p, stream);
    uint64_t* kb2[2] = {kb[c1], kb[c1 ^ 1]};
    uint32_t* vb2[2] = {vb[c1], vb[c1 ^ 1]};
    k_wd_rkey<<<mgrid, WD_T, 0, stream>>>(m, A.arec, A.keys, kp, vb2[0], kb2[0]);
    CK(hipGetLastError());
    const int c2 = radix_sort_u64(kb2, vb2, m, kp.bits + 1, (uint32_t*)cv_scratch.p, stream);
    k_wd_rseg<<<mgrid, WD_T, 0, stream>>>(m, A.arec, kb2[c2], vb2[c2], (uint32_t*)W.stxn.p,
                                          (uint32_t*)W.sinfo.p);
    CK(hipGetLastError());
    const WdRel R{m,       (const uint32_t*)W.stxn.p, (const uint32_t*)W.sinfo.p, (uint64_t*)W.agg.p,
                  (uint64_t*)W.agg.p + tiles, A.rc,   A.pos,                       A.cnt};
    k_wd_rscan<false><<<(unsigned)tiles, WD_T, 0, stream>>>(R);
    k_tile_aggscan<RqOp><<<1, SEG_AGG_T, 0, stream>>>(R.agg, R.pre, tiles, nullptr, nullptr);
    k_wd_rscan<true><<<(unsigned)tiles, WD_T, 0, stream>>>(R);
    CK(hipGetLastError());
  }
  k_wd_rgone<<<launch_grid(n, WD_T, max_grid), WD_T, 0, stream>>>(n, O.leave_dev, A.rc);
  CK(hipGetLastError());
  CK(hipEventRecord(ev1, stream));
  CK(hipMemcpyAsync(hmisc, A.cnt, WD_C_RING * 4, hipMemcpyDeviceToHost, stream));
  if (!O.dev) {
    CK(hipMemcpyAsync(rc_io, A.rc, n, hipMemcpyDeviceToHost, stream));
    CK(hipMemcpyAsync(pos_io, A.pos, n * 4, hipMemcpyDeviceToHost, stream));
  }
  CK(hipStreamSynchronize(stream));
  const uint32_t* hc = (const uint32_t*)hmisc;
  S.n_commit = O.c.count;
  S.n_survivors = hc[WD_C_PROM];
  if (out_left) *out_left = S.n_commit;
  if (out_promoted) *out_promoted = S.n_survivors;
  CR(es.finish(this, 0));
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
