// The NO_WAIT lock table that lives across epochs (dcc_locktab_*): Row_lock's
// lock_type / owner_cnt (concurrency_control/row_lock.cpp) where the batches
// live.  lock_get's grant (row_lock.cpp:183-195: owner_cnt++, lock_type = type)
// is the grant pass of an epoch, lock_release (:240-256: owner_cnt--, LOCK_NONE
// at zero) is dcc_locktab_release.
//
// The table is open addressing over 2^k 16-byte slots with the probe loop
// and the double hashing (ProbeDouble) of dcc_device.h:
//
//   struct LtSlot { u64 key; u32 word; u32 rel; }
//     word  EX:1 | owner_cnt:31     0: LOCK_NONE
//     rel   releases of the call in flight (scratch; zero between calls)
//
// Keys are inserted by CAS and never removed in place, so a probe's stop at an
// empty key stays exact; a released row keeps its slot with word 0.  The host
// knows the slots in use and the rows held from each call's read-back and
// re-inserts the held rows into the second buffer (k_lt_rebuild) before the
// slots in use plus an epoch's requests would pass cap_rows (at most half of
// the slots).
//
// A lock epoch is nowait.hip's with two passes of this file around its rounds:
//   k_lt_seed    per request: the row's word; a held row publishes the tag-0
//                word 0 at the request's per-epoch slot (`own` always, `aux`
//                iff EX-held): k_nw_held's effect without a held list
//   k_lt_grant   after k_nw_final, behind the epoch's error word: every
//                request of a committed txn inserts its key, adds 1 and sets
//                the type.  Committed txns are mutually compatible, so a row
//                takes SH increments or one EX onto a free row: no order
//                between threads is needed.
// Both use the P-lanes-per-txn layout of the k_nw_* kernels (nowait_lanes.h).
//
// Isolation levels (DCC_ISO_*).  READ_COMMITTED: a read may
// meet a row that is EX-held in this table alone.  Of the two ways to tell it
// so, the reads keep a per-epoch slot whenever a table handle is present
// (k_nw_build_rd inserts instead of looking up; they still publish nothing),
// and k_lt_seed stays as it is.  k_lt_grant<true> keeps the EX requests of the
// committed txns only.  READ_UNCOMMITTED: k_lt_seed<true> enters the held rows
// the epoch requests into the per-epoch table itself (there is no build), and
// nothing is granted.  The release kernels take the accesses of the level:
// all of them, the EX ones, or none (REL_*).
//
// A release is four launches back to back and one host synchronisation:
//   k_lt_rcheck  the offsets, before anything indexes with them
//   k_lt_radd    per selected access: find the row (not found: verdict), keep
//                its slot id, rel += 1
//   k_lt_rcmp    per selected access: rel > owner_cnt: verdict.  The sum over
//                the whole call is compared, so two txns that each release a
//                row held once fail together.
//   k_lt_rapply  clear verdict: word -= 1 per access, the decrement that takes
//                the count to 0 clears the type and counts a freed row; any
//                verdict but the offsets': nothing but rel is undone.  Both
//                ways rel is zero again.
// The grant and the release's adds and decrements go through a per-workgroup
// LDS combiner (LtComb): a hot row gets one device atomic per workgroup and
// flush instead of one per request.
// A pass leaves early only on verdict bits that an EARLIER launch set, so every
// selected access has its slot id written before a later pass reads it.  No
// workgroup waits on another and nothing spins.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "dcc.h"
#include "dcc_ctx.h"
#include "dcc_device.h"
#include "nowait_lanes.h"

using namespace dcc;

namespace {

constexpr uint32_t LT_EX = 0x80000000u, LT_CNT = 0x7FFFFFFFu;
struct __attribute__((aligned(16))) LtSlot {
  uint64_t key;
  uint32_t word;
  uint32_t rel;
};
static_assert(sizeof(LtSlot) == 16, "one slot is one 16-byte access");

// control words (u32)
constexpr uint32_t LT_C_ERR = 0, LT_C_NEW = 1, LT_C_ROWS = 2, LT_C_HOLDS = 3, LT_C_FREED = 4, LT_C_SELN = 5,
                   LT_C_SELM = 6, LT_C_OUT = 7, LT_C_WORDS = 8;
constexpr uint32_t LT_ERR_OFF = 1, LT_ERR_KEY = 2, LT_ERR_MISS = 4, LT_ERR_OVER = 8, LT_ERR_FULL = 16;

// the probes of dcc_device.h; SID_NONE from the insert: full, which the
// host's room check (at most half full) keeps from happening
__device__ inline uint32_t lt_insert(LtSlot* tab, uint32_t mask, uint64_t key, bool& claimed) {
  return probe_insert<ProbeDouble>(tab, mask, key, claimed);
}
__device__ inline uint32_t lt_find(const LtSlot* tab, uint32_t mask, uint64_t key) {
  return probe_find<ProbeDouble>(tab, mask, key);
}

// Per-workgroup combiner of the adds to table words: the adds of one slot are
// folded in LDS first and go out as one device atomic per slot and flush.  A
// hot row has as many owners as an epoch has readers of it, and a single word
// serialises device atomics (dcc_device.h, LdsMin): one atomic per request
// made the grant and the release of the 1,048,576 x 16 epoch 5.5 ms and 12.3
// ms.  A workgroup flushes every LT_FLUSH steps, so the
// window is at most half full; an add that finds no room goes out directly.
// A flush before the last one keeps the entries that gathered LT_HOT adds or
// more: a hot row goes out once per workgroup.  Taking the others out breaks
// probe chains, so a slot may come to own two entries; both are flushed, and
// the sums are the same.
constexpr uint32_t LT_NT = 4096;                  // entries per workgroup (32 KB of LDS)
constexpr uint32_t LT_FLUSH = LT_NT / 2 / NW_T;  // steps between two flushes
constexpr uint32_t LT_HOT = 4;                   // adds within one window that make a slot hot
struct LtComb {
  uint32_t sid[LT_NT];
  uint32_t val[LT_NT];
  __device__ void init() {
    for (uint32_t q = threadIdx.x; q < LT_NT; q += NW_T) {
      sid[q] = SID_NONE;
      val[q] = 0;
    }
  }
  // false: no room in the probe window (the caller applies the add itself)
  __device__ bool add(uint32_t s, uint32_t v) {
    uint32_t h = (s * 2654435761u) >> (32 - __builtin_ctz(LT_NT));
#pragma unroll 1
    for (int q = 0; q < 8; q++) {
      const uint32_t cur = sid[h];
      if (cur == s || (cur == SID_NONE && (atomicCAS(&sid[h], SID_NONE, s) == SID_NONE || sid[h] == s))) {
        atomicAdd(&val[h], v);
        return true;
      }
      h = (h + 1) & (LT_NT - 1);
    }
    return false;
  }
  // every thread of the workgroup: f(slot, sum) per entry that leaves; all:
  // the last flush, every entry leaves
  template <class F>
  __device__ void flush(F f, bool all) {
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < LT_NT; q += NW_T) {
      const uint32_t s = sid[q];
      if (s == SID_NONE || (!all && val[q] >= LT_HOT)) continue;
      f(s, val[q]);
      sid[q] = SID_NONE;
      val[q] = 0;
    }
    __syncthreads();
  }
};

__global__ __launch_bounds__(NW_T) void k_lt_clear(LtSlot* __restrict__ tab, uint64_t n_slots) {
  const uint64_t stride = (uint64_t)gridDim.x * NW_T;
  for (uint64_t h = (uint64_t)blockIdx.x * NW_T + threadIdx.x; h < n_slots; h += stride)
    tab[h] = LtSlot{KEY_EMPTY, 0u, 0u};
}

// The rows with owner_cnt > 0 into the cleared buffer `to`.
__global__ __launch_bounds__(NW_T) void k_lt_rebuild(const LtSlot* __restrict__ from, uint64_t n_slots,
                                                     LtSlot* to, uint32_t mask, uint32_t* __restrict__ ctl) {
  const uint64_t stride = (uint64_t)gridDim.x * NW_T;
  for (uint64_t h = (uint64_t)blockIdx.x * NW_T + threadIdx.x; h < n_slots; h += stride) {
    const LtSlot s = from[h];
    if (s.key == KEY_EMPTY || (s.word & LT_CNT) == 0) continue;
    bool claimed;
    const uint32_t q = lt_insert(to, mask, s.key, claimed);
    if (q == SID_NONE) atomicOr(&ctl[LT_C_ERR], LT_ERR_FULL);
    else to[q].word = s.word;  // one slot per key in `from`: one writer
  }
}

struct LtSeed {
  uint64_t n;
  const uint32_t* off;
  const uint64_t* keys;
  const uint32_t* sid;
  Slot* tab;  // the per-epoch table
  uint32_t lp;
  const LtSlot* lt;
  uint32_t mask;
  uint32_t emask;  // INS: the per-epoch table's mask
  uint32_t* err;   // INS: the epoch's error word
};

// INS (READ_UNCOMMITTED): no request has a per-epoch slot; a held row gets one here.
template <bool INS>
__global__ __launch_bounds__(NW_T) void k_lt_seed(LtSeed A) {
  const Seg g = seg_of(A.lp);
  const uint32_t gpb = NW_T >> A.lp;
  for (uint64_t g0 = (uint64_t)blockIdx.x * gpb; g0 < A.n; g0 += (uint64_t)gridDim.x * gpb) {
    const uint64_t t = g0 + g.gl;
    if (t >= A.n) continue;
    const uint32_t o0 = A.off[t], len = A.off[t + 1] - o0;
    if (g.a >= len) continue;
    const uint64_t x = (uint64_t)o0 + g.a;
    uint32_t s = SID_NONE;
    if constexpr (!INS) {
      s = A.sid[x];
      if (s == SID_NONE) continue;  // the epoch fails on its own (per-epoch table full)
    }
    const uint32_t h = lt_find(A.lt, A.mask, A.keys[x]);
    if (h == SID_NONE) continue;
    const uint32_t w = A.lt[h].word;
    if ((w & LT_CNT) == 0) continue;
    if constexpr (INS) {
      bool claimed;
      s = probe_insert<ProbeDouble>(A.tab, A.emask, A.keys[x], claimed);
      if (s == SID_NONE) {
        atomicOr(A.err, NW_ERR_FULL);
        continue;
      }
    }
    own_min(&A.tab[s].own, 0u);  // a held row: the committed word below every txn
    if (w & LT_EX) own_min(&A.tab[s].aux, 0u);
  }
}

// The requests that stay in the table: those of the txns with state ==
// ST_COMMIT, P = 2^lp lanes per txn; off == nullptr: a plain list, entry t is
// one request (lp 0), every one of them (state == nullptr).
struct LtGrant {
  uint64_t n;
  const uint32_t* off;
  const uint64_t* keys;
  const uint8_t* at;
  const uint8_t* state;
  uint32_t lp;
  const uint32_t* err;  // read first: nothing is written unless it is clear
  LtSlot* lt;
  uint32_t mask;
  uint32_t* ctl;
};

// EXONLY (READ_COMMITTED): the read locks were released right after the reads.
template <bool EXONLY>
__global__ __launch_bounds__(NW_T) void k_lt_grant(LtGrant A) {
  __shared__ LtComb C;
  __shared__ uint32_t s_new, s_rows, s_holds, s_err, s_stop;
  C.init();
  if (threadIdx.x == 0) {
    s_new = 0;
    s_rows = 0;
    s_holds = 0;
    s_err = 0;
    s_stop = *A.err;  // one read per workgroup: every thread takes the same way
  }
  __syncthreads();
  if (s_stop) return;
  const Seg g = seg_of(A.lp);
  const uint32_t gpb = NW_T >> A.lp;
  uint32_t c_new = 0, c_rows = 0, c_holds = 0, err = 0, step = 0;
  auto grant = [&](uint32_t h, uint32_t c) {  // owner_cnt += c
    const uint32_t old = atomicAdd(&A.lt[h].word, c);
    c_rows += (old & LT_CNT) == 0 ? 1u : 0u;
    c_holds += c;
  };
  for (uint64_t g0 = (uint64_t)blockIdx.x * gpb; g0 < A.n; g0 += (uint64_t)gridDim.x * gpb) {
    const uint64_t t = g0 + g.gl;
    bool v = t < A.n && (!A.state || A.state[t] == ST_COMMIT);  // an aborted txn leaves no trace
    uint64_t x = t;
    if (v && A.off) {
      const uint32_t o0 = A.off[t], len = A.off[t + 1] - o0;
      v = g.a < len;
      x = (uint64_t)o0 + g.a;
    }
    if constexpr (EXONLY) v = v && is_ex(A.at[x]);
    if (v) {
      bool claimed;
      const uint32_t h = lt_insert(A.lt, A.mask, A.keys[x], claimed);
      if (h == SID_NONE) {
        err = LT_ERR_FULL;
      } else {
        c_new += claimed ? 1u : 0u;
        // lock_type = EX; a stale read only costs an atomic that changes nothing
        if (is_ex(A.at[x]) && !(A.lt[h].word & LT_EX)) atomicOr(&A.lt[h].word, LT_EX);
        if (!C.add(h, 1u)) grant(h, 1u);
      }
    }
    if (++step % LT_FLUSH == 0) C.flush(grant, false);
  }
  C.flush(grant, true);
  if (c_new) atomicAdd(&s_new, c_new);
  if (c_rows) atomicAdd(&s_rows, c_rows);
  if (c_holds) atomicAdd(&s_holds, c_holds);
  if (err) atomicOr(&s_err, err);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_new) atomicAdd(&A.ctl[LT_C_NEW], s_new);
    if (s_rows) atomicAdd(&A.ctl[LT_C_ROWS], s_rows);
    if (s_holds) atomicAdd(&A.ctl[LT_C_HOLDS], s_holds);
    if (s_err) atomicOr(&A.ctl[LT_C_ERR], s_err);
  }
}

__global__ __launch_bounds__(NW_T) void k_lt_keys(const uint64_t* __restrict__ keys, uint64_t n,
                                                  uint32_t* __restrict__ ctl) {
  const uint64_t stride = (uint64_t)gridDim.x * NW_T;
  bool bad = false;
  for (uint64_t x = (uint64_t)blockIdx.x * NW_T + threadIdx.x; x < n; x += stride) bad |= keys[x] == KEY_EMPTY;
  if (bad) atomicOr(&ctl[LT_C_ERR], LT_ERR_KEY);
}

// ---- release
// the select's predicate (csr_select.h): rc[t] == want; no rc: every txn
struct RcSel {
  const uint8_t* rc;
  uint8_t want;
  __device__ bool take(uint64_t t) const { return !rc || rc[t] == want; }
};

// off == nullptr: a plain key list, entry t is one access
struct LtRel {
  uint64_t n, nnz;
  const uint32_t* off;
  const uint64_t* keys;
  RcSel S;
  uint32_t lp;  // log2 lanes per txn; a longer txn takes several steps of its lanes
  LtSlot* lt;
  uint32_t mask;
  uint32_t* sid;  // [nnz] the row's slot of every selected access
  uint32_t* ctl;
  const uint8_t* at;  // REL_EX: the access types
};
// the accesses of a selected txn that are released: SERIALIZABLE, READ_COMMITTED, READ_UNCOMMITTED
constexpr int REL_ALL = 0, REL_EX = 1, REL_NONE = 2;

__global__ __launch_bounds__(NW_T) void k_lt_rcheck(const uint32_t* __restrict__ off, uint64_t n, uint64_t nnz,
                                                    uint32_t* __restrict__ ctl) {
  const uint64_t stride = (uint64_t)gridDim.x * NW_T;
  bool bad = false;
  for (uint64_t t = (uint64_t)blockIdx.x * NW_T + threadIdx.x; t < n; t += stride) {
    const uint32_t a0 = off[t], b0 = off[t + 1];
    bad |= b0 < a0 || (t == 0 && a0 != 0) || (t == n - 1 && b0 != nnz);
  }
  if (bad) atomicOr(&ctl[LT_C_ERR], LT_ERR_OFF);
}

// The selected accesses of the lanes' txns, one after the other: f(x) with x
// the access' position in keys / sid; step_end() by every thread after each
// step of the workgroup.  Returns through sel_n / sel_m what the txns' first
// lanes counted (REL_EX: every lane, its own released accesses).
template <int REL, class F, class G>
__device__ inline void rel_for_each(const LtRel& A, uint32_t& sel_n, uint32_t& sel_m, F f, G step_end) {
  const uint32_t P = 1u << A.lp, a = threadIdx.x & (P - 1), gl = threadIdx.x >> A.lp;
  const uint32_t gpb = NW_T >> A.lp;
  for (uint64_t g0 = (uint64_t)blockIdx.x * gpb; g0 < A.n; g0 += (uint64_t)gridDim.x * gpb) {
    const uint64_t t = g0 + gl;
    if (t < A.n && A.S.take(t)) {
      uint64_t o0 = t;
      uint32_t len = 1;
      if (A.off) {
        o0 = A.off[t];
        len = A.off[t + 1] - (uint32_t)o0;
      }
      if (a == 0) {
        sel_n++;
        if constexpr (REL == REL_ALL) sel_m += len;
      }
      if constexpr (REL == REL_ALL) {
        for (uint32_t q = a; q < len; q += P) f(o0 + q);
      } else if constexpr (REL == REL_EX) {
        for (uint32_t q = a; q < len; q += P)
          if (is_ex(A.at[o0 + q])) {
            sel_m++;
            f(o0 + q);
          }
      }
    }
    step_end();
  }
}

template <int REL>
__global__ __launch_bounds__(NW_T) void k_lt_radd(LtRel A) {
  __shared__ LtComb C;
  __shared__ uint32_t s_n, s_m, s_err;
  if (A.ctl[LT_C_ERR] & LT_ERR_OFF) return;  // set by the launch before only
  C.init();
  if (threadIdx.x == 0) {
    s_n = 0;
    s_m = 0;
    s_err = 0;
  }
  __syncthreads();
  uint32_t sel_n = 0, sel_m = 0, err = 0, step = 0;
  auto add = [&](uint32_t h, uint32_t c) { atomicAdd(&A.lt[h].rel, c); };
  rel_for_each<REL>(
      A, sel_n, sel_m,
      [&](uint64_t x) {
        const uint32_t h = lt_find(A.lt, A.mask, A.keys[x]);
        A.sid[x] = h;
        if (h == SID_NONE) err = LT_ERR_MISS;  // a row the table does not have
        else if (!C.add(h, 1u)) add(h, 1u);
      },
      [&]() {
        if (++step % LT_FLUSH == 0) C.flush(add, false);
      });
  C.flush(add, true);
  if (sel_n) atomicAdd(&s_n, sel_n);
  if (sel_m) atomicAdd(&s_m, sel_m);
  if (err) atomicOr(&s_err, err);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_n) atomicAdd(&A.ctl[LT_C_SELN], s_n);
    if (s_m) atomicAdd(&A.ctl[LT_C_SELM], s_m);
    if (s_err) atomicOr(&A.ctl[LT_C_ERR], s_err);
  }
}

template <int REL>
__global__ __launch_bounds__(NW_T) void k_lt_rcmp(LtRel A) {
  if (A.ctl[LT_C_ERR] & (LT_ERR_OFF | LT_ERR_MISS)) return;  // set by the launches before only
  uint32_t sel_n = 0, sel_m = 0;
  bool over = false;
  rel_for_each<REL>(
      A, sel_n, sel_m,
      [&](uint64_t x) {
        const LtSlot* s = &A.lt[A.sid[x]];
        over |= s->rel > (s->word & LT_CNT);  // the call's releases of the row against its owners
      },
      []() {});
  if (over) atomicOr(&A.ctl[LT_C_ERR], LT_ERR_OVER);
}

template <int REL>
__global__ __launch_bounds__(NW_T) void k_lt_rapply(LtRel A) {
  __shared__ LtComb C;
  __shared__ uint32_t s_freed;
  const uint32_t verdict = A.ctl[LT_C_ERR];  // final: this launch sets no bit
  if (verdict & LT_ERR_OFF) return;           // nothing was touched
  C.init();
  if (threadIdx.x == 0) s_freed = 0;
  __syncthreads();
  uint32_t sel_n = 0, sel_m = 0, freed = 0, step = 0;
  auto apply = [&](uint32_t h, uint32_t c) {
    if (!verdict) {
      const uint32_t old = atomicSub(&A.lt[h].word, c);  // owner_cnt -= c
      if ((old & LT_CNT) == c) {                         // the last owners: lock_type = LOCK_NONE
        atomicAnd(&A.lt[h].word, LT_CNT);
        freed++;
      }
    }
    A.lt[h].rel = 0;  // whoever touches the row stores the same zero
  };
  rel_for_each<REL>(
      A, sel_n, sel_m,
      [&](uint64_t x) {
        const uint32_t h = A.sid[x];
        if (h != SID_NONE && !C.add(h, 1u)) apply(h, 1u);
      },
      [&]() {
        if (++step % LT_FLUSH == 0) C.flush(apply, false);
      });
  C.flush(apply, true);
  if (freed) atomicAdd(&s_freed, freed);
  __syncthreads();
  if (threadIdx.x == 0 && s_freed) atomicAdd(&A.ctl[LT_C_FREED], s_freed);
}

// (key, lock_type, owner_cnt) of the held rows, one position per row taken
// with one atomic per wave.
__global__ __launch_bounds__(NW_T) void k_lt_export(const LtSlot* __restrict__ tab, uint64_t n_slots,
                                                    uint64_t* __restrict__ keys, uint8_t* __restrict__ type,
                                                    uint32_t* __restrict__ cnt, uint64_t cap,
                                                    uint32_t* __restrict__ ctl) {
  const uint64_t stride = (uint64_t)gridDim.x * NW_T;
  const uint64_t first = (uint64_t)blockIdx.x * NW_T + threadIdx.x;
  for (uint64_t h0 = first - lane_id(); h0 < n_slots; h0 += stride) {  // whole waves: the ballot needs every lane
    const uint64_t h = h0 + lane_id();
    LtSlot s{KEY_EMPTY, 0u, 0u};
    if (h < n_slots) s = tab[h];
    const bool held = s.key != KEY_EMPTY && (s.word & LT_CNT) != 0;
    const uint64_t bm = ballot64(held);
    if (!bm) continue;
    uint32_t base = 0;
    if (lane_id() == (uint32_t)__builtin_ctzll(bm)) base = atomicAdd(&ctl[LT_C_OUT], (uint32_t)__popcll(bm));
    base = __shfl(base, __builtin_ctzll(bm));
    const uint64_t q = (uint64_t)base + (uint32_t)__popcll(bm & lanemask_lt());
    if (held && q < cap) {
      if (keys) keys[q] = s.key;
      if (type) type[q] = (s.word & LT_EX) ? DCC_LOCK_EX : DCC_LOCK_SH;
      if (cnt) cnt[q] = s.word & LT_CNT;
    }
  }
}

}  // namespace

int dcc_ctx::locktab_alloc(dcc_locktab* lt) {
  uint64_t slots = 64;
  while (slots < 2 * lt->P.cap_rows) slots <<= 1;
  lt->n_slots = slots;
  for (auto& t : lt->tab) CR(t.ensure(this, slots * sizeof(LtSlot), "lock table"));
  CR(lt->ctl.ensure(this, LT_C_WORDS * 4, "lock table control words"));
  // a host export writes at most cap_rows rows
  const uint64_t rows = std::max<uint64_t>(lt->P.cap_rows, 1);
  CR(lt->st_keys.ensure(this, rows * 8, "lock table export keys"));
  CR(lt->st_type.ensure(this, rows, "lock table export types"));
  CR(lt->st_cnt.ensure(this, rows * 4, "lock table export counts"));
  return locktab_clear(lt);
}

int dcc_ctx::locktab_clear(dcc_locktab* lt) {
  dcc_ctx* ctx = this;
  k_lt_clear<<<launch_grid(lt->n_slots, NW_T * 4, (unsigned)n_cu * 16), NW_T, 0, stream>>>(
      (LtSlot*)lt->tab[lt->cur].p, lt->n_slots);
  CK(hipGetLastError());
  CK(hipStreamSynchronize(stream));
  lt->slots_used = lt->rows_held = lt->holds = 0;
  return DCC_OK;
}

int dcc_ctx::locktab_begin(dcc_locktab* lt, uint64_t incoming, const char* what) {
  dcc_ctx* ctx = this;
  const uint64_t bound = lt->P.cap_rows;  // <= n_slots / 2
  lt->rebuilt = false;
  if (lt->holds + incoming > LT_CNT)
    return fail(DCC_ERANGE, "lock table %s: %llu requests on top of %llu held ones exceed the 31-bit owner count",
                what, (unsigned long long)incoming, (unsigned long long)lt->holds);
  uint32_t* ctl = (uint32_t*)lt->ctl.p;
  CK(hipMemsetAsync(ctl, 0, LT_C_WORDS * 4, stream));
  if (lt->slots_used + incoming > bound) {
    if (lt->rows_held + incoming > bound)
      return fail(DCC_ERANGE, "lock table %s: %llu requests beside %llu held rows, room for %llu rows", what,
                  (unsigned long long)incoming, (unsigned long long)lt->rows_held, (unsigned long long)bound);
    // the held rows alone into the other buffer; the once-held ones are dropped
    const unsigned grid = launch_grid(lt->n_slots, NW_T * 4, (unsigned)n_cu * 16);
    LtSlot* to = (LtSlot*)lt->tab[lt->cur ^ 1].p;
    k_lt_clear<<<grid, NW_T, 0, stream>>>(to, lt->n_slots);
    k_lt_rebuild<<<grid, NW_T, 0, stream>>>((const LtSlot*)lt->tab[lt->cur].p, lt->n_slots, to,
                                            (uint32_t)(lt->n_slots - 1), ctl);
    CK(hipGetLastError());
    if (profiling) CK(hipEventRecord(pev[7], stream));
    lt->cur ^= 1;
    lt->slots_used = lt->rows_held;
    lt->rebuilds++;
    lt->rebuilt = true;
  }
  return DCC_OK;
}

int dcc_ctx::locktab_seed(dcc_locktab* lt, const LtEpoch& E) {
  dcc_ctx* ctx = this;
  if (profiling) CK(hipEventRecord(pev[5], stream));
  LtSeed A{E.n,    E.off, E.keys, E.sid, E.tab, E.lp, (const LtSlot*)lt->tab[lt->cur].p, (uint32_t)(lt->n_slots - 1),
           E.mask, (uint32_t*)E.err};
  if (E.level == ISO_RU) k_lt_seed<true><<<E.grid, NW_T, 0, stream>>>(A);
  else k_lt_seed<false><<<E.grid, NW_T, 0, stream>>>(A);
  CK(hipGetLastError());
  return DCC_OK;
}

int dcc_ctx::locktab_grant(dcc_locktab* lt, const LtEpoch& E) {
  dcc_ctx* ctx = this;
  if (profiling) CK(hipEventRecord(pev[6], stream));
  uint32_t* ctl = (uint32_t*)lt->ctl.p;
  LtGrant A{E.n, E.off, E.keys, E.at, E.state, E.lp, E.err, (LtSlot*)lt->tab[lt->cur].p, (uint32_t)(lt->n_slots - 1),
            ctl};
  // fewer, longer workgroups than the epoch's passes: the combiner folds what one workgroup sees
  const unsigned grid = launch_grid(E.n, NW_T >> E.lp, (unsigned)n_cu * 4);
  if (E.level == ISO_RC) k_lt_grant<true><<<grid, NW_T, 0, stream>>>(A);
  else if (E.level == ISO_SER) k_lt_grant<false><<<grid, NW_T, 0, stream>>>(A);  // READ_UNCOMMITTED: nothing stays
  CK(hipGetLastError());
  CK(hipMemcpyAsync((uint8_t*)hmisc + LT_HMISC_OFF, ctl, LT_C_WORDS * 4, hipMemcpyDeviceToHost, stream));
  return DCC_OK;
}

// after the call's last synchronisation, its own errors checked
int dcc_ctx::locktab_end(dcc_locktab* lt, uint64_t* granted) {
  dcc_ctx* ctx = this;
  const uint32_t* hc = (const uint32_t*)((const uint8_t*)hmisc + LT_HMISC_OFF);
  if (hc[LT_C_ERR] & LT_ERR_FULL) return fail(DCC_EIO, "lock table: full below its load bound");
  lt->slots_used += hc[LT_C_NEW];
  lt->rows_held += hc[LT_C_ROWS];
  lt->holds += hc[LT_C_HOLDS];
  if (granted) *granted = hc[LT_C_HOLDS];
  lt->pass_ms[0] = lt->pass_ms[1] = lt->pass_ms[2] = 0;
  if (profiling) {
    float ms = 0;
    if (granted) {  // an epoch: the seed pass ran
      CK(hipEventElapsedTime(&ms, pev[5], pev[1]));
      lt->pass_ms[0] = ms;
    }
    CK(hipEventElapsedTime(&ms, pev[6], pev[4]));
    lt->pass_ms[1] = ms;
    if (lt->rebuilt) {
      CK(hipEventElapsedTime(&ms, pev[0], pev[7]));
      lt->pass_ms[2] = ms;
    }
  }
  return DCC_OK;
}

int dcc_ctx::locktab_acquire(dcc_locktab* lt, const dcc_calvin_held* rows, bool dev) {
  dcc_ctx* ctx = this;
  const uint64_t n = rows ? rows->n : 0;
  if (n == 0) return DCC_OK;
  if (!rows->keys || !rows->acctype) return fail(DCC_EINVAL, "lock table acquire: null keys/acctype");
  if (n > 0xFFFFFFFFull) return fail(DCC_ERANGE, "lock table acquire: more than 2^32-1 rows");
  const uint64_t* hk;
  const uint8_t* ha;
  CR(stage_held(rows, dev, hk, ha));
  const bool prof = profiling;
  if (prof) CK(hipEventRecord(pev[0], stream));
  CR(locktab_begin(lt, n, "acquire"));
  uint32_t* ctl = (uint32_t*)lt->ctl.p;
  const unsigned grid = launch_grid(n, NW_T, (unsigned)n_cu * 16);
  k_lt_keys<<<grid, NW_T, 0, stream>>>(hk, n, ctl);  // a reserved key: nothing is acquired
  LtEpoch E;
  E.n = n;
  E.keys = hk;
  E.at = ha;
  E.err = &ctl[LT_C_ERR];
  E.grid = grid;
  CR(locktab_grant(lt, E));
  if (prof) CK(hipEventRecord(pev[4], stream));
  CK(hipStreamSynchronize(stream));
  const uint32_t* hc = (const uint32_t*)((const uint8_t*)hmisc + LT_HMISC_OFF);
  if (hc[LT_C_ERR] & LT_ERR_KEY) return fail(DCC_EINVAL, "lock table acquire: key equal to DCC_KEY_RESERVED");
  return locktab_end(lt, nullptr);
}

int dcc_ctx::locktab_release(dcc_locktab* lt, const dcc_batch* b, const uint8_t* rc_in, uint8_t want,
                             const uint64_t* keys, uint64_t n_keys, bool keys_dev, uint64_t* out_n,
                             uint64_t* out_nnz, dcc_stats* st) {
  dcc_ctx* ctx = this;
  EpochStats es;
  dcc_stats& S = es.S;
  if (out_n) *out_n = 0;
  if (out_nnz) *out_nnz = 0;
  LtRel A{};
  int rel = REL_ALL;
  if (b) {
    CR(check_batch(b, false));  // txn length is free here; the offsets are checked on the device
    const uint32_t iso = b->flags & (DCC_ISO_READ_COMMITTED | DCC_ISO_READ_UNCOMMITTED);
    if (iso == (DCC_ISO_READ_COMMITTED | DCC_ISO_READ_UNCOMMITTED))
      return fail(DCC_EINVAL, "lock table release: both isolation bits set");
    rel = iso == DCC_ISO_READ_COMMITTED ? REL_EX : iso ? REL_NONE : REL_ALL;
    A.n = b->n_txn;
  } else {
    if (n_keys && !keys) return fail(DCC_EINVAL, "lock table release: null keys");
    A.n = n_keys;
  }
  if (A.n == 0) {
    S.alg_bytes = dcc_locktab_release_alg_bytes(0, 0, 0);
    es.wall();
    if (st) *st = S;
    return DCC_OK;
  }
  if (A.n > 0xFFFFFFFFull) return fail(DCC_ERANGE, "lock table release: more than 2^32-1 txns");
  if (b) {
    const bool dev = (b->flags & DCC_DEVICE_PTRS) != 0;
    DevBatch d;
    CR(stage_batch(b, d));  // compact forms are widened here
    A.nnz = d.nnz;
    A.off = d.off;
    A.keys = d.keys;
    A.at = d.acctype;
    A.S.want = want;
    if (rc_in) CR(stage(lt->st_rc, rc_in, A.n, dev, "lock table release rc", A.S.rc));
    // lanes per txn: the power of two at or above the mean length, 64 at most
    const uint64_t mean = (A.nnz + A.n - 1) / A.n;
    while (A.lp < 6 && (1ull << A.lp) < mean) A.lp++;
  } else {
    A.nnz = A.n;
    CR(stage(held_keys, keys, A.n * 8, keys_dev, "lock table release keys", A.keys));
  }
  CR(nw_sid.ensure(this, std::max<uint64_t>(A.nnz, 1) * 4, "nowait slot ids"));
  uint32_t* ctl = (uint32_t*)lt->ctl.p;
  A.lt = (LtSlot*)lt->tab[lt->cur].p;
  A.mask = (uint32_t)(lt->n_slots - 1);
  A.sid = (uint32_t*)nw_sid.p;
  A.ctl = ctl;
  const unsigned max_grid = (unsigned)n_cu * 16;
  const unsigned grid = launch_grid(A.n, NW_T >> A.lp, max_grid);
  const unsigned grid_c = launch_grid(A.n, NW_T >> A.lp, (unsigned)n_cu * 4);  // the passes with a combiner
  const bool prof = profiling;
  CK(hipMemsetAsync(ctl, 0, LT_C_WORDS * 4, stream));
  CK(hipEventRecord(ev0, stream));
  if (prof) CK(hipEventRecord(pev[0], stream));
  if (A.off) k_lt_rcheck<<<launch_grid(A.n, NW_T * 4, max_grid), NW_T, 0, stream>>>(A.off, A.n, A.nnz, ctl);
  if (prof) CK(hipEventRecord(pev[1], stream));
  if (rel == REL_EX) k_lt_radd<REL_EX><<<grid_c, NW_T, 0, stream>>>(A);
  else if (rel == REL_NONE) k_lt_radd<REL_NONE><<<grid_c, NW_T, 0, stream>>>(A);  // counts the selected txns
  else k_lt_radd<REL_ALL><<<grid_c, NW_T, 0, stream>>>(A);
  if (prof) CK(hipEventRecord(pev[2], stream));
  if (rel == REL_EX) k_lt_rcmp<REL_EX><<<grid, NW_T, 0, stream>>>(A);
  else if (rel == REL_ALL) k_lt_rcmp<REL_ALL><<<grid, NW_T, 0, stream>>>(A);
  if (prof) CK(hipEventRecord(pev[3], stream));
  if (rel == REL_EX) k_lt_rapply<REL_EX><<<grid_c, NW_T, 0, stream>>>(A);
  else if (rel == REL_ALL) k_lt_rapply<REL_ALL><<<grid_c, NW_T, 0, stream>>>(A);
  CK(hipGetLastError());
  if (prof) CK(hipEventRecord(pev[4], stream));
  CK(hipEventRecord(ev1, stream));
  CK(hipMemcpyAsync(hmisc, ctl, LT_C_WORDS * 4, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  const uint32_t* hc = (const uint32_t*)hmisc;
  const uint32_t verdict = hc[LT_C_ERR];
  if (verdict & LT_ERR_OFF) return fail(DCC_EINVAL, "batch: malformed offsets");
  const uint64_t ns = hc[LT_C_SELN], ms = hc[LT_C_SELM];
  if (out_n) *out_n = ns;
  if (out_nnz) *out_nnz = ms;
  S.n_commit = ns;
  S.n_abort = A.n - ns;
  if (verdict & LT_ERR_MISS) return fail(DCC_EINVAL, "lock table release: a row the table does not have");
  if (verdict & LT_ERR_OVER)
    return fail(DCC_EINVAL, "lock table release: a row released more often than it is held");
  if (ms > lt->holds || hc[LT_C_FREED] > lt->rows_held)
    return fail(DCC_EIO, "lock table release: the counts disagree with the host's");
  lt->holds -= ms;
  lt->rows_held -= hc[LT_C_FREED];
  S.alg_bytes = dcc_locktab_release_alg_bytes(b ? A.n : 0, ns, ms);
  CR(es.finish(this, 4));
  if (st) *st = S;
  return DCC_OK;
}

int dcc_ctx::locktab_export(dcc_locktab* lt, uint64_t* keys, uint8_t* lock_type, uint32_t* owner_cnt,
                            uint64_t cap, bool dev, uint64_t* out_n) {
  dcc_ctx* ctx = this;
  const uint64_t rows = lt->rows_held;
  if (out_n) *out_n = rows;
  if (cap < rows)
    return fail(DCC_ERANGE, "lock table export: %llu rows held, room for %llu", (unsigned long long)rows,
                (unsigned long long)cap);
  if (rows == 0) return DCC_OK;
  uint64_t* dk = keys ? (dev ? keys : (uint64_t*)lt->st_keys.p) : nullptr;
  uint8_t* dt = lock_type ? (dev ? lock_type : (uint8_t*)lt->st_type.p) : nullptr;
  uint32_t* dc = owner_cnt ? (dev ? owner_cnt : (uint32_t*)lt->st_cnt.p) : nullptr;
  uint32_t* ctl = (uint32_t*)lt->ctl.p;
  CK(hipMemsetAsync(ctl, 0, LT_C_WORDS * 4, stream));
  // rows <= cap_rows, the size of the staging arrays
  k_lt_export<<<launch_grid(lt->n_slots, NW_T * 4, (unsigned)n_cu * 16), NW_T, 0, stream>>>(
      (const LtSlot*)lt->tab[lt->cur].p, lt->n_slots, dk, dt, dc, rows, ctl);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(hmisc, ctl, LT_C_WORDS * 4, hipMemcpyDeviceToHost, stream));
  if (!dev) {
    if (keys) CK(hipMemcpyAsync(keys, dk, rows * 8, hipMemcpyDeviceToHost, stream));
    if (lock_type) CK(hipMemcpyAsync(lock_type, dt, rows, hipMemcpyDeviceToHost, stream));
    if (owner_cnt) CK(hipMemcpyAsync(owner_cnt, dc, rows * 4, hipMemcpyDeviceToHost, stream));
  }
  CK(hipStreamSynchronize(stream));
  if (((const uint32_t*)hmisc)[LT_C_OUT] != rows)
    return fail(DCC_EIO, "lock table export: %u rows found, the host counts %llu", ((const uint32_t*)hmisc)[LT_C_OUT],
                (unsigned long long)rows);
  return DCC_OK;
}

extern "C" uint64_t dcc_locktab_epoch_alg_bytes(uint64_t n_txn, uint64_t nnz, uint64_t nnz_granted,
                                                int with_conflict) {
  return dcc_nowait_alg_bytes(n_txn, nnz, with_conflict) + 16 * nnz + n_txn + 25 * nnz_granted;
}

extern "C" uint64_t dcc_locktab_release_alg_bytes(uint64_t n_txn, uint64_t n_sel, uint64_t nnz_sel) {
  (void)n_sel;
  return (n_txn ? 4 * (n_txn + 1) + n_txn : 0) + (8 + 12 + 48) * nnz_sel;
}

// the table's call on the context that runs it: rank 0's of a multi-GPU one
template <typename F>
static int lt_run(dcc_locktab* lt, bool detach, F call) {
  dcc_ctx* ctx = lt->owner;
  dcc_pipe_drain(ctx);  // pipelined OCC epochs in flight complete first
  return dcc_on_device(ctx, detach, call);
}

extern "C" int dcc_locktab_create(dcc_ctx* ctx, const dcc_locktab_params* params, dcc_locktab** out) {
  if (!ctx || !out) return DCC_EINVAL;
  *out = nullptr;
  if (!params) return ctx->fail(DCC_EINVAL, "lock table: null params");
  if (params->flags) return ctx->fail(DCC_EINVAL, "lock table: unknown flags");
  if (params->cap_rows > (1ull << 29)) return ctx->fail(DCC_ERANGE, "lock table: cap_rows exceeds 2^29 (2^30 slots)");
  std::unique_ptr<dcc_locktab> lt(new dcc_locktab());
  lt->owner = ctx;
  lt->P = *params;
  const int e = lt_run(lt.get(), false, [&](dcc_ctx* s) { return s->locktab_alloc(lt.get()); });
  if (e != DCC_OK) return e;  // what was allocated goes with lt
  *out = lt.get();
  ctx->locktabs.push_back(std::move(lt));
  return DCC_OK;
}

extern "C" void dcc_locktab_destroy(dcc_locktab* lt) {
  if (!lt) return;
  dcc_ctx* ctx = lt->owner;
  (void)lt_run(lt, false, [&](dcc_ctx* s) {  // its last call's work is done before the memory goes
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    return DCC_OK;
  });
  auto& v = ctx->locktabs;
  for (size_t i = 0; i < v.size(); i++)
    if (v[i].get() == lt) {
      v.erase(v.begin() + i);  // the DevBuf members free the device memory
      return;
    }
}

extern "C" int dcc_locktab_lock_epoch(dcc_locktab* lt, const dcc_batch* batch, uint8_t* out_rc,
                                      uint32_t* out_conflict, dcc_stats* out_stats) {
  if (!lt || !batch || !out_rc) return DCC_EINVAL;
  // the whole epoch on one GPU, as dcc_nowait_lock_epoch: no collective
  return lt_run(lt, true, [&](dcc_ctx* s) {
    return s->nowait_epoch(batch, nullptr, out_rc, out_conflict, out_stats, lt);
  });
}

extern "C" int dcc_locktab_release(dcc_locktab* lt, const dcc_batch* batch, const uint8_t* rc, uint8_t want,
                                   uint64_t* out_n, uint64_t* out_nnz, dcc_stats* out_stats) {
  if (!lt || !batch) return DCC_EINVAL;
  return lt_run(lt, false, [&](dcc_ctx* s) {
    return s->locktab_release(lt, batch, rc, want, nullptr, 0, false, out_n, out_nnz, out_stats);
  });
}

extern "C" int dcc_locktab_acquire_rows(dcc_locktab* lt, const dcc_calvin_held* rows, uint32_t flags) {
  if (!lt) return DCC_EINVAL;
  return lt_run(lt, false,
                [&](dcc_ctx* s) { return s->locktab_acquire(lt, rows, (flags & DCC_DEVICE_PTRS) != 0); });
}

extern "C" int dcc_locktab_release_rows(dcc_locktab* lt, const uint64_t* keys, uint64_t n, uint32_t flags) {
  if (!lt) return DCC_EINVAL;
  return lt_run(lt, false, [&](dcc_ctx* s) {
    return s->locktab_release(lt, nullptr, nullptr, 0, keys, n, (flags & DCC_DEVICE_PTRS) != 0, nullptr, nullptr,
                              nullptr);
  });
}

extern "C" int dcc_locktab_export(dcc_locktab* lt, uint64_t* keys, uint8_t* lock_type, uint32_t* owner_cnt,
                                  uint64_t cap, uint32_t flags, uint64_t* out_n) {
  if (!lt) return DCC_EINVAL;
  return lt_run(lt, false, [&](dcc_ctx* s) {
    return s->locktab_export(lt, keys, lock_type, owner_cnt, cap, (flags & DCC_DEVICE_PTRS) != 0, out_n);
  });
}

extern "C" int dcc_locktab_size(const dcc_locktab* lt, uint64_t* rows_held, uint64_t* slots_used,
                                uint64_t* rebuilds) {
  if (!lt) return DCC_EINVAL;
  if (rows_held) *rows_held = lt->rows_held;
  if (slots_used) *slots_used = lt->slots_used;
  if (rebuilds) *rebuilds = lt->rebuilds;
  return DCC_OK;
}

extern "C" int dcc_locktab_clear(dcc_locktab* lt) {
  if (!lt) return DCC_EINVAL;
  return lt_run(lt, false, [&](dcc_ctx* s) { return s->locktab_clear(lt); });
}

extern "C" int dcc_locktab_pass_ms(const dcc_locktab* lt, double out_ms[3]) {
  if (!lt || !out_ms) return DCC_EINVAL;
  for (int q = 0; q < 3; q++) out_ms[q] = lt->pass_ms[q];
  return DCC_OK;
}
