// NO_WAIT two-phase locking for a whole epoch (dcc_nowait_lock_epoch).
//
// Reference: the txns of the batch call get_row for their accesses, txn by
// txn in index order, against Row_lock in NO_WAIT mode (storage/row.cpp:
// 226-238, concurrency_control/row_lock.cpp:52-216).  An aborted txn releases
// what it took (system/txn.cpp:747-761, row_lock.cpp:240-256) and leaves no
// trace, a txn that gets every lock holds them to the end of the epoch, so
//
//   abort(i) <=> self_conflict(i)
//             OR some access (k, t) of i conflicts with the held prefix
//             OR exists j < i, commit(j), j holds k in mode t', t == EX or t' == EX
//
// Per key this needs two minima over the non-aborted requesters: of any mode
// (Slot::own) and of EX mode (Slot::aux).  An EX access of txn i is KILLED if
// the `own` minimum is a committed txn below i and BLOCKED if it is an
// undecided one; an SH access reads `aux` the same way.  The lowest undecided
// txn is decided in every round, so the rounds reach the unique fixed point.
//
// Words are the tagged owner words of dcc_device.h with the txn index shifted
// by one: tag 0 | 0 is a held row (below every txn), tag 0 | i + 1 a committed
// requester, round tag | i + 1 an undecided requester of that round.  Newer
// rounds carry smaller tags, so one atomicMin replaces the stale words of
// older rounds, and a committed word is never displaced.
//
// A txn takes P consecutive lanes (P = the power of two >= the epoch's
// longest txn), one access per lane, so adjacent lanes load adjacent
// accesses; per-txn reductions are ballots masked to the txn's lanes.
//
// Kernels (the batch check and the rounds loop are seg_rounds.h's, DESIGN.md
// §8n):
//           k_nw_held    held rows into the table (tag-0 words)
//           k_nw_build   every requested key into the table, the slot id of
//                        every request, self-conflicts decided, round-1 words
//           k_nw_decide  one round over the undecided list: KILLED -> abort,
//                        clear -> commit + tag-0 words, BLOCKED -> next list
//           k_nw_publish the next round's words of the txns still undecided
//           k_nw_retag   round tags exhausted: drop every tagged word
//           k_nw_final   RC bytes, counts, first conflicting request
//
// Key-sharded (DCC_SHARD_SELF on a context with a communicator; DESIGN.md
// §8p): every rank holds the whole batch and the whole held list, and rank r
// enters only the rows with dcc_key_shard(key, R) == r into its table, which
// is sized from its own requests and held rows (k_nw_count).  A request of
// another rank's row carries SID_REMOTE in sid[] and takes no part in any
// pass of this rank.  The kernels are the SH instantiations of the ones
// above; a round splits k_nw_decide in two around the exchange:
//           NW_EVAL      the rank's accesses of every undecided txn into one
//                        status byte per txn (0 none, 1 blocked, 2 killed)
//           byte-MAX all-reduce of the n status bytes
//           NW_APPLY     state from the reduced byte (the same on every rank),
//                        tag-0 words of the commits on this rank's rows,
//                        the blocked txns to the next list
// A txn that names a row twice with EX on either side is found by the row's
// rank, which marks its status byte killed in the build; the other ranks
// learn of it in round 1's exchange.  Their round-1 words of that txn block
// its readers for that one round and carry a stale tag from round 2 on.
// After the fixed point each rank's first conflicting request goes through
// one more byte-MAX exchange as 64 - ordinal (k_nw_final, k_nw_conf).
//
// Isolation levels (DCC_ISO_*): the same replay with the
// reference's early releases.  READ_COMMITTED releases a read lock right after
// the read, so a read leaves nothing: only EX requests get a slot and a word.
// `aux` is the minimum EX requester, `own` only says "held in any mode" (the
// tag-0 word 0); an EX access reads both, an SH access `aux`.  The build is
// two launches, for the grid-wide order between them:
//           k_nw_build_ex  EX requests: table_insert, sid[], round-1 `aux` word
//           k_nw_build_rd  RD/SCAN requests: table_find (SID_ABSENT: the row is
//                          not in the table, the request can never conflict);
//                          self-conflicts (an earlier access of the slot is EX)
// The round-1 words are out before k_nw_build_rd knows the self-conflicts: the
// words of a self-aborted txn cost its readers one blocked round, exactly as
// the key-sharded path's above, and carry a stale tag from round 2 on.
// The rounds are the ISO instantiations of k_nw_decide / k_nw_publish /
// k_nw_final.  READ_UNCOMMITTED releases every lock after its access: no
// access leaves a trace, k_nw_ru decides every txn against the held rows in
// one pass, and without held rows no table is built.
//
// Host (the phase shape of DESIGN.md §8n): nw_plan resolves the call once into
// an NwPlan -- key-sharded or not, the level, lock table or held list, when the
// table is sized -- and makes every host-side rejection.  nowait_epoch is then
// a sequence of phases over one NwRun:
//           nw_table     the table for nw_rows(m, hn) rows, where they suffice
//           nw_check     workspaces, the held list staged, k_batch_check next
//                        to k_nw_count / k_nw_count_ex, the read-back
//           nw_table     ... or for the rows the check counted (key-sharded;
//                        READ_COMMITTED without a lock table)
//           nw_build     ev0, locktab_begin, the table cleared, k_nw_held, the
//                        build kernels, locktab_seed
//           nw_decide    nw_rounds<SH, ISO>, the one round body of the three
//                        modes with rounds, or k_nw_ru
//           nw_readout   locktab_grant, ev1, the outputs, counts and stats
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <type_traits>

#include "dcc.h"
#include "dcc_ctx.h"
#include "dcc_device.h"
#include "dcc_scan.h"
#include "nowait_lanes.h"
#include "occ_kernels.h"
#include "seg_rounds.h"

using namespace dcc;

namespace {

constexpr uint32_t NW_STAGE = 1024;   // blocked txns a workgroup stages before one list append
// error bits next to CHK_ERR_* (a held key sets CHK_ERR_KEY too)
constexpr uint32_t NW_ERR_STATE = 8;  // NW_ERR_FULL = 4: nowait_lanes.h
// counter words (nw_misc) next to SEG_C_ERR / SEG_C_MAXLEN; the ring holds the list lengths
constexpr uint32_t NW_C_NEX = 2, NW_C_RO = 3, NW_C_COMMIT = 4, NW_C_RING = 8, NW_C_WORDS = NW_C_RING + SEG_RING;
// key-sharded: the rank's own requests / held rows, the reserved key in the held list
constexpr uint32_t NW_C_OWN = 5, NW_C_OWNHELD = 6, NW_ERR_HKEY = 16;
// sid[] of a request whose row another rank owns (SID_NONE: table full)
constexpr uint32_t SID_REMOTE = SID_NONE - 1;
// sid[] of a READ_COMMITTED read whose row is not in the table: nobody holds or
// writes it.  The levels never run key-sharded, so no kernel sees both.
constexpr uint32_t SID_ABSENT = SID_NONE - 2;
// the EX requests of the batch, counted next to the batch check
constexpr uint32_t NW_C_EXREQ = 7;
// status bytes of a sharded round
constexpr uint8_t NW_S_BLOCKED = 1, NW_S_KILLED = 2;

// the request has a slot in this rank's table; READ_COMMITTED (never key-sharded):
// its row is held or has an EX request
template <bool SH, int ISO = ISO_SER>
__device__ inline bool has_slot(uint32_t s) {
  if constexpr (ISO == ISO_RC) return s < SID_ABSENT;
  return SH ? s < SID_REMOTE : s != SID_NONE;
}
__device__ inline bool rc_slot(uint32_t s) { return has_slot<false, ISO_RC>(s); }

// A txn names a row twice with EX on either side (NO_WAIT keeps no owner
// list, row_lock.cpp:176-182): the lanes of the later requests.  Rows compare
// by slot id (one slot per key).  Every lane of the wave calls it.
template <bool SH>
__device__ inline bool self_conflict(const Seg& g, uint32_t lp, bool v, uint32_t s, uint32_t ex) {
  bool sc = false;
  const uint32_t P = 1u << lp;
  for (uint32_t q = 0; q + 1 < P; q++) {
    if (!ballot64(v && g.a > q)) break;  // no lane of the wave has an earlier access q
    const uint32_t so = __shfl(s, (int)(g.seg0 + q));
    const uint32_t eo = __shfl(ex, (int)(g.seg0 + q));
    if (v && q < g.a && so == s && has_slot<SH>(s) && (ex | eo)) sc = true;
  }
  return sc;
}

// READ_COMMITTED: only an earlier EX of the txn is still there (its reads are
// released at once): RD then WR of a row is fine, WR then RD and WR then WR
// abort at the second.  Every lane of the wave calls it.
__device__ inline bool self_conflict_rc(const Seg& g, uint32_t lp, bool v, uint32_t s, uint32_t ex) {
  bool sc = false;
  const uint32_t P = 1u << lp;
  for (uint32_t q = 0; q + 1 < P; q++) {
    if (!ballot64(v && g.a > q)) break;  // no lane of the wave has an earlier access q
    const uint32_t so = __shfl(s, (int)(g.seg0 + q));
    const uint32_t eo = __shfl(ex, (int)(g.seg0 + q));
    if (v && q < g.a && so == s && rc_slot(s) && eo) sc = true;
  }
  return sc;
}

// The rows a rank keeps: all of them, or its key shard.
struct NwAll {};
struct NwOwn {
  uint32_t rank, R;
};
template <bool SH>
using NwWho = std::conditional_t<SH, NwOwn, NwAll>;
template <bool SH>
__device__ inline bool owns(const NwWho<SH>& w, uint64_t key) {
  if constexpr (SH) return key_shard(key, w.R) == w.rank;
  else return true;
}

// Key-sharded: the rank's own requests and held rows (its table's size), and
// the reserved key anywhere in the held list.  Every index is below nnz / hn:
// it runs next to the batch check, before the offsets are known to be sound.
__global__ __launch_bounds__(CHK_T) void k_nw_count(const uint64_t* __restrict__ keys, uint64_t nnz,
                                                    const uint64_t* __restrict__ hkeys, uint64_t hn, NwOwn w,
                                                    uint32_t* __restrict__ cnt) {
  __shared__ uint32_t s_a[CHK_T / 64], s_b[CHK_T / 64];
  const uint64_t tid = (uint64_t)blockIdx.x * CHK_T + threadIdx.x, stride = (uint64_t)gridDim.x * CHK_T;
  uint32_t own = 0, ownh = 0;
  bool bad = false;
  for (uint64_t x = tid; x < nnz; x += stride) own += owns<true>(w, keys[x]) ? 1u : 0u;
  for (uint64_t x = tid; x < hn; x += stride) {
    const uint64_t key = hkeys[x];
    bad |= key == KEY_EMPTY;
    ownh += owns<true>(w, key) ? 1u : 0u;
  }
  if (bad) atomicOr(&cnt[SEG_C_ERR], NW_ERR_HKEY);
  own = block_reduce<CHK_T / 64, AddOp<uint32_t>>(own, s_a);
  ownh = block_reduce<CHK_T / 64, AddOp<uint32_t>>(ownh, s_b);
  if (threadIdx.x == 0) {
    if (own) atomicAdd(&cnt[NW_C_OWN], own);
    if (ownh) atomicAdd(&cnt[NW_C_OWNHELD], ownh);
  }
}

// READ_COMMITTED: the EX requests of the batch, the table's size next to the
// held rows.  Every index is below nnz: it runs next to the batch check.
__global__ __launch_bounds__(CHK_T) void k_nw_count_ex(const uint8_t* __restrict__ at, uint64_t nnz,
                                                       uint32_t* __restrict__ cnt) {
  __shared__ uint32_t s_a[CHK_T / 64];
  const uint64_t tid = (uint64_t)blockIdx.x * CHK_T + threadIdx.x, stride = (uint64_t)gridDim.x * CHK_T;
  uint32_t nex = 0;
  for (uint64_t x = tid; x < nnz; x += stride) nex += is_ex(at[x]);
  nex = block_reduce<CHK_T / 64, AddOp<uint32_t>>(nex, s_a);
  if (threadIdx.x == 0 && nex) atomicAdd(&cnt[NW_C_EXREQ], nex);
}

template <bool SH>
__global__ __launch_bounds__(NW_T) void k_nw_held(const uint64_t* __restrict__ keys,
                                                  const uint8_t* __restrict__ at, uint64_t n, Slot* tab,
                                                  uint32_t mask, uint32_t* __restrict__ cnt, NwWho<SH> who) {
  const uint64_t stride = (uint64_t)gridDim.x * NW_T;
  for (uint64_t x = (uint64_t)blockIdx.x * NW_T + threadIdx.x; x < n; x += stride) {
    const uint64_t key = keys[x];
    if (key == KEY_EMPTY) {
      atomicOr(&cnt[SEG_C_ERR], CHK_ERR_KEY);
      continue;
    }
    if (!owns<SH>(who, key)) continue;
    const uint32_t s = table_insert(tab, mask, key);
    if (s == SID_NONE) {
      atomicOr(&cnt[SEG_C_ERR], NW_ERR_FULL);
      continue;
    }
    own_min(&tab[s].own, 0u);  // committed word below every txn
    if (is_ex(at[x])) own_min(&tab[s].aux, 0u);
  }
}

struct NwArgs {
  uint64_t n;
  const uint32_t* off;
  const uint64_t* keys;
  const uint8_t* at;
  Slot* tab;
  uint32_t mask;
  uint32_t lp;  // log2 lanes per txn
  uint32_t* sid;
  uint8_t* state;
  uint32_t* cnt;
};
struct NwShArgs : NwArgs {
  NwOwn who;
  uint8_t* stat;  // [n] the round's status bytes, then 64 - the conflict ordinal
};
template <bool SH>
using NwA = std::conditional_t<SH, NwShArgs, NwArgs>;

template <bool SH>
__global__ __launch_bounds__(NW_T) void k_nw_build(NwA<SH> A) {
  __shared__ uint32_t s_ro, s_nex;
  if (threadIdx.x == 0) {
    s_ro = 0;
    s_nex = 0;
  }
  __syncthreads();
  const Seg g = seg_of(A.lp);
  const uint32_t gpb = NW_T >> A.lp;
  uint32_t ro = 0, nex = 0;
  for (uint64_t g0 = (uint64_t)blockIdx.x * gpb; g0 < A.n; g0 += (uint64_t)gridDim.x * gpb) {
    const uint64_t t = g0 + g.gl;
    const bool tv = t < A.n;
    uint32_t o0 = 0, len = 0;
    if (tv) {
      o0 = A.off[t];
      len = A.off[t + 1] - o0;
    }
    const bool v = tv && g.a < len;
    const uint64_t x = (uint64_t)o0 + g.a;
    uint32_t ex = 0, s = SID_NONE;
    if (v) {
      ex = is_ex(A.at[x]);
      const uint64_t key = A.keys[x];
      bool mine = true;
      if constexpr (SH) mine = owns<true>(A.who, key);
      s = mine ? table_insert(A.tab, A.mask, key) : SID_REMOTE;
      A.sid[x] = s;
      if (s == SID_NONE) atomicOr(&A.cnt[SEG_C_ERR], NW_ERR_FULL);
    }
    const bool sc = self_conflict<SH>(g, A.lp, v, s, ex);
    const bool selfc = (ballot64(sc) & g.mask) != 0;
    const uint64_t exb = ballot64(v && ex) & g.mask;
    if (v && !selfc && has_slot<SH>(s)) {
      const uint32_t w = own_word(round_tag(1), (uint32_t)t + 1u);
      own_min(&A.tab[s].own, w);
      if (ex) own_min(&A.tab[s].aux, w);
    }
    if (tv && g.a == 0) {
      if constexpr (SH) {  // the state bytes stay equal on every rank: round 1's exchange carries the abort
        A.state[t] = ST_UNDECIDED;
        if (selfc) A.stat[t] = NW_S_KILLED;
      } else {
        A.state[t] = selfc ? ST_ABORT : ST_UNDECIDED;  // an aborted txn publishes nothing
      }
      ro += exb ? 0u : 1u;
      nex += (uint32_t)__popcll(exb);
    }
  }
  if (ro) atomicAdd(&s_ro, ro);
  if (nex) atomicAdd(&s_nex, nex);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_ro) atomicAdd(&A.cnt[NW_C_RO], s_ro);
    if (s_nex) atomicAdd(&A.cnt[NW_C_NEX], s_nex);
  }
}

// READ_COMMITTED build, first launch: the EX requests enter the table and
// publish their round-1 word; a read takes nothing that outlives it.
__global__ __launch_bounds__(NW_T) void k_nw_build_ex(NwArgs A) {
  __shared__ uint32_t s_ro, s_nex;
  if (threadIdx.x == 0) {
    s_ro = 0;
    s_nex = 0;
  }
  __syncthreads();
  const Seg g = seg_of(A.lp);
  const uint32_t gpb = NW_T >> A.lp;
  uint32_t ro = 0, nex = 0;
  for (uint64_t g0 = (uint64_t)blockIdx.x * gpb; g0 < A.n; g0 += (uint64_t)gridDim.x * gpb) {
    const uint64_t t = g0 + g.gl;
    const bool tv = t < A.n;
    uint32_t o0 = 0, len = 0;
    if (tv) {
      o0 = A.off[t];
      len = A.off[t + 1] - o0;
    }
    const bool v = tv && g.a < len;
    const uint64_t x = (uint64_t)o0 + g.a;
    const bool ex = v && is_ex(A.at[x]);
    if (ex) {
      const uint32_t s = table_insert(A.tab, A.mask, A.keys[x]);
      A.sid[x] = s;
      if (s == SID_NONE) atomicOr(&A.cnt[SEG_C_ERR], NW_ERR_FULL);
      else own_min(&A.tab[s].aux, own_word(round_tag(1), (uint32_t)t + 1u));
    }
    const uint64_t exb = ballot64(ex) & g.mask;
    if (tv && g.a == 0) {
      A.state[t] = ST_UNDECIDED;
      ro += exb ? 0u : 1u;
      nex += (uint32_t)__popcll(exb);
    }
  }
  if (ro) atomicAdd(&s_ro, ro);
  if (nex) atomicAdd(&s_nex, nex);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_ro) atomicAdd(&A.cnt[NW_C_RO], s_ro);
    if (s_nex) atomicAdd(&A.cnt[NW_C_NEX], s_nex);
  }
}

// READ_COMMITTED build, second launch (every EX row is in the table): the
// reads look their row up, SID_ABSENT for a row nobody holds or writes; with
// `insert` (a lock table seeds the held rows through the requests' slots,
// k_lt_seed) a read takes a slot too, and still publishes nothing.  Both slot
// ids of a pair are known here, so this pass decides the self-conflicts; the
// round-1 words of such a txn are out already and block its readers for that
// one round (the header comment).
__global__ __launch_bounds__(NW_T) void k_nw_build_rd(NwArgs A, bool insert) {
  const Seg g = seg_of(A.lp);
  const uint32_t gpb = NW_T >> A.lp;
  for (uint64_t g0 = (uint64_t)blockIdx.x * gpb; g0 < A.n; g0 += (uint64_t)gridDim.x * gpb) {
    const uint64_t t = g0 + g.gl;
    const bool tv = t < A.n;
    uint32_t o0 = 0, len = 0;
    if (tv) {
      o0 = A.off[t];
      len = A.off[t + 1] - o0;
    }
    const bool v = tv && g.a < len;
    const uint64_t x = (uint64_t)o0 + g.a;
    uint32_t ex = 0, s = SID_NONE;
    if (v) {
      ex = is_ex(A.at[x]);
      if (ex) {
        s = A.sid[x];
      } else {
        const uint64_t key = A.keys[x];
        if (insert) {
          s = table_insert(A.tab, A.mask, key);
          if (s == SID_NONE) atomicOr(&A.cnt[SEG_C_ERR], NW_ERR_FULL);
        } else {
          s = table_find(A.tab, A.mask, key);
          if (s == SID_NONE) s = SID_ABSENT;
        }
        A.sid[x] = s;
      }
    }
    const bool sc = self_conflict_rc(g, A.lp, v, s, ex);
    const bool selfc = (ballot64(sc) & g.mask) != 0;
    if (tv && g.a == 0 && selfc) A.state[t] = ST_ABORT;
  }
}

// READ_UNCOMMITTED: every lock is released right after its access, so no
// access of the epoch leaves a trace and a txn meets the held rows alone:
// killed iff a row of its is EX-held (`aux` == 0), or held in any mode (`own`
// == 0) and the access EX.  One pass: state, RC, the first such ordinal, the
// counts.  tab == nullptr: no held rows, everything commits.
__global__ __launch_bounds__(NW_T) void k_nw_ru(NwArgs A, uint8_t* __restrict__ rc, uint32_t* __restrict__ conflict) {
  __shared__ uint32_t s_ro, s_nex, s_commit;
  if (threadIdx.x == 0) {
    s_ro = 0;
    s_nex = 0;
    s_commit = 0;
  }
  __syncthreads();
  const Seg g = seg_of(A.lp);
  const uint32_t gpb = NW_T >> A.lp;
  uint32_t ro = 0, nex = 0, commits = 0;
  for (uint64_t g0 = (uint64_t)blockIdx.x * gpb; g0 < A.n; g0 += (uint64_t)gridDim.x * gpb) {
    const uint64_t t = g0 + g.gl;
    const bool tv = t < A.n;
    uint32_t o0 = 0, len = 0;
    if (tv) {
      o0 = A.off[t];
      len = A.off[t + 1] - o0;
    }
    const bool v = tv && g.a < len;
    const uint64_t x = (uint64_t)o0 + g.a;
    uint32_t ex = 0;
    bool c = false;
    if (v) {
      ex = is_ex(A.at[x]);
      if (A.tab) {
        const uint32_t s = table_find(A.tab, A.mask, A.keys[x]);
        if (s != SID_NONE) c = A.tab[s].aux == 0u || (ex && A.tab[s].own == 0u);
      }
    }
    const uint64_t cb = ballot64(c) & g.mask;
    const uint64_t exb = ballot64(v && ex) & g.mask;
    if (tv && g.a == 0) {
      A.state[t] = cb ? ST_ABORT : ST_COMMIT;
      rc[t] = cb ? DCC_RC_ABORT : DCC_RC_RCOK;
      if (conflict) conflict[t] = cb ? (uint32_t)__builtin_ctzll(cb) - g.seg0 : DCC_ACCESS_NONE;
      commits += cb ? 0u : 1u;
      ro += exb ? 0u : 1u;
      nex += (uint32_t)__popcll(exb);
    }
  }
  if (ro) atomicAdd(&s_ro, ro);
  if (nex) atomicAdd(&s_nex, nex);
  if (commits) atomicAdd(&s_commit, commits);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_ro) atomicAdd(&A.cnt[NW_C_RO], s_ro);
    if (s_nex) atomicAdd(&A.cnt[NW_C_NEX], s_nex);
    if (s_commit) atomicAdd(&A.cnt[NW_C_COMMIT], s_commit);
  }
}

// One round.  list == nullptr: every txn (round 1), else the *m_in txns of
// the list.  Blocked txns are staged in LDS and appended to list_out with one
// atomic per NW_STAGE of them (the list order is free: decisions do not
// depend on it).  A commit publishes its tag-0 words right away: a reader
// that sees one early is killed by a txn that does kill it.
// Key-sharded the round is two launches around the exchange: NW_EVAL leaves
// the status byte of every txn it finds blocked or killed on this rank's rows
// (the bytes are clear before it; a txn the build marked is left alone),
// NW_APPLY takes the reduced byte in place of the ballots and clears it.
// ISO_RC (not key-sharded): the words of READ_COMMITTED, see the header comment.
constexpr int NW_ONE = 0, NW_EVAL = 1, NW_APPLY = 2;
template <int MODE, int ISO = ISO_SER>
__global__ __launch_bounds__(NW_T) void k_nw_decide(NwA<MODE != NW_ONE> A, uint32_t tag,
                                                    const uint32_t* __restrict__ list,
                                                    const uint32_t* __restrict__ m_in,
                                                    uint32_t* __restrict__ list_out, uint32_t* m_out) {
  constexpr bool SH = MODE != NW_ONE;
  __shared__ uint32_t l_buf[NW_STAGE];
  __shared__ uint32_t l_cnt, l_base;
  if (threadIdx.x == 0) l_cnt = 0;
  __syncthreads();
  const Seg g = seg_of(A.lp);
  const uint32_t gpb = NW_T >> A.lp;
  const uint64_t m = list ? (uint64_t)*m_in : A.n;
  auto flush = [&]() {  // every thread of the workgroup
    const uint32_t c = l_cnt;
    if (threadIdx.x == 0 && c) l_base = atomicAdd(m_out, c);
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < c; q += NW_T) list_out[l_base + q] = l_buf[q];
    __syncthreads();
    if (threadIdx.x == 0) l_cnt = 0;
    __syncthreads();
  };
  for (uint64_t g0 = (uint64_t)blockIdx.x * gpb; g0 < m; g0 += (uint64_t)gridDim.x * gpb) {
    const uint64_t e = g0 + g.gl;
    const bool ev = e < m;
    uint32_t t = 0;
    bool act = false;
    if (ev) {
      t = list ? list[e] : (uint32_t)e;
      act = A.state[t] == ST_UNDECIDED;
      if constexpr (MODE == NW_EVAL) act = act && (list || A.stat[t] == 0);
    }
    uint32_t o0 = 0, len = 0;
    if (act) {
      o0 = A.off[t];
      len = A.off[t + 1] - o0;
    }
    const bool v = act && g.a < len;
    const uint64_t x = (uint64_t)o0 + g.a;
    uint32_t ex = 0, s = SID_NONE, ps = 0;
    bool killed, blocked;
    if constexpr (MODE == NW_APPLY) {
      const uint32_t sb = act ? A.stat[t] : 0u;  // every lane of the txn, before its lead clears the byte
      killed = sb == NW_S_KILLED;
      blocked = sb == NW_S_BLOCKED;
      if (v && sb == 0) {
        ex = is_ex(A.at[x]);
        s = A.sid[x];
      }
      if (act && g.a == 0 && sb) A.stat[t] = 0;
    } else {
      if (v) {
        ex = is_ex(A.at[x]);
        s = A.sid[x];
        if constexpr (ISO == ISO_RC) {
          if (rc_slot(s)) {
            ps = own_status(A.tab[s].aux, tag, t + 1u);
            if (ex && A.tab[s].own == 0u) ps |= PS_KILLED;  // held in any mode
          }
        } else {
          if (has_slot<SH>(s)) ps = own_status(ex ? A.tab[s].own : A.tab[s].aux, tag, t + 1u);
        }
      }
      killed = (ballot64(ps & PS_KILLED) & g.mask) != 0;
      blocked = !killed && (ballot64(ps & PS_BLOCKED) & g.mask) != 0;
    }
    if constexpr (MODE == NW_EVAL) {
      if (act && g.a == 0 && (killed || blocked)) A.stat[t] = killed ? NW_S_KILLED : NW_S_BLOCKED;
      continue;
    }
    if constexpr (ISO == ISO_RC) {  // commit: the EX locks stay to the end of the epoch
      if (v && !killed && !blocked && ex && rc_slot(s)) own_min(&A.tab[s].aux, t + 1u);
    } else if (v && !killed && !blocked && has_slot<SH>(s)) {  // commit: hold every lock to the end of the epoch
      own_min(&A.tab[s].own, t + 1u);
      if (ex) own_min(&A.tab[s].aux, t + 1u);
    }
    const bool lead = act && g.a == 0;
    if (lead && !blocked) A.state[t] = killed ? ST_ABORT : ST_COMMIT;
    const bool app = lead && blocked;
    const uint64_t bm = ballot64(app);
    if (bm) {
      uint32_t base = 0;
      if (lane_id() == 0) base = atomicAdd(&l_cnt, (uint32_t)__popcll(bm));
      base = __shfl(base, 0);
      if (app) l_buf[base + (uint32_t)__popcll(bm & lanemask_lt())] = t;
    }
    __syncthreads();
    const uint32_t staged = l_cnt;
    __syncthreads();  // every thread has read the count before the next step adds to it
    if (staged > NW_STAGE - NW_T) flush();  // the next step adds at most NW_T
  }
  if constexpr (MODE != NW_EVAL) flush();
}

// The words of round `tag` for the txns still undecided (the list of the
// round before).  Workgroup 0 clears the length word that round appends to.
template <bool SH, int ISO = ISO_SER>
__global__ __launch_bounds__(NW_T) void k_nw_publish(NwA<SH> A, uint32_t tag, const uint32_t* __restrict__ list,
                                                     const uint32_t* __restrict__ m_in, uint32_t* m_zero) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *m_zero = 0;
  const Seg g = seg_of(A.lp);
  const uint32_t gpb = NW_T >> A.lp;
  const uint64_t m = *m_in;
  for (uint64_t g0 = (uint64_t)blockIdx.x * gpb; g0 < m; g0 += (uint64_t)gridDim.x * gpb) {
    const uint64_t e = g0 + g.gl;
    if (e >= m) continue;
    const uint32_t t = list[e];
    const uint32_t o0 = A.off[t], len = A.off[t + 1] - o0;
    if (g.a >= len) continue;
    const uint64_t x = (uint64_t)o0 + g.a;
    if constexpr (ISO == ISO_RC) {  // one word per EX request; a read publishes nothing
      if (!is_ex(A.at[x])) continue;
      const uint32_t s = A.sid[x];
      if (rc_slot(s)) own_min(&A.tab[s].aux, own_word(tag, t + 1u));
      continue;
    }
    const uint32_t s = A.sid[x];
    if (!has_slot<SH>(s)) continue;
    const uint32_t w = own_word(tag, t + 1u);
    own_min(&A.tab[s].own, w);
    if (is_ex(A.at[x])) own_min(&A.tab[s].aux, w);
  }
}

__global__ __launch_bounds__(NW_T) void k_nw_retag(Slot* tab, uint64_t cap) {
  const uint64_t stride = (uint64_t)gridDim.x * NW_T;
  for (uint64_t h = (uint64_t)blockIdx.x * NW_T + threadIdx.x; h < cap; h += stride) {
    if (tab[h].key == KEY_EMPTY) continue;
    if (tab[h].own >> IDX_BITS) tab[h].own = OWN_EMPTY;
    if (tab[h].aux >> IDX_BITS) tab[h].aux = OWN_EMPTY;
  }
}

// RC bytes and the commit count; for an aborted txn the first access whose
// lock_get returned Abort: the first that names a row again with EX on either
// side, or that conflicts with a held row or with a committed txn below it
// (the committed-only words: tag 0).
// Key-sharded: the first such access among this rank's rows, as 64 - its
// ordinal in the whole txn (1 .. 64, MAX_TXN_LEN is 64; 0: none here) into the
// status byte, whose byte-MAX over the ranks is the lowest ordinal
// (k_nw_conf); `conflict` only says whether the ordinals are wanted.
// READ_COMMITTED: the first access that has an earlier EX of its own on its
// slot, or a tag-0 `aux` word below the txn, or (when EX) a held row.
template <bool SH, int ISO = ISO_SER>
__global__ __launch_bounds__(NW_T) void k_nw_final(NwA<SH> A, uint8_t* __restrict__ rc,
                                                   uint32_t* __restrict__ conflict) {
  __shared__ uint32_t s_commit;
  if (threadIdx.x == 0) s_commit = 0;
  __syncthreads();
  const Seg g = seg_of(A.lp);
  const uint32_t gpb = NW_T >> A.lp;
  uint32_t commits = 0;
  for (uint64_t g0 = (uint64_t)blockIdx.x * gpb; g0 < A.n; g0 += (uint64_t)gridDim.x * gpb) {
    const uint64_t t = g0 + g.gl;
    const bool tv = t < A.n;
    const uint8_t st = tv ? A.state[t] : (uint8_t)ST_COMMIT;
    const bool ab = tv && st != ST_COMMIT;
    if (tv && g.a == 0) {
      rc[t] = st == ST_COMMIT ? DCC_RC_RCOK : DCC_RC_ABORT;
      commits += st == ST_COMMIT ? 1u : 0u;
      if (st == ST_UNDECIDED) atomicOr(&A.cnt[SEG_C_ERR], NW_ERR_STATE);
    }
    if (!conflict) continue;
    if (!ballot64(ab)) {  // no aborted txn in the wave
      if (tv && g.a == 0) {
        if constexpr (SH) A.stat[t] = 0;
        else conflict[t] = DCC_ACCESS_NONE;
      }
      continue;
    }
    uint32_t o0 = 0, len = 0;
    if (ab) {
      o0 = A.off[t];
      len = A.off[t + 1] - o0;
    }
    const bool v = ab && g.a < len;
    const uint64_t x = (uint64_t)o0 + g.a;
    uint32_t ex = 0, s = SID_NONE;
    bool c = false;
    if (v) {
      ex = is_ex(A.at[x]);
      s = A.sid[x];
      if constexpr (ISO == ISO_RC) {
        if (rc_slot(s)) {
          const uint32_t w = A.tab[s].aux;
          c = ((w >> IDX_BITS) == 0 && (w & IDX_MASK) < (uint32_t)t + 1u) || (ex && A.tab[s].own == 0u);
        }
      } else if (has_slot<SH>(s)) {
        const uint32_t w = ex ? A.tab[s].own : A.tab[s].aux;
        c = (w >> IDX_BITS) == 0 && (w & IDX_MASK) < (uint32_t)t + 1u;
      }
    }
    if constexpr (ISO == ISO_RC) c = self_conflict_rc(g, A.lp, v, s, ex) || c;
    else c = self_conflict<SH>(g, A.lp, v, s, ex) || c;
    const uint64_t cb = ballot64(c) & g.mask;
    if (tv && g.a == 0) {
      if constexpr (SH) {
        A.stat[t] = ab && cb ? (uint8_t)(MAX_TXN_LEN - ((uint32_t)__builtin_ctzll(cb) - g.seg0)) : (uint8_t)0;
      } else {
        uint32_t o = DCC_ACCESS_NONE;
        if (ab) {
          if (cb) o = (uint32_t)__builtin_ctzll(cb) - g.seg0;
          else atomicOr(&A.cnt[SEG_C_ERR], NW_ERR_STATE);  // aborted without a conflicting request
        }
        conflict[t] = o;
      }
    }
  }
  if (commits) atomicAdd(&s_commit, commits);
  __syncthreads();
  if (threadIdx.x == 0 && s_commit) atomicAdd(&A.cnt[NW_C_COMMIT], s_commit);
}

// Key-sharded: the conflict ordinals from the reduced bytes of k_nw_final.
__global__ __launch_bounds__(NW_T) void k_nw_conf(uint64_t n, const uint8_t* __restrict__ state,
                                                  const uint8_t* __restrict__ stat, uint32_t* __restrict__ conflict,
                                                  uint32_t* __restrict__ cnt) {
  const uint64_t stride = (uint64_t)gridDim.x * NW_T;
  for (uint64_t t = (uint64_t)blockIdx.x * NW_T + threadIdx.x; t < n; t += stride) {
    const uint32_t b = stat[t];
    const bool ab = state[t] != ST_COMMIT;
    if (ab && !b) atomicOr(&cnt[SEG_C_ERR], NW_ERR_STATE);  // aborted without a conflicting request on any rank
    conflict[t] = ab && b ? MAX_TXN_LEN - b : DCC_ACCESS_NONE;
  }
}

// ------------------------------------------------------------------ host
// What the call asks for, resolved once (nw_plan) before anything is staged.
// The per-epoch table is sized from (m, hn) before the check, from the check's
// counts after it, or not built at all (nw_rows).
constexpr int NW_TAB_NONE = 0, NW_TAB_EARLY = 1, NW_TAB_LATE = 2;
struct NwPlan {
  bool sh = false;   // key-sharded: the batch is the whole epoch on every rank (DCC_SHARD_SELF)
  bool lt = false;   // a lock table's held rows take the place of a held list
  bool dev = false;  // DCC_DEVICE_PTRS
  int iso = ISO_SER, tab = NW_TAB_EARLY;
  uint32_t iso_bits = 0;  // the batch's DCC_ISO_* bits
  uint64_t hn = 0;        // held rows
};

// One epoch's launch state (as tso_kernels.h's TsRun): the phases fill and read it.
struct NwRun {
  NwPlan P;
  DevBatch d;
  uint64_t n = 0, m = 0, cap = 0, nnz_ex = 0, per_block = 0;
  uint32_t rounds = 0;
  unsigned max_grid = 1;
  uint32_t *cnt = nullptr, *ring = nullptr, *lists[2] = {}, *conf_dev = nullptr;
  uint8_t* rc_dev = nullptr;
  const uint64_t* hk = nullptr;  // the held list on the device
  const uint8_t* ha = nullptr;
  NwShArgs A{};  // the kernels that are not key-sharded take its NwArgs
  LtEpoch L;
};

// Every host-side rejection of a call, in the order the caller sees them.
int nw_plan(dcc_ctx* ctx, const dcc_batch* b, const dcc_calvin_held* held, bool lt, NwPlan& P) {
  CR(ctx->check_batch(b, false));  // the offsets are checked on the device (k_batch_check)
  // key-sharded: the batch is the whole epoch on every rank (DCC_SHARD_SELF); a lock table is one GPU's
  P.lt = lt;
  P.sh = !lt && ctx->sharded() && (b->flags & DCC_SHARD_SELF) != 0;
  if (ctx->comm_ranks() > 1 && !P.sh)
    return ctx->fail(DCC_ENOTSUP,
                     "nowait: more than one rank takes the whole epoch with DCC_SHARD_SELF and no lock table");
  P.iso_bits = b->flags & (DCC_ISO_READ_COMMITTED | DCC_ISO_READ_UNCOMMITTED);
  if (P.iso_bits == (DCC_ISO_READ_COMMITTED | DCC_ISO_READ_UNCOMMITTED))
    return ctx->fail(DCC_EINVAL, "nowait: both isolation bits set");
  P.iso = P.iso_bits == DCC_ISO_READ_COMMITTED ? ISO_RC : P.iso_bits ? ISO_RU : ISO_SER;
  if (P.sh && P.iso != ISO_SER)  // on every rank alike, before any collective
    return ctx->fail(DCC_ENOTSUP, "nowait: a key-sharded epoch is SERIALIZABLE only");
  P.hn = held ? held->n : 0;
  if (lt && P.hn) return ctx->fail(DCC_EINVAL, "nowait: a held list next to a lock table");
  if (P.hn && (!held->keys || !held->acctype)) return ctx->fail(DCC_EINVAL, "nowait: null held keys/acctype");
  P.dev = (b->flags & DCC_DEVICE_PTRS) != 0;
  if (b->n_txn >= (uint64_t)IDX_MASK)  // owner words carry index + 1
    return ctx->fail(DCC_ERANGE, "nowait: n_txn %llu exceeds %u", (unsigned long long)b->n_txn, IDX_MASK - 1);
  P.tab = P.sh || (P.iso == ISO_RC && !lt) ? NW_TAB_LATE : P.iso == ISO_RU && !lt && !P.hn ? NW_TAB_NONE : NW_TAB_EARLY;
  return DCC_OK;
}

// The rows the per-epoch table must hold; `hc`: the check's counted words, of a
// table sized late.  Key-sharded: the rank's own requests and held rows.  A lock
// table: every request keeps a slot (k_lt_seed marks the held rows through
// them; READ_UNCOMMITTED: of the table's rows at most one per request).
// READ_COMMITTED: the held rows and the EX requests.  READ_UNCOMMITTED: the held
// rows alone (NW_TAB_NONE without them).
uint64_t nw_rows(const NwPlan& P, uint64_t m, const uint32_t* hc) {
  if (P.sh) return (uint64_t)hc[NW_C_OWN] + hc[NW_C_OWNHELD];
  if (P.lt) return m;
  if (P.iso == ISO_RC) return (uint64_t)hc[NW_C_EXREQ] + P.hn;
  return P.iso == ISO_RU ? P.hn : m + P.hn;
}
int nw_table(dcc_ctx* ctx, NwRun& R, uint64_t rows) {
  R.cap = dcc_ctx::table_capacity(rows);
  if (R.cap > (1ull << 30)) return ctx->fail(DCC_ERANGE, "nowait: table capacity exceeds 2^30 slots");
  return ctx->table.ensure(ctx, R.cap * sizeof(Slot), "table");
}

// The workspaces, the held list on the device, and the check: a malformed
// batch is rejected before anything indexes with its offsets (every rank
// checks the whole batch and the whole held list: all reject alike, before any
// collective).  Next to it the counts that size a late table.
int nw_check(dcc_ctx* ctx, NwRun& R, const dcc_calvin_held* held, uint8_t* out_rc, uint32_t* out_conflict) {
  const NwPlan& P = R.P;
  hipStream_t stream = ctx->stream;
  const uint64_t n = R.n, m = R.m;
  CR(ctx->nowait_reserve(n, m, out_conflict != nullptr && !P.dev, false));
  uint32_t* cnt = R.cnt = (uint32_t*)ctx->nw_misc.p;
  R.ring = cnt + NW_C_RING;
  R.lists[0] = (uint32_t*)ctx->nw_list.p;
  R.lists[1] = R.lists[0] + n;
  R.rc_dev = P.dev ? out_rc : (uint8_t*)ctx->rc.p;
  R.conf_dev = out_conflict ? (P.dev ? out_conflict : (uint32_t*)ctx->nw_conf.p) : nullptr;
  R.max_grid = (unsigned)ctx->n_cu * 16;
  const NwOwn who{(uint32_t)ctx->comm_rank(), (uint32_t)ctx->comm_ranks()};
  CR(ctx->stage_held(held, P.dev, R.hk, R.ha));

  CK(hipMemsetAsync(cnt, 0, NW_C_WORDS * 4, stream));
  k_batch_check<false><<<launch_grid(std::max(n, m), CHK_T * 4, R.max_grid), CHK_T, 0, stream>>>(
      R.d.off, n, R.d.keys, m, cnt);
  if (P.sh)
    k_nw_count<<<launch_grid(std::max(m, P.hn), CHK_T * 4, R.max_grid), CHK_T, 0, stream>>>(R.d.keys, m, R.hk, P.hn,
                                                                                          who, cnt);
  if (P.iso == ISO_RC)
    k_nw_count_ex<<<launch_grid(m, CHK_T * 4, R.max_grid), CHK_T, 0, stream>>>(R.d.acctype, m, cnt);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(ctx->hmisc, cnt, P.sh || P.iso == ISO_RC ? NW_C_RING * 4 : 8, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  const uint32_t* hc = (const uint32_t*)ctx->hmisc;
  BatchShape shape;
  CR(batch_checked(ctx, hc, m, false, shape));
  if (P.sh && (hc[SEG_C_ERR] & NW_ERR_HKEY))
    return ctx->fail(DCC_EINVAL, "nowait: held key equal to DCC_KEY_RESERVED");
  R.nnz_ex = P.iso == ISO_RC ? hc[NW_C_EXREQ] : 0;
  R.per_block = NW_T >> shape.lp;  // txns per workgroup step
  R.A = NwShArgs{NwArgs{n, R.d.off, R.d.keys, R.d.acctype, nullptr, 0, shape.lp, (uint32_t*)ctx->nw_sid.p,
                        (uint8_t*)ctx->state.p, cnt},
                 who, (uint8_t*)ctx->nw_stat.p};  // tab and mask: nw_build
  return DCC_OK;
}

// What the lock table's passes read of the epoch.
LtEpoch nw_lt_epoch(const NwArgs& A, unsigned grid, int iso) {
  return LtEpoch{A.n, A.off, A.keys, A.at, A.sid, A.state, A.tab, A.lp, &A.cnt[SEG_C_ERR], grid, A.mask, iso};
}

// The table: cleared, the held rows, every request (k_nw_ru looks the held
// rows up itself: READ_UNCOMMITTED builds nothing).  A lock table's held rows
// take the place of a held list: their tag-0 words (locktab_seed).
int nw_build(dcc_ctx* ctx, NwRun& R, dcc_locktab* lt) {
  const NwPlan& P = R.P;
  hipStream_t stream = ctx->stream;
  const uint64_t n = R.n, cap = R.cap;
  CK(hipEventRecord(ctx->ev0, stream));
  if (ctx->profiling) CK(hipEventRecord(ctx->pev[0], stream));
  // room for every request that can stay, or DCC_ERANGE
  if (lt) CR(ctx->locktab_begin(lt, P.iso == ISO_RC ? R.nnz_ex : P.iso == ISO_RU ? 0 : R.m, "lock epoch"));
  Slot* tab = R.A.tab = cap ? (Slot*)ctx->table.p : nullptr;
  const uint32_t mask = R.A.mask = (uint32_t)(cap - 1);
  if (cap) CK(hipMemsetAsync(tab, 0xFF, cap * sizeof(Slot), stream));
  if (P.hn) {
    const unsigned hgrid = launch_grid(P.hn, NW_T, R.max_grid);
    if (P.sh) k_nw_held<true><<<hgrid, NW_T, 0, stream>>>(R.hk, R.ha, P.hn, tab, mask, R.cnt, R.A.who);
    else k_nw_held<false><<<hgrid, NW_T, 0, stream>>>(R.hk, R.ha, P.hn, tab, mask, R.cnt, NwAll{});
  }
  const unsigned grid = launch_grid(n, R.per_block, R.max_grid);
  if (P.sh) {
    CK(hipMemsetAsync(R.A.stat, 0, n, stream));  // every pass that sets a byte clears it again
    k_nw_build<true><<<grid, NW_T, 0, stream>>>(R.A);
  } else if (P.iso == ISO_RC) {
    k_nw_build_ex<<<grid, NW_T, 0, stream>>>(R.A);
    k_nw_build_rd<<<grid, NW_T, 0, stream>>>(R.A, lt != nullptr);
  } else if (P.iso == ISO_SER) {
    k_nw_build<false><<<grid, NW_T, 0, stream>>>(R.A);
  }
  CK(hipGetLastError());
  if (lt) {
    R.L = nw_lt_epoch(R.A, grid, P.iso);
    CR(ctx->locktab_seed(lt, R.L));
  }
  if (ctx->profiling) CK(hipEventRecord(ctx->pev[1], stream));
  return DCC_OK;
}

// The rounds (seg_rounds.h's loop): decide(r) reads its list length `left` and
// appends the blocked txns to the list whose length word publish(r) cleared
// (the whole ring is clear before round 1, which takes every txn and clears
// nothing).  Rounds past the fixed point find empty lists.  `bound` sizes the
// grids.  Then the RC bytes and the conflict ordinals.
// Key-sharded, the state bytes and so the ring are the same on every rank:
// every rank enqueues the same rounds, the ones past the fixed point too, and
// each of them makes its one exchange.
template <bool SH, int ISO>
int nw_rounds(dcc_ctx* ctx, NwRun& R) {
  static_assert(!(SH && ISO != ISO_SER), "a key-sharded epoch is SERIALIZABLE only");
  hipStream_t stream = ctx->stream;
  const NwA<SH> A = R.A;  // the lambda's arguments in locals, as they were
  uint32_t* lists[2] = {R.lists[0], R.lists[1]};
  const uint64_t n = R.n, cap = R.cap, per_block = R.per_block;
  const unsigned max_grid = R.max_grid;
  // READ_COMMITTED: one more round than SERIALIZABLE at most: the words of the self-aborted txns
  const uint64_t max_r = n + (ISO == ISO_RC ? 3 : 2);
  auto round = [&](uint32_t r, const uint32_t* left, uint32_t* left_out, uint64_t bound) {
    const uint32_t er = (r - 1) % MAX_TAG_ROUND + 1;  // tags 62 .. 1, then again
    const uint32_t tag = round_tag(er);
    const uint32_t* lin = r > 1 ? lists[r & 1] : nullptr;
    const unsigned grid = launch_grid(bound, per_block, max_grid);
    if (r > 1) {
      if (er == 1)  // tag space exhausted: drop the tagged words, every undecided txn republishes
        k_nw_retag<<<launch_grid(cap, NW_T * 4, max_grid), NW_T, 0, stream>>>(A.tab, cap);
      k_nw_publish<SH, ISO><<<grid, NW_T, 0, stream>>>(A, tag, lin, left, left_out);
    }
    if constexpr (SH) {  // evaluate / all-reduce / apply; the collective can fail
      k_nw_decide<NW_EVAL><<<grid, NW_T, 0, stream>>>(A, tag, lin, left, nullptr, nullptr);
      CR(ctx->comm_allreduce_max_u8(A.stat, n));
      k_nw_decide<NW_APPLY><<<grid, NW_T, 0, stream>>>(A, tag, lin, left, lists[(r + 1) & 1], left_out);
      return DCC_OK;
    } else {
      k_nw_decide<NW_ONE, ISO><<<grid, NW_T, 0, stream>>>(A, tag, lin, left, lists[(r + 1) & 1], left_out);
    }
  };
  CR(rounds_loop(ctx, R.ring, n, max_r, "nowait", R.rounds, round));
  k_nw_final<SH, ISO><<<launch_grid(n, per_block, max_grid), NW_T, 0, stream>>>(A, R.rc_dev, R.conf_dev);
  if constexpr (SH) {
    if (R.conf_dev) {  // the lowest conflicting ordinal over the ranks
      CR(ctx->comm_allreduce_max_u8(A.stat, n));
      k_nw_conf<<<launch_grid(n, NW_T * 4, max_grid), NW_T, 0, stream>>>(n, A.state, A.stat, R.conf_dev, R.cnt);
    }
  }
  return DCC_OK;
}

int nw_decide(dcc_ctx* ctx, NwRun& R) {
  if (R.P.sh) return nw_rounds<true, ISO_SER>(ctx, R);
  if (R.P.iso == ISO_RC) return nw_rounds<false, ISO_RC>(ctx, R);
  if (R.P.iso == ISO_SER) return nw_rounds<false, ISO_SER>(ctx, R);
  // READ_UNCOMMITTED, no rounds: one pass against the held rows
  hipStream_t stream = ctx->stream;
  if (ctx->profiling) CK(hipEventRecord(ctx->pev[2], stream));
  k_nw_ru<<<launch_grid(R.n, R.per_block, R.max_grid), NW_T, 0, stream>>>(R.A, R.rc_dev, R.conf_dev);
  if (ctx->profiling) CK(hipEventRecord(ctx->pev[3], stream));
  return DCC_OK;
}

// The lock table's grants, the outputs and the counts.
int nw_readout(dcc_ctx* ctx, NwRun& R, dcc_locktab* lt, uint8_t* out_rc, uint32_t* out_conflict, EpochStats& es) {
  hipStream_t stream = ctx->stream;
  const uint64_t n = R.n;
  dcc_stats& S = es.S;
  CK(hipGetLastError());
  if (lt) CR(ctx->locktab_grant(lt, R.L));  // the committed txns' requests stay in the table
  if (ctx->profiling) CK(hipEventRecord(ctx->pev[4], stream));
  CK(hipEventRecord(ctx->ev1, stream));
  if (!R.P.dev) {
    CK(hipMemcpyAsync(out_rc, R.rc_dev, n, hipMemcpyDeviceToHost, stream));
    if (out_conflict) CK(hipMemcpyAsync(out_conflict, R.conf_dev, n * 4, hipMemcpyDeviceToHost, stream));
  }
  CK(hipMemcpyAsync(ctx->hmisc, R.cnt, NW_C_RING * 4, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  const uint32_t* hc = (const uint32_t*)ctx->hmisc;
  if (hc[SEG_C_ERR] & CHK_ERR_KEY) return ctx->fail(DCC_EINVAL, "nowait: held key equal to DCC_KEY_RESERVED");
  if (hc[SEG_C_ERR] & NW_ERR_FULL) return ctx->fail(DCC_EIO, "nowait: lock table full");
  if (hc[SEG_C_ERR] & NW_ERR_STATE) return ctx->fail(DCC_EIO, "nowait: inconsistent decisions");
  S.rounds = R.rounds;
  S.n_commit = hc[NW_C_COMMIT];
  S.n_abort = n - hc[NW_C_COMMIT];
  S.nnz_w = hc[NW_C_NEX];
  S.n_readonly = hc[NW_C_RO];
  S.alg_bytes = dcc_nowait_iso_alg_bytes(n, R.m, R.P.hn, out_conflict != nullptr, R.P.iso_bits);
  if (lt) {
    uint64_t granted = 0;
    CR(ctx->locktab_end(lt, &granted));
    S.alg_bytes = dcc_locktab_epoch_alg_bytes(n, R.m, granted, out_conflict != nullptr);
  }
  return es.finish(ctx, 4);
}

}  // namespace

int dcc_ctx::nowait_reserve(uint64_t n, uint64_t nnz, bool with_conflict, bool whole_table) {
  CR(nw_misc.ensure(this, NW_C_WORDS * 4, "nowait counters"));
  CR(nw_stat.ensure(this, n + 16, "nowait status bytes"));
  CR(nw_sid.ensure(this, std::max<uint64_t>(nnz, 1) * 4, "nowait slot ids"));
  CR(nw_list.ensure(this, 2 * std::max<uint64_t>(n, 1) * 4, "nowait undecided lists"));
  if (with_conflict) CR(nw_conf.ensure(this, std::max<uint64_t>(n, 1) * 4, "nowait conflicts"));
  CR(state.ensure(this, n + 16, "state"));
  CR(rc.ensure(this, n + 16, "rc"));
  if (whole_table) CR(table.ensure(this, table_capacity(nnz) * sizeof(Slot), "table"));
  return DCC_OK;
}

// The epoch as phases over one NwRun: plan / table (sized early) / check and
// count / table (sized late) / build / rounds / read-out.
int dcc_ctx::nowait_epoch(const dcc_batch* b, const dcc_calvin_held* held, uint8_t* out_rc,
                          uint32_t* out_conflict, dcc_stats* st, dcc_locktab* lt) {
  EpochStats es;
  if (!out_rc) return fail(DCC_EINVAL, "nowait: null out_rc");
  NwRun R;
  CR(nw_plan(this, b, held, lt != nullptr, R.P));
  if (R.P.sh) es.S.n_shards = (uint32_t)comm_ranks();
  if (b->n_txn == 0) {
    if (st) *st = es.S;
    return DCC_OK;
  }
  CR(stage_batch(b, R.d));
  R.n = R.d.n;
  R.m = R.d.nnz;
  if (R.P.tab == NW_TAB_EARLY) CR(nw_table(this, R, nw_rows(R.P, R.m, nullptr)));
  CR(nw_check(this, R, held, out_rc, out_conflict));
  if (R.P.tab == NW_TAB_LATE) CR(nw_table(this, R, nw_rows(R.P, R.m, (const uint32_t*)hmisc)));
  CR(nw_build(this, R, lt));
  CR(nw_decide(this, R));
  CR(nw_readout(this, R, lt, out_rc, out_conflict, es));
  if (st) *st = es.S;
  return DCC_OK;
}

extern "C" uint64_t dcc_nowait_alg_bytes(uint64_t n_txn, uint64_t nnz, int with_conflict) {
  // offsets, key + access type per request, one 16-B lock-table slot per
  // request, RC byte, conflict ordinal
  return 4 * (n_txn + 1) + 9 * nnz + 16 * nnz + n_txn + (with_conflict ? 4 * n_txn : 0);
}

extern "C" uint64_t dcc_nowait_iso_alg_bytes(uint64_t n_txn, uint64_t nnz, uint64_t held_n, int with_conflict,
                                             uint32_t flags) {
  // READ_COMMITTED: a read still probes one slot.  READ_UNCOMMITTED without held rows builds no table.
  const uint64_t all = dcc_nowait_alg_bytes(n_txn, nnz, with_conflict);
  const bool ru = (flags & (DCC_ISO_READ_COMMITTED | DCC_ISO_READ_UNCOMMITTED)) == DCC_ISO_READ_UNCOMMITTED;
  return ru && held_n == 0 ? all - 16 * nnz : all;
}

extern "C" int dcc_nowait_lock_epoch(dcc_ctx* ctx, const dcc_batch* batch, const dcc_calvin_held* held,
                                     uint8_t* out_rc, uint32_t* out_conflict, dcc_stats* out_stats) {
  if (!ctx || !batch || !out_rc) return DCC_EINVAL;
  dcc_pipe_drain(ctx);  // pipelined OCC epochs in flight complete first
  if (ctx->multi && (batch->flags & DCC_SHARD_SELF) && dcc_multi_size(ctx) > 1) {  // key-sharded over the ranks
    // nw_plan's rejection, kept here too: it comes before dcc_multi_nowait_epoch's own checks and
    // its empty-batch exit, and answers both isolation bits with DCC_ENOTSUP (one context: DCC_EINVAL)
    if (batch->flags & (DCC_ISO_READ_COMMITTED | DCC_ISO_READ_UNCOMMITTED))
      return ctx->fail(DCC_ENOTSUP, "nowait: a key-sharded epoch is SERIALIZABLE only");
    return dcc_multi_nowait_epoch(ctx, batch, held, out_rc, out_conflict, out_stats);
  }
  if (ctx->multi)  // without the flag: the whole epoch on rank 0, no collective
    return dcc_multi_on_rank0(ctx, true, [&](dcc_ctx* s) {
      return s->nowait_epoch(batch, held, out_rc, out_conflict, out_stats);
    });
  if (hipSetDevice(ctx->device) != hipSuccess) return DCC_ENODEV;
  return ctx->nowait_epoch(batch, held, out_rc, out_conflict, out_stats);
}
