// Multi-version timestamp ordering (CC_ALG MVCC) for a whole epoch
// (dcc_mvcc_validate_epoch), with the rows' latest version / rts persistent in
// the context's third row table and every row version in a device-resident
// store that epochs append to and dcc_mvcc_trim cuts.
//
// Reference: concurrency_control/row_mvcc.cpp, in the one-txn-in-flight model
// of the TIMESTAMP engine (tso.hip): the txns run in index
// order, each one atomically.  With no second txn in flight Row_mvcc::access
// reduces to (DESIGN.md §8l has the argument, tests/mvcc_ref.py checks it):
//
//   R_REQ  never waits, never aborts: returns the newest-inserted version with
//          wts <= ts, else the base row (:266-270); rts = max(rts, ts)
//   P_REQ  abort iff ts < rts, rts the largest read timestamp of the row
//          (:218-239: the write timestamps are a subset of the read ones)
//   W_REQ  installs the version ts (a committed txn's WR accesses)
//   XP_REQ drops the prewrite: the rts bumps of an aborted txn stay
//
// So the decisions are TIMESTAMP's rounds with one difference -- a RD / SCAN
// never stops or fails its txn -- and run on tso_kernels.h's kernels with the
// engine type Mv.  A committed writer passed ts >= rts >= every version of the
// row, so a row's versions are non-decreasing in ts in commit order, across
// epochs too, and "the newest-inserted version with wts <= ts" is the last
// element of a prefix of the row's version list: it can be binary-searched.
//
// After the decisions:
//   final apply   (k_ts_scan<apply, final, Mv>)  every executed non-XP access
//                 with ts > dw -- dw the exclusive segmented prefix maximum of
//                 the committed writers' ts, the row's latest version at the
//                 head -- sees dw.  ts <= dw is late: dw == ts may be the
//                 txn's own earlier WR of the row, which it must not see, or a
//                 tie with another txn, which it must; late accesses are
//                 appended to a list (one atomic per wave, any order).  A
//                 segment's last element leaves the row's new (latest version,
//                 rts) next to its slot; nothing writes the rows here.
//   k_mv_commits  <count> / k_mv_offsets / <compact>: the sorted records with
//                 "WR and txn committed", compacted in order into (key, ts,
//                 txn): the epoch's versions in (row, index) order, which is
//                 (row, ts) order.  Row order is raw key order: the sort runs
//                 on KeyPack-packed keys, and make_keypack (radix_sort.hip)
//                 takes the varying bits from bit 0 up into ascending
//                 positions, an order-preserving extraction for keys that
//                 agree in every other bit, as a batch's do by construction.
//   k_mv_lookup   one lane per late access: binary search of the epoch list
//                 with the prefix-closed predicate key < K || (key == K &&
//                 txn < i && ts <= t); if the element found is not of row K,
//                 binary search of the store as it was before the epoch with
//                 (key, ts) <= (K, t); else the base row.
//   k_mv_merge    store + epoch list into the store's other buffer by rank:
//                 an element's position is its index plus a binary search in
//                 the other side, old elements before new ones of a key.
//   k_mv_rows     the rows' new values, from what the final apply left.
// k_mv_rows returns at once if the epoch's error word is set, and the host
// swaps the store's buffers only if it is clear: after an epoch that fails
// behind the decisions the rows and the store are those from before it (rows
// the batch named are in the table as (0, 0), which reads as unknown).
// Nothing spins and no workgroup waits on another.
#include <hip/hip_runtime.h>

#include "dcc.h"
#include "dcc_ctx.h"

using namespace dcc;

namespace dcc {
namespace {
constexpr uint32_t TS_T = 256;                    // threads per workgroup
constexpr uint32_t TS_ITEMS = 4;                  // consecutive sorted accesses per thread
}  // namespace
}  // namespace dcc

#include "mvcc_store.h"
#include "tso_kernels.h"

namespace {

// engine counter words (next to tso_kernels.h's): late accesses; the epoch's versions (u64)
constexpr uint32_t MV_C_NLATE = TS_C_ENGINE, MV_C_NC = TS_C_ENGINE + 2;
static_assert(TS_T == MVS_T, "the store kernels' workgroup");

struct MvScanArgs : ScanArgs {
  uint64_t* vts;     // [m] the version of every access, batch order (null: not wanted)
  uint32_t* late;    // [m] the late accesses
  uint32_t* nlate;
  uint32_t* lslot;   // [m] at a segment's last element: the row's slot
  ulonglong2* rowv;  //     and its new (latest version, rts)
};

// tso_kernels.h's engine: a read never fails, the final apply resolves the
// versions and leaves the rows' new values for k_mv_rows.
struct Mv {
  static constexpr bool MVCC = true;
  static constexpr const char* name = "mvcc";
  using Scan = MvScanArgs;
  struct Out {
    uint32_t x[TS_ITEMS];
    uint32_t mask = 0;  // bit k: the thread's k-th access is late
  };
  // dw: the newest version installed before the access
  __device__ static void access_out(const MvScanArgs& A, Out& o, uint32_t k, uint32_t x, uint32_t info,
                                    uint32_t st, uint64_t ts, uint64_t dw) {
    if (!A.vts) return;
    const uint32_t q = info & 0xFFu, ty = (info >> 8) & 3u;
    const bool exec = ty != DCC_XP && (st_state(st) == ST_COMMIT || q < st_prog(st));
    o.x[k] = x;
    if (!exec) A.vts[x] = DCC_VTS_NONE;
    else if (ts > dw) A.vts[x] = dw;
    else o.mask |= 1u << k;
  }
  __device__ static void row_out(const MvScanArgs& A, uint64_t s, uint32_t slot, uint64_t dw, uint64_t de) {
    A.lslot[s] = slot;
    A.rowv[s] = make_ulonglong2(dw, de);
  }
  // the thread's late accesses behind the wave's: one atomic per wave (every
  // lane of the wave is here)
  __device__ static void flush(const MvScanArgs& A, const Out& o) {
    if (!A.vts) return;
    uint32_t total;
    const uint32_t ex = wave_excl<AddOp<uint32_t>>((uint32_t)__popc(o.mask), total);
    if (!total) return;
    uint32_t b = 0;
    if (lane_id() == 0) b = atomicAdd(A.nlate, total);
    uint32_t pos = (uint32_t)__shfl(b, 0) + ex;
#pragma unroll
    for (uint32_t k = 0; k < TS_ITEMS; k++)
      if ((o.mask >> k) & 1u) A.late[pos++] = o.x[k];
  }
};

// a timestamp of 0 (Row_mvcc::conflict's "none", and the base row of out_vts)
// or UINT64_MAX (DCC_VTS_NONE) rejects the batch
__global__ __launch_bounds__(TS_T) void k_mv_tscheck(const uint64_t* __restrict__ ts, uint64_t n,
                                                     uint32_t* __restrict__ cnt) {
  bool bad = false;
  for (uint64_t t = (uint64_t)blockIdx.x * TS_T + threadIdx.x; t < n; t += (uint64_t)gridDim.x * TS_T) {
    const uint64_t v = ts[t];
    bad |= v == 0 || v == ~0ull;
  }
  if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(&cnt[SEG_C_ERR], TS_ERR_TS);
}

// ----------------------------------------------------- the epoch's versions
// One TS_TILE tile of the sorted records per workgroup, 4 consecutive per
// thread.  !SCATTER: the tile's number of committed WR records into toff.
// SCATTER: behind the tile's offset (toff after k_mv_offsets) the committed WR
// records in order: (raw key, ts, txn).
template <bool SCATTER>
__global__ __launch_bounds__(TS_T) void k_mv_commits(uint64_t m, const uint32_t* __restrict__ s_info,
                                                     const uint32_t* __restrict__ s_txn,
                                                     const uint64_t* __restrict__ s_ts,
                                                     const uint32_t* __restrict__ sv,
                                                     const uint32_t* __restrict__ stp,
                                                     const uint64_t* __restrict__ keys, uint64_t* toff,
                                                     uint64_t* __restrict__ ek, uint64_t* __restrict__ et,
                                                     uint32_t* __restrict__ ex) {
  __shared__ uint32_t s_w[TS_T / 64];
  const uint64_t base = (uint64_t)blockIdx.x * TS_TILE + (uint64_t)threadIdx.x * TS_ITEMS;
  uint32_t txn[TS_ITEMS], mask = 0;
#pragma unroll
  for (uint32_t k = 0; k < TS_ITEMS; k++) {
    txn[k] = 0;
    if (base + k < m) {
      txn[k] = s_txn[base + k];
      const bool cw = ((s_info[base + k] >> 8) & 3u) == DCC_WR && st_state(stp[txn[k]]) == ST_COMMIT;
      mask |= cw ? 1u << k : 0u;
    }
  }
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
      ex[pos] = txn[k];
      pos++;
    }
}

// ------------------------------------------------------------- late lookup
__global__ __launch_bounds__(TS_T) void k_mv_lookup(const uint32_t* __restrict__ late,
                                                    const uint32_t* __restrict__ nlate,
                                                    const uint64_t* __restrict__ keys,
                                                    const uint4* __restrict__ arec,
                                                    const uint64_t* __restrict__ ek,
                                                    const uint64_t* __restrict__ et,
                                                    const uint32_t* __restrict__ ex,
                                                    const uint64_t* __restrict__ nc_p, MvStore S,
                                                    uint64_t* __restrict__ vts) {
  const uint32_t nl = *nlate;
  const uint64_t nc = *nc_p;
  for (uint64_t l = (uint64_t)blockIdx.x * TS_T + threadIdx.x; l < nl; l += (uint64_t)gridDim.x * TS_T) {
    const uint32_t x = late[l];
    const uint4 r = arec[x];
    const uint32_t i = r.x;
    const uint64_t t = (uint64_t)r.z | ((uint64_t)r.w << 32), K = keys[x];
    // the epoch's versions of row K installed before txn i with wts <= t end
    // the prefix of the list that the predicate holds for
    uint64_t lo = 0, hi = nc;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      const uint64_t kk = ek[mid];
      if (kk < K || (kk == K && ex[mid] < i && et[mid] <= t)) lo = mid + 1;
      else hi = mid;
    }
    uint64_t v = DCC_VTS_BASE;
    if (lo && ek[lo - 1] == K) {
      v = et[lo - 1];
    } else {
      const uint64_t p = mv_upper(S.k, S.t, S.n, K, t);
      if (p && S.k[p - 1] == K) v = S.t[p - 1];
    }
    vts[x] = v;
  }
}

// The rows' new (latest version, rts), one plain store pair per row; nothing
// if the epoch's error word is set.
__global__ __launch_bounds__(TS_T) void k_mv_rows(uint64_t m, const uint32_t* __restrict__ s_info,
                                                  const uint32_t* __restrict__ lslot,
                                                  const ulonglong2* __restrict__ rowv, RowSlot* tab,
                                                  const uint32_t* __restrict__ err) {
  if (*err) return;
  for (uint64_t s = (uint64_t)blockIdx.x * TS_T + threadIdx.x; s < m; s += (uint64_t)gridDim.x * TS_T) {
    if (!(s_info[s] & TS_I_LAST)) continue;
    const ulonglong2 v = rowv[s];
    RowSlot* r = &tab[lslot[s]];
    r->*WTS = v.x;
    r->*RTS = v.y;
  }
}

// clear_history(W_REQ, floor) of every row (row_mvcc.cpp:42-73): a version
// goes iff the next newer version of its row is below the floor too.  Tiles of
// TS_TILE store elements; !SCATTER counts the kept ones, SCATTER moves them.
template <bool SCATTER>
__global__ __launch_bounds__(TS_T) void k_mv_trim(MvStore S, uint64_t floor, uint64_t* toff,
                                                  uint64_t* __restrict__ dk, uint64_t* __restrict__ dt) {
  __shared__ uint32_t s_w[TS_T / 64];
  const uint64_t base = (uint64_t)blockIdx.x * TS_TILE + (uint64_t)threadIdx.x * TS_ITEMS;
  uint32_t mask = 0;
#pragma unroll
  for (uint32_t k = 0; k < TS_ITEMS; k++) {
    const uint64_t i = base + k;
    if (i < S.n) {
      const bool drop = i + 1 < S.n && S.k[i + 1] == S.k[i] && S.t[i + 1] < floor;
      mask |= drop ? 0u : 1u << k;
    }
  }
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
      dk[pos] = S.k[base + k];
      dt[pos] = S.t[base + k];
      pos++;
    }
}

}  // namespace

// The store's other buffer with room for `need` versions (its content is not
// kept: a merge or a trim writes all of it).
int dcc_ctx::mvcc_store_room(uint64_t need) {
  const int o = mv_cur ^ 1;
  if (need * 8 <= mv_sk[o].cap && need * 8 <= mv_st[o].cap) return DCC_OK;
  const uint64_t want = std::max<uint64_t>(need + need / 2, 4096);  // amortised growth
  CR(mv_sk[o].ensure(this, want * 8, "mvcc version keys"));
  CR(mv_st[o].ensure(this, want * 8, "mvcc version timestamps"));
  return DCC_OK;
}

int dcc_ctx::mvcc_reserve(uint64_t n, uint64_t nnz, bool with_conflict, bool with_vts) {
  const uint64_t mm = std::max<uint64_t>(nnz, 1);
  const uint64_t mt = (mm + TS_TILE - 1) / TS_TILE * TS_TILE;
  CR(tso_reserve(n, nnz, with_conflict));  // the decisions run in the TIMESTAMP epoch's workspaces
  CR(mv_ek.ensure(this, mt * 8, "mvcc epoch version keys"));
  CR(mv_et.ensure(this, mt * 8, "mvcc epoch version timestamps"));
  CR(mv_ex.ensure(this, mt * 4, "mvcc epoch version txns"));
  CR(mv_late.ensure(this, mt * 4, "mvcc late accesses"));
  CR(mv_lslot.ensure(this, mt * 4, "mvcc row slots"));
  CR(mv_toff.ensure(this, (mt / TS_TILE + 1) * 8, "mvcc tile offsets"));
  if (with_vts) CR(mv_vts.ensure(this, mm * 8, "mvcc versions out"));
  return DCC_OK;
}

int dcc_ctx::mvcc_epoch(const dcc_batch* b, const uint64_t* ts_in, uint8_t* out_rc, uint32_t* out_conflict,
                        uint64_t* out_vts, dcc_stats* st) {
  dcc_ctx* ctx = this;
  EpochStats es;
  dcc_stats& S = es.S;
  if (!out_rc) return fail(DCC_EINVAL, "mvcc: null out_rc");
  if (!ts_in) return fail(DCC_EINVAL, "mvcc: null ts");
  CR(check_batch(b, false));  // the offsets are checked on the device (k_batch_check)
  if (comm_ranks() > 1) return fail(DCC_ENOTSUP, "mvcc: single-GPU engine");
  const bool dev = (b->flags & DCC_DEVICE_PTRS) != 0;
  if (b->n_txn == 0) {
    if (st) *st = S;
    return DCC_OK;
  }
  DevBatch d;
  CR(stage_batch(b, d));
  const uint64_t n = d.n, m = d.nnz;
  CR(mvcc_reserve(n, m, out_conflict != nullptr && !dev, out_vts != nullptr && !dev));
  const uint64_t* ts_dev;
  CR(stage(ts_stage, ts_in, n * 8, dev, "mvcc timestamps", ts_dev));
  uint8_t* rc_dev = dev ? out_rc : (uint8_t*)rc.p;
  uint32_t* conf_dev = out_conflict ? (dev ? out_conflict : (uint32_t*)ts_conf.p) : nullptr;
  uint64_t* vts_dev = out_vts ? (dev ? out_vts : (uint64_t*)mv_vts.p) : nullptr;
  const bool prof = profiling;

  TsRun R;
  CR(ts_build<Mv>(
      this, mv_rows, d, ts_dev, R,
      [&](uint32_t* cnt) {
        k_mv_tscheck<<<launch_grid(n, TS_T * 4, (unsigned)n_cu * 16), TS_T, 0, stream>>>(ts_dev, n, cnt);
        CK(hipGetLastError());
        return (int)DCC_OK;
      },
      // the store's other buffer takes the merge: room for every WR access
      // before anything of the epoch is kept
      [&] { return R.nnz_w ? mvcc_store_room(mv_n + R.nnz_w) : (int)DCC_OK; }));
  uint32_t* cnt = R.cnt;
  uint64_t* nc_dev = (uint64_t*)&cnt[MV_C_NC];
  const auto scan = [&](const ScanArgs& sa) {
    MvScanArgs a;
    (ScanArgs&)a = sa;
    a.vts = vts_dev;
    a.late = (uint32_t*)mv_late.p;
    a.nlate = &cnt[MV_C_NLATE];
    a.lslot = (uint32_t*)mv_lslot.p;
    a.rowv = sa.bnd;  // the bounds are done with when the rounds are
    return a;
  };
  CR(ts_rounds<Mv>(this, R, scan));
  const TsArgs& A = R.A;
  const uint64_t tiles = R.tiles;
  const unsigned max_grid = R.max_grid;
  const MvStore old{(const uint64_t*)mv_sk[mv_cur].p, (const uint64_t*)mv_st[mv_cur].p, mv_n};
  if (m) {
    // every txn decided: versions by the fast path, the late list, the rows' new values
    const MvScanArgs SA = scan(R.SA);
    k_ts_scan<false, true, Mv><<<(unsigned)tiles, TS_T, 0, stream>>>(SA);
    k_tile_aggscan<TqOp><<<1, SEG_AGG_T, 0, stream>>>(SA.agg, SA.pre, tiles, nullptr, nullptr);
    k_ts_scan<true, true, Mv><<<(unsigned)tiles, TS_T, 0, stream>>>(SA);
    // the epoch's versions in (row, index) order
    uint64_t* toff = (uint64_t*)mv_toff.p;
    uint64_t* ek = (uint64_t*)mv_ek.p;
    uint64_t* et = (uint64_t*)mv_et.p;
    uint32_t* ex = (uint32_t*)mv_ex.p;
    k_mv_commits<false><<<(unsigned)tiles, TS_T, 0, stream>>>(m, SA.s_info, SA.s_txn, SA.s_ts, SA.sv, SA.stp,
                                                              d.keys, toff, ek, et, ex);
    k_mv_offsets<<<1, MVS_OFF_T, 0, stream>>>(toff, tiles, nc_dev);
    k_mv_commits<true><<<(unsigned)tiles, TS_T, 0, stream>>>(m, SA.s_info, SA.s_txn, SA.s_ts, SA.sv, SA.stp,
                                                             d.keys, toff, ek, et, ex);
    if (vts_dev)
      k_mv_lookup<<<launch_grid(m, TS_T, max_grid), TS_T, 0, stream>>>(SA.late, SA.nlate, d.keys, A.arec, ek, et, ex,
                                                                       nc_dev, old, vts_dev);
    if (R.nnz_w)  // an epoch without a WR access installs nothing: the store stays where it is
      k_mv_merge<<<launch_grid(mv_n + R.nnz_w, TS_T, max_grid), TS_T, 0, stream>>>(
          old, ek, et, nc_dev, (uint64_t*)mv_sk[mv_cur ^ 1].p, (uint64_t*)mv_st[mv_cur ^ 1].p);
    k_mv_rows<<<launch_grid(m, TS_T, max_grid), TS_T, 0, stream>>>(m, SA.s_info, SA.lslot, SA.rowv, SA.tab,
                                                                   &cnt[SEG_C_ERR]);
  }
  k_ts_rc<<<launch_grid(n, TS_T, max_grid), TS_T, 0, stream>>>(n, A.stp, rc_dev, conf_dev, cnt);
  CK(hipGetLastError());
  if (prof) CK(hipEventRecord(pev[4], stream));
  CK(hipEventRecord(ev1, stream));
  if (!dev) {
    CK(hipMemcpyAsync(out_rc, rc_dev, n, hipMemcpyDeviceToHost, stream));
    if (out_conflict) CK(hipMemcpyAsync(out_conflict, conf_dev, n * 4, hipMemcpyDeviceToHost, stream));
    if (out_vts && m) CK(hipMemcpyAsync(out_vts, vts_dev, m * 8, hipMemcpyDeviceToHost, stream));
  }
  CK(hipMemcpyAsync(hmisc, cnt, TS_C_RING * 4, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  const uint32_t* hc = (const uint32_t*)hmisc;
  mv_rows.rows += hc[TS_C_ROWS];  // rows entered stay in the table whatever follows
  if (hc[SEG_C_ERR] & TS_ERR_FULL) return fail(DCC_EIO, "mvcc: row table full");
  if (hc[SEG_C_ERR] & TS_ERR_STATE) return fail(DCC_EIO, "mvcc: inconsistent decisions");
  uint64_t nc;
  memcpy(&nc, hc + MV_C_NC, 8);
  if (nc) {  // the merged store is the store (an epoch without a commit leaves it where it is)
    mv_cur ^= 1;
    mv_n += nc;
  }
  S.rounds = R.rounds;
  S.n_commit = hc[TS_C_COMMIT];
  S.n_abort = n - hc[TS_C_COMMIT];
  S.nnz_w = hc[TS_C_NWR];
  S.n_readonly = hc[TS_C_RO];
  S.n_survivors = hc[MV_C_NLATE];
  S.alg_bytes = dcc_mvcc_alg_bytes(n, m, out_conflict != nullptr, out_vts != nullptr);
  CR(es.finish(this, 4));
  if (st) *st = S;
  return DCC_OK;
}

int dcc_ctx::mvcc_trim(uint64_t floor, uint64_t* n_dropped) {
  dcc_ctx* ctx = this;
  if (n_dropped) *n_dropped = 0;
  if (mv_n == 0) return DCC_OK;
  const uint64_t tiles = (mv_n + TS_TILE - 1) / TS_TILE;
  CR(mv_toff.ensure(this, (tiles + 1) * 8, "mvcc tile offsets"));
  CR(mvcc_store_room(mv_n));
  uint64_t* toff = (uint64_t*)mv_toff.p;
  const MvStore old{(const uint64_t*)mv_sk[mv_cur].p, (const uint64_t*)mv_st[mv_cur].p, mv_n};
  uint64_t* dk = (uint64_t*)mv_sk[mv_cur ^ 1].p;
  uint64_t* dt = (uint64_t*)mv_st[mv_cur ^ 1].p;
  k_mv_trim<false><<<(unsigned)tiles, TS_T, 0, stream>>>(old, floor, toff, dk, dt);
  k_mv_offsets<<<1, MVS_OFF_T, 0, stream>>>(toff, tiles, toff + tiles);
  k_mv_trim<true><<<(unsigned)tiles, TS_T, 0, stream>>>(old, floor, toff, dk, dt);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(hmisc, toff + tiles, 8, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  uint64_t kept;
  memcpy(&kept, hmisc, 8);
  if (kept > mv_n) return fail(DCC_EIO, "mvcc: trim kept more versions than the store holds");
  if (n_dropped) *n_dropped = mv_n - kept;
  if (kept != mv_n) {
    mv_cur ^= 1;
    mv_n = kept;
  }
  return DCC_OK;
}

int dcc_ctx::mvcc_export(uint64_t* keys, uint64_t* ts, uint64_t cap, uint64_t* n_out) {
  dcc_ctx* ctx = this;
  if (n_out) *n_out = mv_n;
  if (cap < mv_n) return fail(DCC_ERANGE, "mvcc: %llu versions, room for %llu", (unsigned long long)mv_n,
                              (unsigned long long)cap);
  if (mv_n == 0) return DCC_OK;
  if (keys) CK(hipMemcpyAsync(keys, mv_sk[mv_cur].p, mv_n * 8, hipMemcpyDeviceToHost, stream));
  if (ts) CK(hipMemcpyAsync(ts, mv_st[mv_cur].p, mv_n * 8, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  return DCC_OK;
}

extern "C" uint64_t dcc_mvcc_alg_bytes(uint64_t n_txn, uint64_t nnz, int with_conflict, int with_vts) {
  // the TIMESTAMP epoch's (one 24-B row {key, latest version, rts} per
  // access) and the version of every access; the store's share depends on its
  // size and is not in it
  return dcc_tso_alg_bytes(n_txn, nnz, with_conflict) + (with_vts ? 8 * nnz : 0);
}

extern "C" int dcc_mvcc_validate_epoch(dcc_ctx* ctx, const dcc_batch* batch, const uint64_t* ts, uint8_t* out_rc,
                                       uint32_t* out_conflict, uint64_t* out_vts, dcc_stats* out_stats) {
  if (!ctx || !batch || !out_rc || !ts) return DCC_EINVAL;
  dcc_pipe_drain(ctx);  // pipelined OCC epochs in flight complete first
  // a multi-GPU context: the whole epoch on rank 0 (rows and versions are one GPU's), no collective
  return dcc_on_device(ctx, true, [&](dcc_ctx* s) {
    return s->mvcc_epoch(batch, ts, out_rc, out_conflict, out_vts, out_stats);
  });
}

extern "C" int dcc_mvcc_rows_get(dcc_ctx* ctx, const uint64_t* keys, uint64_t* wts, uint64_t* rts, uint64_t n) {
  if (!ctx || (n && (!keys || !wts || !rts))) return DCC_EINVAL;
  return dcc_on_device(ctx, false, [&](dcc_ctx* s) { return s->mv_rows.get<TsProbe>(s, keys, wts, rts, n); });
}

extern "C" uint64_t dcc_mvcc_rows_size(const dcc_ctx* ctx) {
  if (ctx && ctx->multi) ctx = dcc_multi_sub((dcc_ctx*)ctx, 0);
  return ctx ? ctx->mv_rows.size() : 0;
}

extern "C" uint64_t dcc_mvcc_versions_size(const dcc_ctx* ctx) {
  if (ctx && ctx->multi) ctx = dcc_multi_sub((dcc_ctx*)ctx, 0);
  return ctx ? ctx->mv_n : 0;
}

extern "C" int dcc_mvcc_versions_export(dcc_ctx* ctx, uint64_t* keys, uint64_t* ts, uint64_t cap,
                                        uint64_t* n_out) {
  if (!ctx) return DCC_EINVAL;
  return dcc_on_device(ctx, false, [&](dcc_ctx* s) { return s->mvcc_export(keys, ts, cap, n_out); });
}

extern "C" int dcc_mvcc_trim(dcc_ctx* ctx, uint64_t ts_floor, uint64_t* n_dropped) {
  if (!ctx) return DCC_EINVAL;
  return dcc_on_device(ctx, false, [&](dcc_ctx* s) { return s->mvcc_trim(ts_floor, n_dropped); });
}

extern "C" int dcc_mvcc_clear(dcc_ctx* ctx) {
  if (!ctx) return DCC_EINVAL;
  return dcc_on_device(ctx, false, [](dcc_ctx* s) {
    s->mv_n = 0;  // the buffers stay
    return s->mv_rows.clear(s);
  });
}
