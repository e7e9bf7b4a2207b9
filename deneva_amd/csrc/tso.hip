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
// Kernels (tso_kernels.h, shared with the MVCC engine of mvcc.hip; the batch
// check, k_tile_aggscan and the rounds loop are seg_rounds.h's):
//           k_ts_prep     packed sort keys, the record of every access, WR / read-only counts
//           k_ts_seg      sorted records (txn, position | type | head | last, ts), heads
//           k_ts_seed     a row-table slot per segment head (find or insert)
//           k_ts_scan     per 1,024-access tile: its aggregate (reduce) or,
//                         behind the scanned aggregates, the bounds of every
//                         access (apply); the final apply writes the rows
//           k_ts_advance  one round of decisions from the bounds
//           k_ts_rc       RC bytes, conflict ordinals, the commit count
// No workgroup waits on another: a round is reduce / scan of aggregates /
// apply / advance, four launches.
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

#include "tso_kernels.h"

namespace {

// tso_kernels.h's engine: a read meets the committed-writer bound, the final
// apply stores the rows.
struct Tso {
  static constexpr bool MVCC = false;
  static constexpr const char* name = "tso";
  using Scan = ScanArgs;
  struct Out {};
};

}  // namespace

int dcc_ctx::tso_reserve(uint64_t n, uint64_t nnz, bool with_conflict) {
  const uint64_t nn = std::max<uint64_t>(n, 1), mm = std::max<uint64_t>(nnz, 1);
  const uint64_t mt = (mm + TS_TILE - 1) / TS_TILE * TS_TILE;  // whole tiles: 16-B loads
  CR(seg.reserve(this, n, nnz));
  CR(ts_hslot.ensure(this, mt * 4, "tso head slots"));
  CR(ts_bnd.ensure(this, mm * 16, "tso bounds"));
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
  CR(check_batch(b, false));  // the offsets are checked on the device (k_batch_check)
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
  uint8_t* rc_dev = dev ? out_rc : (uint8_t*)rc.p;
  uint32_t* conf_dev = out_conflict ? (dev ? out_conflict : (uint32_t*)ts_conf.p) : nullptr;
  const bool prof = profiling;

  TsRun R;
  CR(ts_build<Tso>(this, ts_rows, d, ts_dev, R, [](uint32_t*) { return DCC_OK; }, [] { return DCC_OK; }));
  CR(ts_rounds<Tso>(this, R, [](const ScanArgs& sa) { return sa; }));
  uint32_t* cnt = R.cnt;
  const TsArgs& A = R.A;
  const ScanArgs& SA = R.SA;
  const uint64_t tiles = R.tiles;
  const unsigned max_grid = R.max_grid;
  if (m) {  // every txn decided: the rows' new state from each segment's last element
    k_ts_scan<false, true, Tso><<<(unsigned)tiles, TS_T, 0, stream>>>(SA);
    k_tile_aggscan<TqOp><<<1, SEG_AGG_T, 0, stream>>>(SA.agg, SA.pre, tiles, nullptr, nullptr);
    k_ts_scan<true, true, Tso><<<(unsigned)tiles, TS_T, 0, stream>>>(SA);
  }
  k_ts_rc<<<launch_grid(n, TS_T, max_grid), TS_T, 0, stream>>>(n, A.stp, rc_dev, conf_dev, cnt);
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
  if (hc[SEG_C_ERR] & TS_ERR_FULL) return fail(DCC_EIO, "tso: row table full");
  if (hc[SEG_C_ERR] & TS_ERR_STATE) return fail(DCC_EIO, "tso: inconsistent decisions");
  S.rounds = R.rounds;
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
