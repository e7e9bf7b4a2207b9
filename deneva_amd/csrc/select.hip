// Select the txns of an epoch by decision into a CSR (dcc_batch_select): the
// carry between two epochs of a device-resident batch.  The aborted txns of
// epoch e are the front of epoch e + 1 (the reference's abort queue,
// system/abort_queue.cpp, retried at once; its back-off is the device queue
// of abortq.hip), the committed ones are the held prefix of the next NO_WAIT /
// Calvin call.
//
// A stream compaction over a ragged CSR.  Txn i is selected iff rc[i] == want;
// selected txns keep their index order and their accesses their list order.
// The tile bodies are csr_select.h's (shared with the abort queue), here with
// the decision byte as the predicate and the identity as the source mapping.
//
// Kernels:  k_sel_count    one pair per tile of SEL_T consecutive txns; the
//                          offsets are checked here, before anything indexes
//                          with them
//           k_sel_scan     one workgroup: exclusive scan of the tile pairs,
//                          the totals, the verdict (offsets / capacities)
//           k_sel_scatter  per tile: the scan again in LDS, the per-txn rows,
//                          then the tile's output range [0, tile accesses)
//                          walked by all lanes: lane p finds its txn by binary
//                          search over the tile's LDS scan values
// No workgroup waits on another: the tile bases come from the launch before.
// The scatter reads the verdict first and writes nothing unless it is clear,
// so the host reads the totals once, after the last launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>

#include "csr_select.h"
#include "dcc.h"
#include "dcc_ctx.h"
#include "dcc_device.h"
#include "dcc_scan.h"

using namespace dcc;

namespace {

// control words (sel_misc): u64 [0] verdict, [1] selected txns | accesses << 32
constexpr uint32_t SEL_C_ERR = 0, SEL_C_TOTAL = 1, SEL_C_WORDS = 2;

// Txn t is selected iff rc[t] == want; the per-txn arrays carried with it.
struct RcSel {
  const uint8_t* rc;
  const uint32_t* src_in;
  const uint64_t *start_tn, *finish_tn, *order;  // inputs of the arrays carried (else null)
  uint8_t want;
  uint64_t *o_start, *o_finish, *o_order;
  uint32_t* o_src;
  __device__ void begin() {}
  __device__ uint64_t src(uint64_t t) const { return t; }
  __device__ bool take(uint64_t t, uint64_t) const { return rc[t] == want; }
  __device__ void row(uint64_t q, uint64_t t, uint64_t) const {
    if (o_src) o_src[q] = src_in ? src_in[t] : (uint32_t)t;
    if (o_start) o_start[q] = start_tn[t];
    if (o_finish) o_finish[q] = finish_tn[t];
    if (o_order) o_order[q] = order[t];
  }
};

__global__ __launch_bounds__(SEL_T) void k_sel_count(const uint32_t* __restrict__ off, uint64_t n, uint64_t nnz,
                                                     const uint8_t* __restrict__ rc, uint8_t want,
                                                     uint64_t n_tiles, uint64_t* __restrict__ part,
                                                     uint64_t* __restrict__ ctl) {
  RcSel S{};
  S.rc = rc;
  S.want = want;
  csr_count_tiles<true>(off, n, nnz, S, n_tiles, part, &ctl[SEL_C_ERR]);
}

__global__ __launch_bounds__(SEL_T) void k_sel_scan(uint64_t* __restrict__ part, uint64_t n_tiles,
                                                    uint64_t cap_txn, uint64_t cap_nnz, uint64_t nnz_base,
                                                    uint64_t* __restrict__ ctl) {
  csr_scan_tiles(part, n_tiles, cap_txn, cap_nnz, nnz_base, &ctl[SEL_C_ERR], &ctl[SEL_C_TOTAL]);
}

struct SelArgs {
  CsrMove M;
  RcSel S;
};

__global__ __launch_bounds__(SEL_T) void k_sel_scatter(SelArgs A) { csr_scatter_tiles(A.M, A.S); }

uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

}  // namespace

int dcc_ctx::select_reserve(uint64_t n, uint64_t nnz) {
  CR(sel_misc.ensure(this, SEL_C_WORDS * 8, "select control words"));
  CR(sel_part.ensure(this, ((n + SEL_T - 1) / SEL_T + 1) * 8, "select tile pairs"));
  // a host call: rc and src_in in, every output array out
  CR(sel_rc.ensure(this, n, "select rc"));
  CR(sel_src.ensure(this, n * 4, "select src"));
  CR(sel_out.ensure(this, nnz * 8 + 3 * n * 8 + up16((n + 1) * 4) + n * 4 + nnz + 64, "select outputs"));
  return DCC_OK;
}

int dcc_ctx::select_batch(const dcc_batch* b, const uint8_t* rc_in, uint8_t want, const uint32_t* src_in,
                          const dcc_select_out* out, uint64_t* out_n, uint64_t* out_nnz, dcc_stats* st) {
  dcc_ctx* ctx = this;
  EpochStats es;
  dcc_stats& S = es.S;
  if (out_n) *out_n = 0;
  if (out_nnz) *out_nnz = 0;
  if (!out || !out->offsets) return fail(DCC_EINVAL, "select: null out / out offsets");
  if (out->cap_nnz && (!out->keys || !out->acctype)) return fail(DCC_EINVAL, "select: null out keys/acctype");
  CR(check_batch(b, false));  // txn length is free here; the offsets are checked on the device
  const uint64_t n = b->n_txn;
  if (n && !rc_in) return fail(DCC_EINVAL, "select: null rc");
  if (out->nnz_base > 0xFFFFFFFFull) return fail(DCC_ERANGE, "select: nnz_base exceeds 2^32-1");
  const bool dev = (b->flags & DCC_DEVICE_PTRS) != 0;
  if (n == 0) {
    const uint32_t v = (uint32_t)out->nnz_base;
    if (dev) {
      *(uint32_t*)hmisc = v;
      CK(hipMemcpyAsync(out->offsets + out->txn_base, hmisc, 4, hipMemcpyHostToDevice, stream));
      CK(hipStreamSynchronize(stream));
    } else {
      out->offsets[out->txn_base] = v;
    }
    S.alg_bytes = dcc_select_alg_bytes(0, 0, 0, 0);
    es.wall();
    if (st) *st = S;
    return DCC_OK;
  }
  DevBatch d;
  CR(stage_batch(b, d));  // compact forms are widened here: the gather reads the wide form
  const uint64_t m = d.nnz;
  const uint64_t n_tiles = (n + SEL_T - 1) / SEL_T;
  CR(sel_misc.ensure(this, SEL_C_WORDS * 8, "select control words"));
  CR(sel_part.ensure(this, (n_tiles + 1) * 8, "select tile pairs"));
  uint64_t* ctl = (uint64_t*)sel_misc.p;
  uint64_t* part = (uint64_t*)sel_part.p;

  const bool w_start = d.start_tn && out->start_tn, w_finish = d.finish_tn && out->finish_tn,
             w_order = d.order && out->order, w_src = out->src != nullptr;
  // the most the call can write: the capacities, and no more than the batch holds
  const uint64_t room_n = std::min(out->cap_txn, n), room_m = std::min(out->cap_nnz, m);
  SelArgs A{};
  A.M.n = n;
  A.M.n_tiles = n_tiles;
  A.M.off = d.off;
  A.M.keys = d.keys;
  A.M.at = d.acctype;
  A.S.want = want;
  A.M.nnz_base = out->nnz_base;
  A.M.part = part;
  A.M.err = &ctl[SEL_C_ERR];
  if (w_start) A.S.start_tn = d.start_tn;
  if (w_finish) A.S.finish_tn = d.finish_tn;
  if (w_order) A.S.order = d.order;
  uint64_t *h_keys = nullptr, *h_tn[3] = {};
  uint32_t *h_off = nullptr, *h_src = nullptr;
  uint8_t* h_at = nullptr;
  CR(stage(sel_rc, rc_in, n, dev, "select rc", A.S.rc));
  if (src_in) CR(stage(sel_src, src_in, n * 4, dev, "select src", A.S.src_in));
  if (dev) {
    A.M.o_off = out->offsets + out->txn_base;
    A.M.o_keys = out->keys ? out->keys + out->nnz_base : nullptr;
    A.M.o_at = out->acctype ? out->acctype + out->nnz_base : nullptr;
    A.S.o_start = w_start ? out->start_tn + out->txn_base : nullptr;
    A.S.o_finish = w_finish ? out->finish_tn + out->txn_base : nullptr;
    A.S.o_order = w_order ? out->order + out->txn_base : nullptr;
    A.S.o_src = w_src ? out->src + out->txn_base : nullptr;
  } else {
    CR(sel_out.ensure(this, room_m * 8 + 3 * room_n * 8 + up16((room_n + 1) * 4) + room_n * 4 + room_m + 64,
                      "select outputs"));
    uint8_t* o = (uint8_t*)sel_out.p;
    h_keys = (uint64_t*)o;
    o += room_m * 8;
    for (int q = 0; q < 3; q++, o += room_n * 8) h_tn[q] = (uint64_t*)o;
    h_off = (uint32_t*)o;
    o += up16((room_n + 1) * 4);
    h_src = (uint32_t*)o;
    o += up16(room_n * 4);
    h_at = o;
    A.M.o_off = h_off;
    A.M.o_keys = h_keys;
    A.M.o_at = h_at;
    A.S.o_start = w_start ? h_tn[0] : nullptr;
    A.S.o_finish = w_finish ? h_tn[1] : nullptr;
    A.S.o_order = w_order ? h_tn[2] : nullptr;
    A.S.o_src = w_src ? h_src : nullptr;
  }

  const unsigned grid = sel_grid(n_tiles, (unsigned)n_cu * 16);
  const bool prof = profiling;
  CK(hipMemsetAsync(ctl, 0, SEL_C_WORDS * 8, stream));
  CK(hipEventRecord(ev0, stream));
  if (prof) CK(hipEventRecord(pev[0], stream));
  k_sel_count<<<grid, SEL_T, 0, stream>>>(d.off, n, m, A.S.rc, want, n_tiles, part, ctl);
  if (prof) CK(hipEventRecord(pev[1], stream));
  k_sel_scan<<<1, SEL_T, 0, stream>>>(part, n_tiles, out->cap_txn, out->cap_nnz, out->nnz_base, ctl);
  if (prof) CK(hipEventRecord(pev[2], stream));
  k_sel_scatter<<<grid, SEL_T, 0, stream>>>(A);
  CK(hipGetLastError());
  if (prof) CK(hipEventRecord(pev[3], stream));
  CK(hipEventRecord(ev1, stream));
  CK(hipMemcpyAsync(hmisc, ctl, SEL_C_WORDS * 8, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  const uint64_t* hc = (const uint64_t*)hmisc;
  const uint64_t verdict = hc[SEL_C_ERR];
  if (verdict & SEL_ERR_OFF) return fail(DCC_EINVAL, "batch: malformed offsets");
  const uint64_t ns = hc[SEL_C_TOTAL] & 0xFFFFFFFFull, ms = hc[SEL_C_TOTAL] >> 32;
  if (out_n) *out_n = ns;
  if (out_nnz) *out_nnz = ms;
  S.n_commit = ns;
  S.n_abort = n - ns;
  if (verdict & SEL_ERR_CAP) {
    if (st) *st = S;
    return fail(DCC_ERANGE, "select: %llu txns / %llu accesses selected, room for %llu / %llu behind nnz_base %llu",
                (unsigned long long)ns, (unsigned long long)ms, (unsigned long long)out->cap_txn,
                (unsigned long long)out->cap_nnz, (unsigned long long)out->nnz_base);
  }
  if (!dev) {
    const uint64_t tb = out->txn_base, xb = out->nnz_base;
    CK(hipMemcpyAsync(out->offsets + tb, h_off, (ns + 1) * 4, hipMemcpyDeviceToHost, stream));
    if (ms) {
      CK(hipMemcpyAsync(out->keys + xb, h_keys, ms * 8, hipMemcpyDeviceToHost, stream));
      CK(hipMemcpyAsync(out->acctype + xb, h_at, ms, hipMemcpyDeviceToHost, stream));
    }
    if (ns) {
      if (w_start) CK(hipMemcpyAsync(out->start_tn + tb, h_tn[0], ns * 8, hipMemcpyDeviceToHost, stream));
      if (w_finish) CK(hipMemcpyAsync(out->finish_tn + tb, h_tn[1], ns * 8, hipMemcpyDeviceToHost, stream));
      if (w_order) CK(hipMemcpyAsync(out->order + tb, h_tn[2], ns * 8, hipMemcpyDeviceToHost, stream));
      if (w_src) CK(hipMemcpyAsync(out->src + tb, h_src, ns * 4, hipMemcpyDeviceToHost, stream));
    }
    CK(hipStreamSynchronize(stream));
  }
  S.alg_bytes = dcc_select_alg_bytes(n, ns, ms, (int)w_start + (int)w_finish + (int)w_order + (int)w_src);
  CR(es.finish(this, 3));
  if (st) *st = S;
  return DCC_OK;
}

extern "C" uint64_t dcc_select_alg_bytes(uint64_t n_txn, uint64_t n_sel, uint64_t nnz_sel, int n_txn_arrays) {
  // offsets and RC read once, (key, type) of every selected access read and
  // written, the selection's offsets written, 16 B per selected txn and
  // per-txn array carried
  return 4 * (n_txn + 1) + n_txn + 18 * nnz_sel + 4 * (n_sel + 1) +
         16 * n_sel * (uint64_t)std::max(n_txn_arrays, 0);
}

extern "C" int dcc_batch_select(dcc_ctx* ctx, const dcc_batch* batch, const uint8_t* rc, uint8_t want,
                                const uint32_t* src_in, const dcc_select_out* out, uint64_t* out_n,
                                uint64_t* out_nnz, dcc_stats* out_stats) {
  if (!ctx || !batch) return DCC_EINVAL;
  dcc_pipe_drain(ctx);  // pipelined OCC epochs in flight complete first
  if (ctx->multi)  // a local data movement: rank 0's GPU, its communicator left alone
    return dcc_multi_on_rank0(ctx, false, [&](dcc_ctx* s) {
      return s->select_batch(batch, rc, want, src_in, out, out_n, out_nnz, out_stats);
    });
  if (hipSetDevice(ctx->device) != hipSuccess) return DCC_ENODEV;
  return ctx->select_batch(batch, rc, want, src_in, out, out_n, out_nnz, out_stats);
}
