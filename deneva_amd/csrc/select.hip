// Select the txns of an epoch by decision into a CSR (dcc_batch_select): the
// carry between two epochs of a device-resident batch.  The aborted txns of
// epoch e are the front of epoch e + 1 (the reference's abort queue,
// system/abort_queue.cpp, without its back-off), the committed ones are the
// held prefix of the next NO_WAIT / Calvin call.
//
// A stream compaction over a ragged CSR.  Txn i is selected iff rc[i] == want;
// selected txns keep their index order and their accesses their list order.
// The pair (selected ? 1 : 0, selected ? len : 0) travels as the two halves of
// one u64 (dcc_scan.h), so one scan places the txn rows and the accesses.
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

#include "dcc.h"
#include "dcc_ctx.h"
#include "dcc_device.h"
#include "dcc_scan.h"

using namespace dcc;

namespace {

constexpr uint32_t SEL_T = 256;  // threads per workgroup = txns per tile
constexpr uint32_t SEL_NW = SEL_T / 64;
constexpr uint32_t SEL_KU = 4;  // keys per lane and step of the gather
constexpr uint32_t SEL_ERR_OFF = 1, SEL_ERR_CAP = 2;
// control words (sel_misc): u64 [0] verdict, [1] selected txns | accesses << 32
constexpr uint32_t SEL_C_ERR = 0, SEL_C_TOTAL = 1, SEL_C_WORDS = 2;

using PairOp = AddOp<uint64_t>;  // low word: txns, high word: accesses

__device__ inline uint64_t sel_pair(bool sel, uint32_t len) { return sel ? (1ull | ((uint64_t)len << 32)) : 0ull; }

__global__ __launch_bounds__(SEL_T) void k_sel_count(const uint32_t* __restrict__ off, uint64_t n, uint64_t nnz,
                                                     const uint8_t* __restrict__ rc, uint8_t want,
                                                     uint64_t n_tiles, uint64_t* __restrict__ part,
                                                     uint64_t* __restrict__ ctl) {
  __shared__ uint64_t s_w[SEL_NW];
  uint32_t err = 0;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t t = tile * SEL_T + threadIdx.x;
    uint64_t v = 0;
    if (t < n) {
      const uint32_t a0 = off[t], b0 = off[t + 1];
      if (b0 < a0) err = SEL_ERR_OFF;
      if (t == 0 && a0 != 0) err = SEL_ERR_OFF;
      if (t == n - 1 && b0 != nnz) err = SEL_ERR_OFF;
      v = sel_pair(rc[t] == want, b0 - a0);
    }
    const uint64_t tot = block_reduce_reuse<PairOp>(v, s_w, SEL_NW);
    if (threadIdx.x == 0) part[tile] = tot;
  }
  if (err) atomicOr((unsigned long long*)&ctl[SEL_C_ERR], (unsigned long long)err);
}

// part[tile] becomes the exclusive prefix of the tile pairs.  With well-formed
// offsets the accesses sum to <= nnz < 2^32, so the halves never carry into
// each other; with malformed ones the verdict keeps every later reader out.
__global__ __launch_bounds__(SEL_T) void k_sel_scan(uint64_t* __restrict__ part, uint64_t n_tiles,
                                                    uint64_t cap_txn, uint64_t cap_nnz, uint64_t nnz_base,
                                                    uint64_t* __restrict__ ctl) {
  __shared__ uint64_t s_w[SEL_NW];
  // thread t owns the consecutive tiles [t * chunk, (t + 1) * chunk): one
  // block scan whatever the tile count
  const uint64_t chunk = (n_tiles + SEL_T - 1) / SEL_T;
  const uint64_t q0 = min(n_tiles, threadIdx.x * chunk), q1 = min(n_tiles, q0 + chunk);
  uint64_t v = 0;
  for (uint64_t q = q0; q < q1; q++) v += part[q];
  uint64_t carry;
  uint64_t run = block_excl<PairOp>(v, s_w, SEL_NW, carry);
  for (uint64_t q = q0; q < q1; q++) {
    const uint64_t x = part[q];
    part[q] = run;
    run += x;
  }
  if (threadIdx.x == 0) {
    const uint64_t ns = carry & 0xFFFFFFFFull, ms = carry >> 32;
    ctl[SEL_C_TOTAL] = carry;
    if (ns > cap_txn || ms > cap_nnz || nnz_base + ms > 0xFFFFFFFFull) ctl[SEL_C_ERR] |= SEL_ERR_CAP;
  }
}

struct SelArgs {
  uint64_t n, n_tiles;
  const uint32_t* off;
  const uint64_t* keys;
  const uint8_t* at;
  const uint8_t* rc;
  const uint32_t* src_in;
  const uint64_t *start_tn, *finish_tn, *order;  // inputs of the arrays carried (else null)
  uint8_t want;
  uint64_t nnz_base;  // value of o_off[0]
  // outputs, already at the bases: row q of the selection is o_*[q]
  uint32_t* o_off;  // [n_sel + 1]
  uint64_t* o_keys;
  uint8_t* o_at;
  uint64_t *o_start, *o_finish, *o_order;
  uint32_t* o_src;
  const uint64_t* part;
  const uint64_t* ctl;
};

// The txn of tile-local output position p: the last t with s_start[t] <= p.
// Unselected and empty txns repeat their successor's start, so that t is the
// one whose accesses cover p.  cnt >= 1 txns, s_start[cnt] = the tile total.
__device__ inline uint32_t sel_find(const uint32_t* s_start, uint32_t cnt, uint32_t p) {
  uint32_t lo = 0, hi = cnt;  // s_start[lo] <= p < s_start[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (s_start[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(SEL_T) void k_sel_scatter(SelArgs A) {
  __shared__ uint64_t s_w[SEL_NW];
  __shared__ uint32_t s_start[SEL_T + 1];  // first output position of the txn within the tile
  __shared__ uint32_t s_src[SEL_T];        // its first access in the batch
  if (A.ctl[SEL_C_ERR]) return;  // malformed offsets or no room: nothing is written
  if (blockIdx.x == 0 && threadIdx.x == 0) A.o_off[0] = (uint32_t)A.nnz_base;
  for (uint64_t tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
    const uint64_t t = tile * SEL_T + threadIdx.x;
    const uint64_t left = A.n - tile * SEL_T;
    const uint32_t cnt = left < SEL_T ? (uint32_t)left : SEL_T;
    uint32_t a0 = 0, len = 0;
    bool sel = false;
    if (t < A.n) {
      a0 = A.off[t];
      len = A.off[t + 1] - a0;
      sel = A.rc[t] == A.want;
    }
    uint64_t tot;
    const uint64_t ex = block_excl_reuse<PairOp>(sel_pair(sel, len), s_w, SEL_NW, tot);
    const uint64_t base = A.part[tile];
    const uint64_t q0 = base & 0xFFFFFFFFull, x0 = base >> 32;  // the tile's first row / access
    const uint32_t st = (uint32_t)(ex >> 32), m = (uint32_t)(tot >> 32);
    s_start[threadIdx.x] = st;
    s_src[threadIdx.x] = a0;
    if (threadIdx.x == 0) s_start[cnt] = m;
    if (sel) {
      const uint64_t q = q0 + (ex & 0xFFFFFFFFull);
      A.o_off[q + 1] = (uint32_t)(A.nnz_base + x0 + st + len);
      if (A.o_src) A.o_src[q] = A.src_in ? A.src_in[t] : (uint32_t)t;
      if (A.o_start) A.o_start[q] = A.start_tn[t];
      if (A.o_finish) A.o_finish[q] = A.finish_tn[t];
      if (A.o_order) A.o_order[q] = A.order[t];
    }
    __syncthreads();
    // keys: one per lane, the whole tile's output range contiguous
    uint64_t* ok = A.o_keys + x0;
    for (uint32_t p0 = threadIdx.x; p0 < m; p0 += SEL_KU * SEL_T) {
      uint64_t k[SEL_KU];  // SEL_KU independent searches and loads in flight per lane
#pragma unroll
      for (uint32_t j = 0; j < SEL_KU; j++) {
        const uint32_t p = p0 + j * SEL_T;
        if (p < m) {
          const uint32_t tl = sel_find(s_start, cnt, p);
          k[j] = A.keys[(uint64_t)s_src[tl] + (p - s_start[tl])];
        }
      }
#pragma unroll
      for (uint32_t j = 0; j < SEL_KU; j++) {
        const uint32_t p = p0 + j * SEL_T;
        if (p < m) ok[p] = k[j];
      }
    }
    // access types: bytes up to the first 4-byte boundary of the output, then
    // four per lane as one u32 store (one u32 load where the four lie in one
    // txn and its source is aligned too), then the bytes left over
    uint8_t* oa = A.o_at + x0;
    const uint32_t head = min(m, (uint32_t)((4 - ((uintptr_t)oa & 3)) & 3));
    const uint32_t quads = (m - head) >> 2;
    if (threadIdx.x < m - 4 * quads) {  // at most 6 bytes
      const uint32_t p = threadIdx.x < head ? threadIdx.x : threadIdx.x + 4 * quads;
      const uint32_t tl = sel_find(s_start, cnt, p);
      oa[p] = A.at[(uint64_t)s_src[tl] + (p - s_start[tl])];
    }
    for (uint32_t g = threadIdx.x; g < quads; g += SEL_T) {
      const uint32_t p = head + 4 * g;
      uint32_t tl = sel_find(s_start, cnt, p);
      const uint8_t* sp = A.at + (uint64_t)s_src[tl] + (p - s_start[tl]);
      uint32_t w;
      if (p + 3 < s_start[tl + 1] && ((uintptr_t)sp & 3) == 0) {
        w = *(const uint32_t*)sp;
      } else {
        w = sp[0];
#pragma unroll
        for (uint32_t k = 1; k < 4; k++) {
          if (p + k >= s_start[tl + 1]) tl = sel_find(s_start, cnt, p + k);
          w |= (uint32_t)A.at[(uint64_t)s_src[tl] + (p + k - s_start[tl])] << (8 * k);
        }
      }
      *(uint32_t*)(oa + p) = w;
    }
    __syncthreads();  // the LDS arrays are rewritten by the next tile
  }
}

unsigned sel_grid(uint64_t tiles, unsigned max_grid) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(tiles, max_grid));
}

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
  A.n = n;
  A.n_tiles = n_tiles;
  A.off = d.off;
  A.keys = d.keys;
  A.at = d.acctype;
  A.want = want;
  A.nnz_base = out->nnz_base;
  A.part = part;
  A.ctl = ctl;
  if (w_start) A.start_tn = d.start_tn;
  if (w_finish) A.finish_tn = d.finish_tn;
  if (w_order) A.order = d.order;
  uint64_t *h_keys = nullptr, *h_tn[3] = {};
  uint32_t *h_off = nullptr, *h_src = nullptr;
  uint8_t* h_at = nullptr;
  CR(stage(sel_rc, rc_in, n, dev, "select rc", A.rc));
  if (src_in) CR(stage(sel_src, src_in, n * 4, dev, "select src", A.src_in));
  if (dev) {
    A.o_off = out->offsets + out->txn_base;
    A.o_keys = out->keys ? out->keys + out->nnz_base : nullptr;
    A.o_at = out->acctype ? out->acctype + out->nnz_base : nullptr;
    A.o_start = w_start ? out->start_tn + out->txn_base : nullptr;
    A.o_finish = w_finish ? out->finish_tn + out->txn_base : nullptr;
    A.o_order = w_order ? out->order + out->txn_base : nullptr;
    A.o_src = w_src ? out->src + out->txn_base : nullptr;
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
    A.o_off = h_off;
    A.o_keys = h_keys;
    A.o_at = h_at;
    A.o_start = w_start ? h_tn[0] : nullptr;
    A.o_finish = w_finish ? h_tn[1] : nullptr;
    A.o_order = w_order ? h_tn[2] : nullptr;
    A.o_src = w_src ? h_src : nullptr;
  }

  const unsigned grid = sel_grid(n_tiles, (unsigned)n_cu * 16);
  const bool prof = profiling;
  CK(hipMemsetAsync(ctl, 0, SEL_C_WORDS * 8, stream));
  CK(hipEventRecord(ev0, stream));
  if (prof) CK(hipEventRecord(pev[0], stream));
  k_sel_count<<<grid, SEL_T, 0, stream>>>(d.off, n, m, A.rc, want, n_tiles, part, ctl);
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
