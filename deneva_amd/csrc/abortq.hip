// The abort queue with back-off, device-resident (dcc_abortq_*): the
// reference's AbortQueue (system/abort_queue.cpp:26-82) where the batch lives.
// A push parks the txns of an epoch with rc == want, each with its abort
// count and its release time due = now + penalty(cnt); a pop releases the
// entries with due < now in (due, seq) order as the front of the next epoch's
// CSR and keeps the others.
//
// The queue is two CSR pools with per-txn src / cnt / due.  Pool order is seq
// order: pushes append, and the pop's compaction of the kept entries into the
// other pool is stable.  So a stable sort of the due entries by `due` alone is
// (due, seq) order, and seq is never stored.
//
// Every data movement is csr_select.h's compaction (the select's tile bodies)
// with another predicate and source mapping:
//   push    rc[t] == want over the batch, into the tail of the current pool
//   pop 0   due[t] < now over the pool: counts and the verdict only, then
//           k_aq_pairs: one (due - lo, pool index) pair per entry, the due
//           ones in pool order in front, the others behind them with the
//           largest key, so the sort's length is the pool's (known to the
//           host) and not the due count (known to the device only)
//   pop 1   radix_sort_u64 of the pairs (stable), over the bits that can
//           differ among due entries: lo <= due < now
//   pop 2   position t < n_due takes the txn perm[t]: the permuted gather
//           into `out`
//   pop 3   due[t] >= now over the pool, into the other pool
// No workgroup waits on another, the launches go out back to back, every
// writing pass reads the verdict word first, and the host synchronises once
// per call: it swaps the pools and advances n / nnz / seq only after a clear
// verdict, so DCC_ERANGE leaves the queue exactly as it was.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "csr_select.h"
#include "dcc.h"
#include "dcc_ctx.h"
#include "dcc_device.h"
#include "dcc_scan.h"
#include "radix_sort.h"

using namespace dcc;

namespace {

// control words: u64 [0] verdict, [1] push: parked / pop: due, [2] gathered,
// [3] kept -- each txns | accesses << 32
constexpr uint32_t AQ_C_ERR = 0, AQ_C_TOTAL = 1, AQ_C_GATHER = 2, AQ_C_KEEP = 3, AQ_C_WORDS = 4;

// abort_queue.cpp:26-34 with the count after the increment
__host__ __device__ inline uint64_t aq_penalty(uint32_t policy, uint64_t penalty, uint64_t pmax, uint32_t cnt) {
  if (policy == DCC_BACKOFF_NONE) return penalty;
  if (policy == DCC_BACKOFF_REFERENCE) {
    const uint64_t x = (penalty * 2) ^ (uint64_t)cnt;  // line 30 as C parses it
    return x > pmax ? x : pmax;
  }
  if (cnt >= 64) return pmax;
  const uint64_t p = penalty << cnt;
  if ((p >> cnt) != penalty) return pmax;
  return p < pmax ? p : pmax;
}
__host__ __device__ inline uint64_t aq_due(uint64_t now, uint64_t pen) {
  const uint64_t d = now + pen;
  return d < now ? ~0ull : d;
}

struct PushSel {
  const uint8_t* rc;
  const uint32_t *src_in, *cnt_in;
  uint8_t want;
  uint32_t policy;
  uint64_t now, penalty, pmax;
  uint32_t *o_src, *o_cnt;
  uint64_t* o_due;
  __device__ void begin() {}
  __device__ uint64_t src(uint64_t t) const { return t; }
  __device__ bool take(uint64_t t, uint64_t) const { return rc[t] == want; }
  __device__ void row(uint64_t q, uint64_t t, uint64_t) const {
    uint32_t c = cnt_in ? cnt_in[t] : 0;
    if (c != 0xFFFFFFFFu) c++;
    o_src[q] = src_in ? src_in[t] : (uint32_t)t;
    o_cnt[q] = c;
    o_due[q] = aq_due(now, aq_penalty(policy, penalty, pmax, c));
  }
};

// pool entries by due < now (flip: the others), with their per-txn arrays
struct DueSel {
  const uint64_t* due;
  uint64_t now;
  bool flip;
  const uint32_t *src_in, *cnt_in;
  uint32_t *o_src, *o_cnt;
  uint64_t* o_due;
  __device__ void begin() {}
  __device__ uint64_t src(uint64_t t) const { return t; }
  __device__ bool take(uint64_t t, uint64_t) const { return (due[t] < now) != flip; }
  __device__ void row(uint64_t q, uint64_t t, uint64_t) const {
    o_src[q] = src_in[t];
    o_cnt[q] = cnt_in[t];
    o_due[q] = due[t];
  }
};

// position t of the sorted pairs: the pool entry perm[t], taken while t < the
// due count (a device value: the launch is sized by the pool)
struct PermSel {
  const uint32_t* perm;
  const uint64_t* total;  // the due pair
  uint64_t n_due;
  const uint32_t *src_in, *cnt_in;
  const uint64_t* due;
  uint32_t *o_src, *o_cnt;  // each may be null
  uint64_t* o_due;
  __device__ void begin() { n_due = *total & 0xFFFFFFFFull; }
  __device__ uint64_t src(uint64_t t) const { return perm[t]; }
  __device__ bool take(uint64_t t, uint64_t) const { return t < n_due; }
  __device__ void row(uint64_t q, uint64_t, uint64_t s) const {
    if (o_src) o_src[q] = src_in[s];
    if (o_cnt) o_cnt[q] = cnt_in[s];
    if (o_due) o_due[q] = due[s];
  }
};

template <bool CHECK, class Sel>
__global__ __launch_bounds__(SEL_T) void k_aq_count(const uint32_t* __restrict__ off, uint64_t n, uint64_t nnz,
                                                    Sel S, uint64_t n_tiles, uint64_t* __restrict__ part,
                                                    uint64_t* __restrict__ err) {
  csr_count_tiles<CHECK>(off, n, nnz, S, n_tiles, part, err);
}

__global__ __launch_bounds__(SEL_T) void k_aq_scan(uint64_t* __restrict__ part, uint64_t n_tiles, uint64_t cap_txn,
                                                   uint64_t cap_nnz, uint64_t nnz_base, uint64_t* __restrict__ err,
                                                   uint64_t* __restrict__ total) {
  csr_scan_tiles(part, n_tiles, cap_txn, cap_nnz, nnz_base, err, total);
}

template <class Sel>
struct AqMove {
  CsrMove M;
  Sel S;
};
template <class Sel>
__global__ __launch_bounds__(SEL_T) void k_aq_scatter(AqMove<Sel> A) {
  csr_scatter_tiles(A.M, A.S);
}

// One sort pair per pool entry t: a due one goes to its rank among the due
// (part: the scanned tile pairs of the due count) with key due - lo, any other
// behind all of them, at n_due + its rank among the others, with the key
// pad = now - lo, larger than every due key.  Writes sort buffers only.
__global__ __launch_bounds__(SEL_T) void k_aq_pairs(const uint64_t* __restrict__ due, uint64_t n, uint64_t n_tiles,
                                                    uint64_t now, uint64_t lo, uint64_t pad,
                                                    const uint64_t* __restrict__ part,
                                                    const uint64_t* __restrict__ total, uint64_t* __restrict__ ok,
                                                    uint32_t* __restrict__ ov) {
  __shared__ uint32_t s_w[SEL_NW];
  const uint64_t n_due = *total & 0xFFFFFFFFull;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t t = tile * SEL_T + threadIdx.x;
    uint64_t dv = 0;
    bool is = false;
    if (t < n) {
      dv = due[t];
      is = dv < now;
    }
    uint32_t tot;
    const uint32_t ex = block_excl_reuse<AddOp<uint32_t>>(is ? 1u : 0u, s_w, SEL_NW, tot);
    if (t < n) {
      const uint64_t before = (part[tile] & 0xFFFFFFFFull) + ex;  // due entries in front of t
      const uint64_t q = is ? before : n_due + (t - before);      // < n either way
      ok[q] = is ? dv - lo : pad;
      ov[q] = (uint32_t)t;
    }
  }
}

uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }
uint64_t aq_tiles(uint64_t n) { return (n + SEL_T - 1) / SEL_T; }
uint32_t bit_length(uint64_t x) { return x ? 64 - (uint32_t)__builtin_clzll(x) : 0; }

// offsets[txn_base] = nnz_base, the whole of an empty release
int write_base(dcc_ctx* ctx, const dcc_select_out* out, bool dev) {
  const uint32_t v = (uint32_t)out->nnz_base;
  if (dev) {
    *(uint32_t*)ctx->hmisc = v;
    CK(hipMemcpyAsync(out->offsets + out->txn_base, ctx->hmisc, 4, hipMemcpyHostToDevice, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
  } else {
    out->offsets[out->txn_base] = v;
  }
  return DCC_OK;
}

}  // namespace

int dcc_ctx::abortq_alloc(dcc_abortq* q) {
  const uint64_t ct = q->P.cap_txn, cm = q->P.cap_nnz;
  for (auto& p : q->pool) {
    CR(p.off.ensure(this, (ct + 1) * 4, "abort queue offsets"));
    CR(p.keys.ensure(this, cm * 8, "abort queue keys"));
    CR(p.at.ensure(this, cm, "abort queue access types"));
    CR(p.src.ensure(this, ct * 4, "abort queue src"));
    CR(p.cnt.ensure(this, ct * 4, "abort queue cnt"));
    CR(p.due.ensure(this, ct * 8, "abort queue due"));
  }
  for (int x = 0; x < 2; x++) {
    CR(q->sk[x].ensure(this, ct * 8, "abort queue sort keys"));
    CR(q->sv[x].ensure(this, ct * 4, "abort queue sort values"));
  }
  CR(q->scratch.ensure(this, rs_scratch_words(ct) * 4, "abort queue sort scratch"));
  CR(q->ctl.ensure(this, AQ_C_WORDS * 8, "abort queue control words"));
  CR(q->part.ensure(this, 3 * (aq_tiles(ct) + 1) * 8, "abort queue tile pairs"));
  return DCC_OK;
}

int dcc_ctx::abortq_push(dcc_abortq* q, const dcc_batch* b, const uint8_t* rc_in, uint8_t want,
                         const uint32_t* src_in, const uint32_t* cnt_in, uint64_t now, uint64_t* out_n,
                         uint64_t* out_nnz, dcc_stats* st) {
  dcc_ctx* ctx = this;
  EpochStats es;
  dcc_stats& S = es.S;
  if (out_n) *out_n = 0;
  if (out_nnz) *out_nnz = 0;
  CR(check_batch(b, false));  // txn length is free here; the offsets are checked on the device
  const uint64_t n = b->n_txn;
  if (n && !rc_in) return fail(DCC_EINVAL, "abort queue push: null rc");
  if (n == 0) {
    S.alg_bytes = dcc_abortq_push_alg_bytes(0, 0, 0);
    es.wall();
    if (st) *st = S;
    return DCC_OK;
  }
  const bool dev = (b->flags & DCC_DEVICE_PTRS) != 0;
  DevBatch d;
  CR(stage_batch(b, d));  // compact forms are widened here: the gather reads the wide form
  const uint64_t m = d.nnz;
  const uint64_t n_tiles = aq_tiles(n);
  CR(sel_part.ensure(this, (n_tiles + 1) * 8, "select tile pairs"));
  uint64_t* ctl = (uint64_t*)q->ctl.p;
  uint64_t* part = (uint64_t*)sel_part.p;
  dcc_abortq::Pool& P = q->pool[q->cur];

  AqMove<PushSel> A{};
  A.M.n = n;
  A.M.n_tiles = n_tiles;
  A.M.off = d.off;
  A.M.keys = d.keys;
  A.M.at = d.acctype;
  A.M.nnz_base = q->nnz;
  A.M.o_off = (uint32_t*)P.off.p + q->n;
  A.M.o_keys = (uint64_t*)P.keys.p + q->nnz;
  A.M.o_at = (uint8_t*)P.at.p + q->nnz;
  A.M.part = part;
  A.M.err = &ctl[AQ_C_ERR];
  A.S.want = want;
  A.S.policy = q->P.policy;
  A.S.now = now;
  A.S.penalty = q->P.penalty;
  A.S.pmax = q->P.penalty_max;
  A.S.o_src = (uint32_t*)P.src.p + q->n;
  A.S.o_cnt = (uint32_t*)P.cnt.p + q->n;
  A.S.o_due = (uint64_t*)P.due.p + q->n;
  CR(stage(sel_rc, rc_in, n, dev, "select rc", A.S.rc));
  if (src_in) CR(stage(sel_src, src_in, n * 4, dev, "select src", A.S.src_in));
  if (cnt_in) CR(stage(q->st_cnt, cnt_in, n * 4, dev, "abort queue cnt_in", A.S.cnt_in));

  const unsigned grid = sel_grid(n_tiles, (unsigned)n_cu * 16);
  const bool prof = profiling;
  CK(hipMemsetAsync(ctl, 0, AQ_C_WORDS * 8, stream));
  CK(hipEventRecord(ev0, stream));
  if (prof) CK(hipEventRecord(pev[0], stream));
  k_aq_count<true, PushSel><<<grid, SEL_T, 0, stream>>>(d.off, n, m, A.S, n_tiles, part, &ctl[AQ_C_ERR]);
  if (prof) CK(hipEventRecord(pev[1], stream));
  k_aq_scan<<<1, SEL_T, 0, stream>>>(part, n_tiles, q->P.cap_txn - q->n, q->P.cap_nnz - q->nnz, q->nnz,
                                     &ctl[AQ_C_ERR], &ctl[AQ_C_TOTAL]);
  if (prof) CK(hipEventRecord(pev[2], stream));
  k_aq_scatter<PushSel><<<grid, SEL_T, 0, stream>>>(A);
  CK(hipGetLastError());
  if (prof) CK(hipEventRecord(pev[3], stream));
  CK(hipEventRecord(ev1, stream));
  CK(hipMemcpyAsync(hmisc, ctl, AQ_C_WORDS * 8, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  const uint64_t* hc = (const uint64_t*)hmisc;
  const uint64_t verdict = hc[AQ_C_ERR];
  if (verdict & SEL_ERR_OFF) return fail(DCC_EINVAL, "batch: malformed offsets");
  const uint64_t ns = hc[AQ_C_TOTAL] & 0xFFFFFFFFull, ms = hc[AQ_C_TOTAL] >> 32;
  if (out_n) *out_n = ns;
  if (out_nnz) *out_nnz = ms;
  S.n_commit = ns;
  S.n_abort = n - ns;
  if (verdict & SEL_ERR_CAP) {
    if (st) *st = S;
    return fail(DCC_ERANGE, "abort queue push: %llu txns / %llu accesses to park, room for %llu / %llu",
                (unsigned long long)ns, (unsigned long long)ms, (unsigned long long)(q->P.cap_txn - q->n),
                (unsigned long long)(q->P.cap_nnz - q->nnz));
  }
  // a clear verdict: the entries are in the pool, the host state follows
  if (ns) {
    if (q->n == 0) q->due_lo = now;
    else q->due_lo = std::min(q->due_lo, now);
  }
  q->n += ns;
  q->nnz += ms;
  q->seq += ns;
  S.alg_bytes = dcc_abortq_push_alg_bytes(n, ns, ms);
  CR(es.finish(this, 3));
  if (st) *st = S;
  return DCC_OK;
}

int dcc_ctx::abortq_pop(dcc_abortq* q, uint64_t now, const dcc_select_out* out, uint32_t* out_cnt,
                        uint64_t* out_due, uint32_t flags, uint64_t* out_n, uint64_t* out_nnz, dcc_stats* st) {
  dcc_ctx* ctx = this;
  EpochStats es;
  dcc_stats& S = es.S;
  if (out_n) *out_n = 0;
  if (out_nnz) *out_nnz = 0;
  if (!out || !out->offsets) return fail(DCC_EINVAL, "abort queue pop: null out / out offsets");
  if (out->cap_nnz && (!out->keys || !out->acctype))
    return fail(DCC_EINVAL, "abort queue pop: null out keys/acctype");
  if (out->nnz_base > 0xFFFFFFFFull) return fail(DCC_ERANGE, "abort queue pop: nnz_base exceeds 2^32-1");
  const bool dev = (flags & DCC_DEVICE_PTRS) != 0;
  const uint64_t n = q->n, m = q->nnz;
  if (n == 0 || now <= q->due_lo) {  // every parked due is >= due_lo: nothing is due
    CR(write_base(this, out, dev));
    S.n_abort = n;
    S.alg_bytes = dcc_abortq_pop_alg_bytes(n, m, 0, 0);
    es.wall();
    if (st) *st = S;
    return DCC_OK;
  }
  const uint64_t n_tiles = aq_tiles(n), pstride = aq_tiles(q->P.cap_txn) + 1;
  uint64_t* ctl = (uint64_t*)q->ctl.p;
  uint64_t* part_due = (uint64_t*)q->part.p;
  uint64_t* part_gat = part_due + pstride;
  uint64_t* part_keep = part_gat + pstride;
  dcc_abortq::Pool& P = q->pool[q->cur];
  dcc_abortq::Pool& Q = q->pool[q->cur ^ 1];
  const uint32_t* p_off = (const uint32_t*)P.off.p;
  const uint64_t* p_due = (const uint64_t*)P.due.p;
  const bool w_src = out->src != nullptr, w_cnt = out_cnt != nullptr, w_due = out_due != nullptr;

  // the sort keys: due - lo of the due entries is < pad = now - lo
  const bool full = (q->P.flags & DCC_ABORTQ_SORT_FULL) != 0;
  const uint64_t lo = full ? 0 : q->due_lo, pad = now - lo;
  const uint32_t bits = full ? 64 : bit_length(pad);

  DueSel due_sel{};
  due_sel.due = p_due;
  due_sel.now = now;
  due_sel.src_in = (const uint32_t*)P.src.p;
  due_sel.cnt_in = (const uint32_t*)P.cnt.p;

  AqMove<PermSel> G{};
  G.M.n = n;
  G.M.n_tiles = n_tiles;
  G.M.off = p_off;
  G.M.keys = (const uint64_t*)P.keys.p;
  G.M.at = (const uint8_t*)P.at.p;
  G.M.nnz_base = out->nnz_base;
  G.M.part = part_gat;
  G.M.err = &ctl[AQ_C_ERR];
  G.S.total = &ctl[AQ_C_TOTAL];
  G.S.src_in = due_sel.src_in;
  G.S.cnt_in = due_sel.cnt_in;
  G.S.due = p_due;
  uint64_t *h_keys = nullptr, *h_due = nullptr;
  uint32_t *h_off = nullptr, *h_src = nullptr, *h_cnt = nullptr;
  uint8_t* h_at = nullptr;
  if (dev) {
    G.M.o_off = out->offsets + out->txn_base;
    G.M.o_keys = out->keys ? out->keys + out->nnz_base : nullptr;
    G.M.o_at = out->acctype ? out->acctype + out->nnz_base : nullptr;
    G.S.o_src = w_src ? out->src + out->txn_base : nullptr;
    G.S.o_cnt = w_cnt ? out_cnt + out->txn_base : nullptr;
    G.S.o_due = w_due ? out_due + out->txn_base : nullptr;
  } else {
    // the most the call can write: the capacities, and no more than the queue holds
    const uint64_t room_n = std::min(out->cap_txn, n), room_m = std::min(out->cap_nnz, m);
    CR(q->st_out.ensure(this, room_m * 8 + room_n * 8 + up16((room_n + 1) * 4) + 2 * up16(room_n * 4) + room_m + 64,
                        "abort queue pop outputs"));
    uint8_t* o = (uint8_t*)q->st_out.p;
    h_keys = (uint64_t*)o;
    o += room_m * 8;
    h_due = (uint64_t*)o;
    o += room_n * 8;
    h_off = (uint32_t*)o;
    o += up16((room_n + 1) * 4);
    h_src = (uint32_t*)o;
    o += up16(room_n * 4);
    h_cnt = (uint32_t*)o;
    o += up16(room_n * 4);
    h_at = o;
    G.M.o_off = h_off;
    G.M.o_keys = h_keys;
    G.M.o_at = h_at;
    G.S.o_src = w_src ? h_src : nullptr;
    G.S.o_cnt = w_cnt ? h_cnt : nullptr;
    G.S.o_due = w_due ? h_due : nullptr;
  }

  AqMove<DueSel> K{};
  K.M.n = n;
  K.M.n_tiles = n_tiles;
  K.M.off = p_off;
  K.M.keys = G.M.keys;
  K.M.at = G.M.at;
  K.M.nnz_base = 0;
  K.M.o_off = (uint32_t*)Q.off.p;
  K.M.o_keys = (uint64_t*)Q.keys.p;
  K.M.o_at = (uint8_t*)Q.at.p;
  K.M.part = part_keep;
  K.M.err = &ctl[AQ_C_ERR];
  K.S = due_sel;
  K.S.flip = true;
  K.S.o_src = (uint32_t*)Q.src.p;
  K.S.o_cnt = (uint32_t*)Q.cnt.p;
  K.S.o_due = (uint64_t*)Q.due.p;

  uint64_t* sk[2] = {(uint64_t*)q->sk[0].p, (uint64_t*)q->sk[1].p};
  uint32_t* sv[2] = {(uint32_t*)q->sv[0].p, (uint32_t*)q->sv[1].p};
  const unsigned grid = sel_grid(n_tiles, (unsigned)n_cu * 16);
  const bool prof = profiling;
  const uint64_t NOCAP = ~0ull;  // the pools hold whatever the queue holds
  CK(hipMemsetAsync(ctl, 0, AQ_C_WORDS * 8, stream));
  CK(hipEventRecord(ev0, stream));
  if (prof) CK(hipEventRecord(pev[0], stream));
  // 0: due flags and counts, the verdict, the sort pairs
  k_aq_count<false, DueSel><<<grid, SEL_T, 0, stream>>>(p_off, n, m, due_sel, n_tiles, part_due, &ctl[AQ_C_ERR]);
  k_aq_scan<<<1, SEL_T, 0, stream>>>(part_due, n_tiles, out->cap_txn, out->cap_nnz, out->nnz_base, &ctl[AQ_C_ERR],
                                     &ctl[AQ_C_TOTAL]);
  k_aq_pairs<<<grid, SEL_T, 0, stream>>>(p_due, n, n_tiles, now, lo, pad, part_due, &ctl[AQ_C_TOTAL], sk[0], sv[0]);
  if (prof) CK(hipEventRecord(pev[1], stream));
  // 1: sort
  const int r = radix_sort_u64(sk, sv, n, bits, (uint32_t*)q->scratch.p, stream);
  G.S.perm = sv[r];
  if (prof) CK(hipEventRecord(pev[2], stream));
  // 2: gather of the released txns
  k_aq_count<false, PermSel><<<grid, SEL_T, 0, stream>>>(p_off, n, m, G.S, n_tiles, part_gat, &ctl[AQ_C_ERR]);
  k_aq_scan<<<1, SEL_T, 0, stream>>>(part_gat, n_tiles, NOCAP, NOCAP, 0, &ctl[AQ_C_ERR], &ctl[AQ_C_GATHER]);
  k_aq_scatter<PermSel><<<grid, SEL_T, 0, stream>>>(G);
  if (prof) CK(hipEventRecord(pev[3], stream));
  // 3: compaction of the kept ones
  k_aq_count<false, DueSel><<<grid, SEL_T, 0, stream>>>(p_off, n, m, K.S, n_tiles, part_keep, &ctl[AQ_C_ERR]);
  k_aq_scan<<<1, SEL_T, 0, stream>>>(part_keep, n_tiles, NOCAP, NOCAP, 0, &ctl[AQ_C_ERR], &ctl[AQ_C_KEEP]);
  k_aq_scatter<DueSel><<<grid, SEL_T, 0, stream>>>(K);
  CK(hipGetLastError());
  if (prof) CK(hipEventRecord(pev[4], stream));
  CK(hipEventRecord(ev1, stream));
  CK(hipMemcpyAsync(hmisc, ctl, AQ_C_WORDS * 8, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  const uint64_t* hc = (const uint64_t*)hmisc;
  const uint64_t verdict = hc[AQ_C_ERR];
  const uint64_t ns = hc[AQ_C_TOTAL] & 0xFFFFFFFFull, ms = hc[AQ_C_TOTAL] >> 32;
  if (out_n) *out_n = ns;
  if (out_nnz) *out_nnz = ms;
  S.n_commit = ns;
  S.n_abort = n - ns;
  if (verdict & SEL_ERR_CAP) {
    if (st) *st = S;
    return fail(DCC_ERANGE, "abort queue pop: %llu txns / %llu accesses due, room for %llu / %llu behind nnz_base %llu",
                (unsigned long long)ns, (unsigned long long)ms, (unsigned long long)out->cap_txn,
                (unsigned long long)out->cap_nnz, (unsigned long long)out->nnz_base);
  }
  if (hc[AQ_C_GATHER] != hc[AQ_C_TOTAL] || (hc[AQ_C_KEEP] & 0xFFFFFFFFull) != n - ns || (hc[AQ_C_KEEP] >> 32) != m - ms)
    return fail(DCC_EIO, "abort queue pop: the passes disagree on the counts");
  if (!dev) {
    const uint64_t tb = out->txn_base, xb = out->nnz_base;
    CK(hipMemcpyAsync(out->offsets + tb, h_off, (ns + 1) * 4, hipMemcpyDeviceToHost, stream));
    if (ms) {
      CK(hipMemcpyAsync(out->keys + xb, h_keys, ms * 8, hipMemcpyDeviceToHost, stream));
      CK(hipMemcpyAsync(out->acctype + xb, h_at, ms, hipMemcpyDeviceToHost, stream));
    }
    if (ns) {
      if (w_src) CK(hipMemcpyAsync(out->src + tb, h_src, ns * 4, hipMemcpyDeviceToHost, stream));
      if (w_cnt) CK(hipMemcpyAsync(out_cnt + tb, h_cnt, ns * 4, hipMemcpyDeviceToHost, stream));
      if (w_due) CK(hipMemcpyAsync(out_due + tb, h_due, ns * 8, hipMemcpyDeviceToHost, stream));
    }
    CK(hipStreamSynchronize(stream));
  }
  // a clear verdict: the kept entries are the other pool
  if (ns) {
    q->cur ^= 1;
    q->n = n - ns;
    q->nnz = m - ms;
    if (q->n == 0) q->due_lo = ~0ull;
  }
  S.alg_bytes = dcc_abortq_pop_alg_bytes(n, m, ns, ms);
  CR(es.finish(this, 4));
  if (st) *st = S;
  return DCC_OK;
}

extern "C" uint64_t dcc_abortq_push_alg_bytes(uint64_t n_txn, uint64_t n_sel, uint64_t nnz_sel) {
  return dcc_select_alg_bytes(n_txn, n_sel, nnz_sel, 1) + 12 * n_sel;
}

extern "C" uint64_t dcc_abortq_pop_alg_bytes(uint64_t n_q, uint64_t nnz_q, uint64_t n_due, uint64_t nnz_due) {
  (void)nnz_due;
  const uint64_t flags = 8 * n_q + 4 * (n_q + 1);
  if (n_due == 0) return flags;
  return flags + 24 * n_q + 18 * nnz_q + 4 * (n_due + 1) + 4 * (n_q - n_due + 1) + 32 * n_q;
}

// the queue's call on the context that runs it: rank 0's of a multi-GPU one
template <typename F>
static int aq_run(dcc_abortq* q, F call) {
  dcc_ctx* ctx = q->owner;
  dcc_pipe_drain(ctx);  // pipelined OCC epochs in flight complete first
  if (ctx->multi)       // a local data movement: rank 0's GPU, its communicator left alone
    return dcc_multi_on_rank0(ctx, false, call);
  if (hipSetDevice(ctx->device) != hipSuccess) return DCC_ENODEV;
  return call(ctx);
}

extern "C" int dcc_abortq_create(dcc_ctx* ctx, const dcc_abortq_params* params, dcc_abortq** out) {
  if (!ctx || !out) return DCC_EINVAL;
  *out = nullptr;
  if (!params) return ctx->fail(DCC_EINVAL, "abort queue: null params");
  if (params->cap_txn > 0xFFFFFFFFull || params->cap_nnz > 0xFFFFFFFFull)
    return ctx->fail(DCC_ERANGE, "abort queue: cap_txn / cap_nnz exceed 2^32-1");
  if (params->policy > DCC_BACKOFF_EXP) return ctx->fail(DCC_EINVAL, "abort queue: unknown policy");
  std::unique_ptr<dcc_abortq> q(new dcc_abortq());
  q->owner = ctx;
  q->P = *params;
  const int e = aq_run(q.get(), [&](dcc_ctx* s) { return s->abortq_alloc(q.get()); });
  if (e != DCC_OK) return e;  // what was allocated goes with q
  *out = q.get();
  ctx->abortqs.push_back(std::move(q));
  return DCC_OK;
}

extern "C" void dcc_abortq_destroy(dcc_abortq* q) {
  if (!q) return;
  dcc_ctx* ctx = q->owner;
  (void)aq_run(q, [&](dcc_ctx* s) {  // its last call's work is done before the memory goes
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    return DCC_OK;
  });
  auto& v = ctx->abortqs;
  for (size_t i = 0; i < v.size(); i++)
    if (v[i].get() == q) {
      v.erase(v.begin() + i);  // the DevBuf members free the device memory
      return;
    }
}

extern "C" int dcc_abortq_push(dcc_abortq* q, const dcc_batch* batch, const uint8_t* rc, uint8_t want,
                               const uint32_t* src_in, const uint32_t* cnt_in, uint64_t now, uint64_t* out_n,
                               uint64_t* out_nnz, dcc_stats* out_stats) {
  if (!q || !batch) return DCC_EINVAL;
  return aq_run(q, [&](dcc_ctx* s) {
    return s->abortq_push(q, batch, rc, want, src_in, cnt_in, now, out_n, out_nnz, out_stats);
  });
}

extern "C" int dcc_abortq_pop(dcc_abortq* q, uint64_t now, const dcc_select_out* out, uint32_t* out_cnt,
                              uint64_t* out_due, uint32_t flags, uint64_t* out_n, uint64_t* out_nnz,
                              dcc_stats* out_stats) {
  if (!q) return DCC_EINVAL;
  return aq_run(q, [&](dcc_ctx* s) {
    return s->abortq_pop(q, now, out, out_cnt, out_due, flags, out_n, out_nnz, out_stats);
  });
}

extern "C" int dcc_abortq_size(const dcc_abortq* q, uint64_t* out_n, uint64_t* out_nnz) {
  if (!q) return DCC_EINVAL;
  if (out_n) *out_n = q->n;
  if (out_nnz) *out_nnz = q->nnz;
  return DCC_OK;
}

extern "C" int dcc_abortq_clear(dcc_abortq* q) {
  if (!q) return DCC_EINVAL;
  q->n = q->nnz = 0;
  q->due_lo = ~0ull;
  return DCC_OK;
}
