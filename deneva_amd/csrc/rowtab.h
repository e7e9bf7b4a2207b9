// The persistent row table of MaaT and TIMESTAMP: RowTab's methods
// (dcc_ctx.h) and their kernels.  One 32-byte slot per row -- the key and its
// two values side by side, so the access that finds a row has its values in
// the same 64-byte line -- open addressing with a unit step from the home slot
// of the engine's probe policy P (dcc_device.h), at most half full, 2^12 to
// 2^31 slots, doubling with a rehash.  The device counts the rows a call adds
// (ctl[RT_NEW]) and the host adds that to `rows`; an engine's epoch does the
// same with its own kernels and counter words.
//
// Included by the engine's .hip: the kernels are per file, the methods are
// instantiated with the engine's policy.
#pragma once
#include <algorithm>
#include <cstring>

#include "dcc_ctx.h"
#include "dcc_device.h"
#include "dcc_scan.h"

namespace dcc {

struct __attribute__((aligned(32))) RowSlot {
  uint64_t key, a, b, pad;
};
static_assert(sizeof(RowSlot) == 32, "row slot");
constexpr uint32_t RT_MIN_BITS = 12, RT_MAX_BITS = 31;
constexpr uint32_t RT_ERR = 0, RT_NEW = 1, RT_WORDS = 2;  // ctl: a walk ran out; rows added

namespace {

// an empty table: every key KEY_EMPTY, values 0
__global__ __launch_bounds__(256) void k_rt_clear(RowSlot* rt, uint64_t cap) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * 256)
    rt[i] = RowSlot{KEY_EMPTY, 0, 0, 0};
}

// insert `key` or find it, and overwrite its values; 1: a new row.  A walk
// that ran out is reported and writes nothing.
template <class P>
__device__ inline uint32_t row_put(RowSlot* rt, uint32_t mask, uint64_t key, uint64_t a, uint64_t b,
                                   uint32_t* ctl) {
  bool ins;
  const uint32_t s = probe_insert<P>(rt, mask, key, ins);
  if (s == ROW_NONE) {
    atomicOr(&ctl[RT_ERR], 1u);
    return 0;
  }
  rt[s].a = a;
  rt[s].b = b;
  return ins;
}
// every row of the old table into the new one (values carried)
template <class P>
__global__ __launch_bounds__(256) void k_rt_rehash(const RowSlot* ot, uint64_t ocap, RowSlot* nt, uint32_t nmask,
                                                   uint32_t* ctl) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < ocap; i += (uint64_t)gridDim.x * 256) {
    const RowSlot o = ot[i];
    if (o.key != KEY_EMPTY) row_put<P>(nt, nmask, o.key, o.a, o.b, ctl);
  }
}
template <class P>
__global__ __launch_bounds__(256) void k_rt_set(const uint64_t* keys, const uint64_t* a, const uint64_t* b,
                                                uint64_t n, RowSlot* rt, uint32_t mask, uint32_t* ctl) {
  uint32_t c = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
    c += row_put<P>(rt, mask, keys[i], a[i], b[i], ctl);
  block_add<4>(c, &ctl[RT_NEW]);
}
// (0, 0) for a key the table does not have
template <class P>
__global__ __launch_bounds__(256) void k_rt_get(const uint64_t* keys, uint64_t n, const RowSlot* rt, uint32_t mask,
                                                uint64_t* a, uint64_t* b) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const uint32_t s = probe_find<P>(rt, mask, keys[i]);
    a[i] = s == ROW_NONE ? 0 : rt[s].a;
    b[i] = s == ROW_NONE ? 0 : rt[s].b;
  }
}

inline unsigned rt_grid(uint64_t items) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + 255) / 256, 16384));
}

}  // namespace
}  // namespace dcc

// Capacity for `want` rows at <= 50 % load.  The new table is built completely
// and its error word read before it replaces the one in use; a policy with a
// bounded walk that reports one past its bound gets twice the slots, rehashed
// from the old, intact table again.
template <class P>
int RowTab::reserve(dcc_ctx* ctx, uint64_t want) {
  using namespace dcc;
  if (bits && 2 * want <= (1ull << bits)) return DCC_OK;
  uint32_t nb = std::max(bits, RT_MIN_BITS);
  while ((1ull << nb) < 2 * want) nb++;
  CR(ctl.ensure(ctx, RT_WORDS * 4, "row table counters"));
  DevBuf nt;
  for (;; nb++) {
    if (nb > RT_MAX_BITS) return ctx->fail(DCC_ERANGE, "%s: row table exceeds 2^31 slots", name);
    const uint64_t cap = 1ull << nb, ocap = 1ull << bits;
    CR(nt.ensure(ctx, cap * sizeof(RowSlot), "row table"));
    k_rt_clear<<<rt_grid(cap), 256, 0, ctx->stream>>>((RowSlot*)nt.p, cap);
    CK(hipMemsetAsync(ctl.p, 0, RT_WORDS * 4, ctx->stream));
    if (bits)
      k_rt_rehash<P><<<rt_grid(ocap), 256, 0, ctx->stream>>>((const RowSlot*)buf.p, ocap, (RowSlot*)nt.p,
                                                             (uint32_t)(cap - 1), (uint32_t*)ctl.p);
    CK(hipGetLastError());
    uint32_t err = 0;
    CK(hipMemcpyAsync(&err, ctl.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if (!err) break;
    if (P::walk_last == ~0u) return ctx->fail(DCC_EIO, "%s: row table rehash failed", name);
  }
  buf = std::move(nt);
  bits = nb;
  return DCC_OK;
}

inline int RowTab::clear(dcc_ctx* ctx) {
  if (bits) {
    dcc::k_rt_clear<<<dcc::rt_grid(1ull << bits), 256, 0, ctx->stream>>>((dcc::RowSlot*)buf.p, 1ull << bits);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(ctx->stream));
  }
  rows = 0;
  return DCC_OK;
}

// Insert and overwrite.  A reserved key rejects the call before the table changes.
template <class P>
int RowTab::set(dcc_ctx* ctx, const uint64_t* keys, const uint64_t* a, const uint64_t* b, uint64_t n) {
  using namespace dcc;
  for (uint64_t i = 0; i < n; i++)
    if (keys[i] == DCC_KEY_RESERVED) return ctx->fail(DCC_EINVAL, "%s rows: key equal to DCC_KEY_RESERVED", name);
  if (n == 0) return DCC_OK;
  CR(reserve<P>(ctx, rows + n));
  DevBuf tmp;
  CR(tmp.ensure(ctx, n * 24, "row table seed"));
  uint64_t* t = (uint64_t*)tmp.p;
  CK(hipMemsetAsync(ctl.p, 0, RT_WORDS * 4, ctx->stream));
  CK(hipMemcpyAsync(t, keys, n * 8, hipMemcpyHostToDevice, ctx->stream));
  CK(hipMemcpyAsync(t + n, a, n * 8, hipMemcpyHostToDevice, ctx->stream));
  CK(hipMemcpyAsync(t + 2 * n, b, n * 8, hipMemcpyHostToDevice, ctx->stream));
  k_rt_set<P><<<rt_grid(n), 256, 0, ctx->stream>>>(t, t + n, t + 2 * n, n, (RowSlot*)buf.p, mask(),
                                                   (uint32_t*)ctl.p);
  CK(hipGetLastError());
  uint32_t hc[RT_WORDS];
  CK(hipMemcpyAsync(hc, ctl.p, sizeof hc, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  rows += hc[RT_NEW];  // rows entered stay in the table whatever follows
  if (hc[RT_ERR]) return ctx->fail(DCC_EIO, "%s: row table full", name);
  return DCC_OK;
}

template <class P>
int RowTab::get(dcc_ctx* ctx, const uint64_t* keys, uint64_t* a, uint64_t* b, uint64_t n) {
  using namespace dcc;
  if (n == 0) return DCC_OK;
  if (!bits) {
    memset(a, 0, n * 8);
    memset(b, 0, n * 8);
    return DCC_OK;
  }
  DevBuf tmp;
  CR(tmp.ensure(ctx, n * 24, "row table get"));
  uint64_t* t = (uint64_t*)tmp.p;
  CK(hipMemcpyAsync(t, keys, n * 8, hipMemcpyHostToDevice, ctx->stream));
  k_rt_get<P><<<rt_grid(n), 256, 0, ctx->stream>>>(t, n, (const RowSlot*)buf.p, mask(), t + n, t + 2 * n);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(a, t + n, n * 8, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipMemcpyAsync(b, t + 2 * n, n * 8, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return DCC_OK;
}
