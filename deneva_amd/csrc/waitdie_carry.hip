// Carry a WAIT_DIE population across epochs (dcc_waitdie_carry): the txns that
// are not GONE (and the GONE ones the caller revives) move to the front of a
// new CSR with their ts / rc / pos / src, the fresh arrivals are appended
// behind them as (RUN, 0).  DESIGN.md §8o.
//
// The stayers are a stream compaction over a ragged CSR: csr_select.h's tile
// bodies with a Sel whose predicate is the state byte and whose rows are the
// WAIT_DIE state.  New here: the state rule of the epoch's check (live_txn.h)
// applied in the counting pass, a capacity verdict that covers stayers +
// fresh, and the append, which starts at a base only the device knows.
//
// Kernels:  k_wc_count    one pair per tile of SEL_T txns; the offsets and the
//                         (rc, pos, revive) rule are checked here, the revived
//                         txns counted: per wave into LDS, one word per
//                         workgroup out (no global atomic on an accepted call)
//           k_wc_fresh    the fresh offsets, checked before the append indexes
//                         with them
//           k_wc_scan     one workgroup: exclusive scan of the tile pairs, the
//                         stayers' totals, the verdict for stayers + fresh
//           k_wc_scatter  the stayers: csr_scatter_tiles
//           k_wc_append   the fresh txns behind the stayers' totals: a
//                         streaming copy, 16 bytes per lane where source and
//                         destination allow, scalar heads and tails
// No workgroup waits on another.  The scatter and the append read the verdict
// first and write nothing unless it is clear; the host reads totals and
// verdict once, after the last launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>

#include "csr_select.h"
#include "dcc.h"
#include "dcc_ctx.h"
#include "dcc_device.h"
#include "dcc_scan.h"
#include "live_txn.h"

using namespace dcc;

namespace {

// control words (sel_misc): u64 [0] verdict, [1] stayers | their accesses << 32,
// [2] revived txns
constexpr uint32_t WC_C_ERR = 0, WC_C_TOTAL = 1, WC_C_REVIVED = 2, WC_C_WORDS = 3;
// verdict bits next to SEL_ERR_OFF / SEL_ERR_CAP
constexpr uint32_t WC_ERR_RC = 4, WC_ERR_POS = 8, WC_ERR_REVIVE = 16, WC_ERR_FOFF = 32;
constexpr uint32_t WC_T = 256;  // threads per workgroup of the append

// Txn t stays iff it is not GONE or is revived.  With CHECK (the counting
// pass) take() also applies the state rule of the epoch's check (live_txn.h's
// live_state_ok / live_pos_ok), so an accepted output is a state the epoch
// accepts, and counts the revived txns.
template <bool CHECK>
struct CarrySel {
  const uint32_t* off;
  const uint64_t* ts;
  const uint8_t* rc;
  const uint32_t* pos;
  const uint8_t* revive;   // or null
  const uint32_t* src_in;  // or null
  uint64_t* ctl;           // CHECK: the control words
  uint32_t* lds_rev;       // CHECK: the workgroup's revived txns (LDS)
  uint64_t* o_ts;
  uint8_t* o_rc;
  uint32_t* o_pos;
  uint32_t* o_src;  // or null
  __device__ void begin() {}
  __device__ uint64_t src(uint64_t t) const { return t; }
  __device__ bool take(uint64_t t, uint64_t) const {
    const uint8_t r = rc[t];
    const bool rev = revive && revive[t] != 0;
    if (CHECK) {
      uint32_t err = 0;
      if (!live_state_ok(r)) {
        err = WC_ERR_RC;
      } else if (r != DCC_WD_GONE) {
        const uint32_t a0 = off[t], b0 = off[t + 1];
        if (b0 >= a0 && !live_pos_ok(r, pos[t], b0 - a0)) err = WC_ERR_POS;
        if (rev) err |= WC_ERR_REVIVE;
      }
      if (err) atomicOr((unsigned long long*)&ctl[WC_C_ERR], (unsigned long long)err);
      // one LDS add per wave: the lowest revived lane adds the wave's count
      const bool rv = rev && r == DCC_WD_GONE;
      const uint64_t mask = __ballot(rv);
      if (rv && (uint32_t)__ffsll((long long)mask) - 1 == (threadIdx.x & 63))
        atomicAdd(lds_rev, (uint32_t)__popcll(mask));
    }
    return r != DCC_WD_GONE || rev;
  }
  __device__ void row(uint64_t q, uint64_t t, uint64_t) const {
    const uint8_t r = rc[t];
    const bool gone = r == DCC_WD_GONE;  // taken and GONE: revived
    o_ts[q] = ts[t];
    o_rc[q] = gone ? (uint8_t)DCC_WD_RUN : r;
    o_pos[q] = gone ? 0u : pos[t];
    if (o_src) o_src[q] = src_in ? src_in[t] : (uint32_t)t;
  }
};

__global__ __launch_bounds__(SEL_T) void k_wc_count(const uint32_t* __restrict__ off, uint64_t n, uint64_t nnz,
                                                    const uint8_t* __restrict__ rc,
                                                    const uint32_t* __restrict__ pos,
                                                    const uint8_t* __restrict__ revive, uint64_t n_tiles,
                                                    uint64_t* __restrict__ part, uint64_t* __restrict__ ctl,
                                                    uint32_t* __restrict__ rev_part) {
  __shared__ uint32_t s_rev;
  if (threadIdx.x == 0) s_rev = 0;
  __syncthreads();
  CarrySel<true> S{};
  S.off = off;
  S.rc = rc;
  S.pos = pos;
  S.revive = revive;
  S.ctl = ctl;
  S.lds_rev = &s_rev;
  csr_count_tiles<true>(off, n, nnz, S, n_tiles, part, &ctl[WC_C_ERR]);
  __syncthreads();
  if (threadIdx.x == 0) rev_part[blockIdx.x] = s_rev;
}

__global__ __launch_bounds__(WC_T) void k_wc_fresh(const uint32_t* __restrict__ off, uint64_t n, uint64_t nnz,
                                                   uint64_t* __restrict__ ctl) {
  bool bad = false;
  for (uint64_t j = (uint64_t)blockIdx.x * WC_T + threadIdx.x; j < n; j += (uint64_t)gridDim.x * WC_T) {
    const uint32_t a0 = off[j], b0 = off[j + 1];
    bad |= b0 < a0 || (j == 0 && a0 != 0) || (j == n - 1 && b0 != nnz);
  }
  if (bad) atomicOr((unsigned long long*)&ctl[WC_C_ERR], (unsigned long long)WC_ERR_FOFF);
}

// The stayers' totals, and the verdict for stayers + fresh: the stayers must
// fit what the fresh txns leave of the capacities, and all accesses a uint32_t.
__global__ __launch_bounds__(SEL_T) void k_wc_scan(uint64_t* __restrict__ part, uint64_t n_tiles, uint64_t cap_txn,
                                                   uint64_t cap_nnz, uint64_t n_fresh, uint64_t nnz_fresh,
                                                   const uint32_t* __restrict__ rev_part, uint32_t n_rev_part,
                                                   uint64_t* __restrict__ ctl) {
  csr_scan_tiles(part, n_tiles, cap_txn >= n_fresh ? cap_txn - n_fresh : 0,
                 cap_nnz >= nnz_fresh ? cap_nnz - nnz_fresh : 0, nnz_fresh, &ctl[WC_C_ERR], &ctl[WC_C_TOTAL]);
  // the same thread as the scan's verdict
  if (threadIdx.x == 0 && (n_fresh > cap_txn || nnz_fresh > cap_nnz)) ctl[WC_C_ERR] |= SEL_ERR_CAP;
  // the counting workgroups' revived txns
  uint32_t rev = 0;
  for (uint32_t q = threadIdx.x; q < n_rev_part; q += SEL_T) rev += rev_part[q];
  if (rev) atomicAdd((unsigned long long*)&ctl[WC_C_REVIVED], (unsigned long long)rev);
}

struct WcArgs {
  CsrMove M;
  CarrySel<false> S;
};

__global__ __launch_bounds__(SEL_T) void k_wc_scatter(WcArgs A) { csr_scatter_tiles(A.M, A.S); }

// The fresh txns and where they go (the outputs at row 0 / access 0: the
// append adds the stayers' totals itself).
struct WcFresh {
  uint64_t n, nnz;
  const uint32_t* off;
  const void* keys;   // u64, or u32 with k32
  const uint8_t* at;  // bytes, or 2-bit codes with a2
  const uint64_t* ts;
  uint32_t src_base;
  bool k32, a2;
  uint32_t* o_off;
  uint64_t* o_keys;
  uint8_t* o_at;
  uint64_t* o_ts;
  uint8_t* o_rc;
  uint32_t* o_pos;
  uint32_t* o_src;  // or null
  const uint64_t* ctl;
};

// four 2-bit codes of a byte as four bytes
__device__ inline uint32_t wc_spread(uint32_t b) {
  uint32_t x = (b | (b << 12)) & 0x000F000Fu;
  return (x | (x << 6)) & 0x03030303u;
}

__device__ inline uint32_t wc_bytes4(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__global__ __launch_bounds__(WC_T) void k_wc_append(WcFresh F) {
  if (F.ctl[WC_C_ERR]) return;  // a rejected call or no room: nothing is written
  const uint64_t tot = F.ctl[WC_C_TOTAL];
  const uint64_t q0 = tot & 0xFFFFFFFFull, x0 = tot >> 32;  // the first fresh row / access
  const uint64_t tid = (uint64_t)blockIdx.x * WC_T + threadIdx.x, stride = (uint64_t)gridDim.x * WC_T;

  // per-txn rows; o_off[q0] is the scatter's
  for (uint64_t j = tid; j < F.n; j += stride) {
    const uint64_t q = q0 + j;
    F.o_off[q + 1] = (uint32_t)(x0 + F.off[j + 1]);
    F.o_ts[q] = F.ts[j];
    F.o_rc[q] = (uint8_t)DCC_WD_RUN;
    F.o_pos[q] = 0;
    if (F.o_src) F.o_src[q] = F.src_base + (uint32_t)j;
  }

  // keys: the destination is 8-byte aligned; one key up to its first 16-byte
  // boundary, pairs as one 16-byte store each, one key left over
  uint64_t* ok = F.o_keys + x0;
  const uint64_t kh = std::min<uint64_t>(F.nnz, ((uintptr_t)ok >> 3) & 1);
  const uint64_t pairs = (F.nnz - kh) >> 1;
  if (F.k32) {
    const uint32_t* k = (const uint32_t*)F.keys;
    if (tid == 0 && kh) ok[0] = k[0];
    if (tid == 1 && ((F.nnz - kh) & 1)) ok[F.nnz - 1] = k[F.nnz - 1];
    const bool al = ((uintptr_t)(k + kh) & 7) == 0;
    for (uint64_t g = tid; g < pairs; g += stride) {
      const uint64_t i = kh + 2 * g;
      uint2 v;
      if (al) {
        v = *(const uint2*)(k + i);
      } else {
        v.x = k[i];
        v.y = k[i + 1];
      }
      *(ulonglong2*)(ok + i) = make_ulonglong2(v.x, v.y);
    }
  } else {
    const uint64_t* k = (const uint64_t*)F.keys;
    if (tid == 0 && kh) ok[0] = k[0];
    if (tid == 1 && ((F.nnz - kh) & 1)) ok[F.nnz - 1] = k[F.nnz - 1];
    const bool al = ((uintptr_t)(k + kh) & 15) == 0;
    for (uint64_t g = tid; g < pairs; g += stride) {
      const uint64_t i = kh + 2 * g;
      ulonglong2 v;
      if (al) {
        v = *(const ulonglong2*)(k + i);
      } else {
        v.x = k[i];
        v.y = k[i + 1];
      }
      *(ulonglong2*)(ok + i) = v;
    }
  }

  // access types: the destination has any alignment; bytes up to its first
  // 16-byte boundary, 16 per lane as one store, the bytes left over
  uint8_t* oa = F.o_at + x0;
  const uint64_t ah = std::min<uint64_t>(F.nnz, (16 - ((uintptr_t)oa & 15)) & 15);
  const uint64_t chunks = (F.nnz - ah) >> 4;
  const uint64_t tail0 = ah + 16 * chunks;
  if (tid < ah + (F.nnz - tail0)) {  // at most 30 bytes
    const uint64_t p = tid < ah ? tid : tail0 + (tid - ah);
    oa[p] = F.a2 ? (uint8_t)((F.at[p >> 2] >> (2 * (p & 3))) & 3) : F.at[p];
  }
  if (F.a2) {
    // 16 codes = 32 bits from bit 2p on; p & 3 is that of the head
    const uint32_t sh = 2 * (uint32_t)(ah & 3);
    for (uint64_t g = tid; g < chunks; g += stride) {
      const uint64_t p = ah + 16 * g;
      const uint8_t* sp = F.at + (p >> 2);
      uint64_t v = ((uintptr_t)sp & 3) == 0 ? *(const uint32_t*)sp : wc_bytes4(sp);
      if (sh) v |= (uint64_t)sp[4] << 32;  // the fifth byte exists when the window is shifted
      const uint32_t bits = (uint32_t)(v >> sh);
      *(uint4*)(oa + p) = make_uint4(wc_spread(bits & 0xFFu), wc_spread((bits >> 8) & 0xFFu),
                                     wc_spread((bits >> 16) & 0xFFu), wc_spread(bits >> 24));
    }
  } else {
    const uint32_t mis = (uint32_t)((uintptr_t)(F.at + ah) & 15);
    for (uint64_t g = tid; g < chunks; g += stride) {
      const uint64_t p = ah + 16 * g;
      const uint8_t* sp = F.at + p;
      uint4 w;
      if (mis == 0) {
        w = *(const uint4*)sp;
      } else if ((mis & 3) == 0) {
        const uint32_t* s4 = (const uint32_t*)sp;
        w = make_uint4(s4[0], s4[1], s4[2], s4[3]);
      } else {
        w = make_uint4(wc_bytes4(sp), wc_bytes4(sp + 4), wc_bytes4(sp + 8), wc_bytes4(sp + 12));
      }
      *(uint4*)(oa + p) = w;
    }
  }
}

uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

// the staged outputs of a host call inside wc_out, for room_n txns / room_m accesses
struct HostOut {
  uint64_t *keys, *ts;
  uint32_t *off, *pos, *src;
  uint8_t *rc, *at;
  static uint64_t bytes(uint64_t room_n, uint64_t room_m) {
    return up16(room_m * 8) + up16(room_n * 8) + up16((room_n + 1) * 4) + 2 * up16(room_n * 4) + up16(room_n) +
           up16(room_m) + 64;
  }
  HostOut(void* base, uint64_t room_n, uint64_t room_m) {
    uint8_t* o = (uint8_t*)base;
    keys = (uint64_t*)o;
    o += up16(room_m * 8);
    ts = (uint64_t*)o;
    o += up16(room_n * 8);
    off = (uint32_t*)o;
    o += up16((room_n + 1) * 4);
    pos = (uint32_t*)o;
    o += up16(room_n * 4);
    src = (uint32_t*)o;
    o += up16(room_n * 4);
    rc = o;
    o += up16(room_n);
    at = o;
  }
};

}  // namespace

int dcc_ctx::carry_reserve(uint64_t n, uint64_t nnz) {
  CR(sel_misc.ensure(this, WC_C_WORDS * 8, "select control words"));
  CR(sel_part.ensure(this, ((n + SEL_T - 1) / SEL_T + 1) * 8 + (uint64_t)n_cu * 16 * 4, "select tile pairs"));
  // a host call: the fresh batch in, every output array out (the population
  // and its state go through the staging of the batch and of the WAIT_DIE calls)
  CR(wc_foff.ensure(this, (n + 1) * 4, "carry fresh offsets"));
  CR(wc_fkeys.ensure(this, nnz * 8, "carry fresh keys"));
  CR(wc_fat.ensure(this, nnz + 16, "carry fresh access types"));
  CR(wc_fts.ensure(this, n * 8, "carry fresh timestamps"));
  CR(sel_src.ensure(this, n * 4, "select src"));
  CR(wc_out.ensure(this, HostOut::bytes(n, nnz), "carry outputs"));
  return DCC_OK;
}

int dcc_ctx::waitdie_carry(const dcc_waitdie_carry_args* a, uint64_t* out_n, uint64_t* out_nnz, uint64_t* out_kept,
                           dcc_stats* st) {
  dcc_ctx* ctx = this;
  EpochStats es;
  dcc_stats& S = es.S;
  if (out_n) *out_n = 0;
  if (out_nnz) *out_nnz = 0;
  if (out_kept) *out_kept = 0;
  if (!a || !a->batch || !a->out) return fail(DCC_EINVAL, "waitdie_carry: null args / batch / out");
  if (!a->ts || !a->rc || !a->pos) return fail(DCC_EINVAL, "waitdie_carry: null ts / rc / pos");
  if (!a->out_ts || !a->out_rc || !a->out_pos) return fail(DCC_EINVAL, "waitdie_carry: null out_ts / out_rc / out_pos");
  const dcc_batch* b = a->batch;
  const dcc_batch* f = a->fresh;
  const dcc_select_out* out = a->out;
  if (!out->offsets) return fail(DCC_EINVAL, "waitdie_carry: null out offsets");
  if (out->cap_nnz && (!out->keys || !out->acctype)) return fail(DCC_EINVAL, "waitdie_carry: null out keys/acctype");
  if (out->txn_base || out->nnz_base) return fail(DCC_EINVAL, "waitdie_carry: txn_base and nnz_base must be 0");
  if (f && !a->fresh_ts) return fail(DCC_EINVAL, "waitdie_carry: fresh without fresh_ts");
  if (f && ((f->flags ^ b->flags) & DCC_DEVICE_PTRS))
    return fail(DCC_EINVAL, "waitdie_carry: batch and fresh must agree on DCC_DEVICE_PTRS");
  CR(check_batch(b, false));  // txn length is free here; the offsets are checked on the device
  if (f) CR(check_batch(f, false));
  if (f && f->n_txn == 0) {
    if (f->nnz) return fail(DCC_EINVAL, "waitdie_carry: fresh has accesses and no txn");
    f = nullptr;
  }
  const bool dev = (b->flags & DCC_DEVICE_PTRS) != 0;
  const uint64_t n = b->n_txn, nf = f ? f->n_txn : 0, mf = f ? f->nnz : 0;
  DevBatch d;
  if (n) CR(stage_batch(b, d));  // compact forms are widened here: the gather reads the wide form
  const uint64_t m = d.nnz;
  const uint64_t n_tiles = (n + SEL_T - 1) / SEL_T;
  CR(sel_misc.ensure(this, WC_C_WORDS * 8, "select control words"));
  // the tile pairs, then one revived count per counting workgroup
  const unsigned grid = sel_grid(n_tiles, (unsigned)n_cu * 16);
  CR(sel_part.ensure(this, (n_tiles + 1) * 8 + (uint64_t)grid * 4, "select tile pairs"));
  uint64_t* ctl = (uint64_t*)sel_misc.p;
  uint64_t* part = (uint64_t*)sel_part.p;
  uint32_t* rev_part = (uint32_t*)(part + n_tiles + 1);

  WcArgs A{};
  A.M.n = n;
  A.M.n_tiles = n_tiles;
  A.M.off = d.off;
  A.M.keys = d.keys;
  A.M.at = d.acctype;
  A.M.nnz_base = 0;
  A.M.part = part;
  A.M.err = &ctl[WC_C_ERR];
  A.S.off = d.off;
  const bool w_src = out->src != nullptr;
  if (n) {
    CR(stage(lv_hts, a->ts, n * 8, dev, "waitdie timestamps", A.S.ts));
    CR(stage(lv_hrc, a->rc, n, dev, "waitdie rc", A.S.rc));
    CR(stage(lv_hpos, a->pos, n * 4, dev, "waitdie pos", A.S.pos));
    if (a->revive) CR(stage(lv_hleave, a->revive, n, dev, "waitdie revive", A.S.revive));
    if (a->src_in) CR(stage(sel_src, a->src_in, n * 4, dev, "select src", A.S.src_in));
  }
  WcFresh F{};
  F.n = nf;
  F.nnz = mf;
  F.src_base = a->fresh_src_base;
  F.ctl = ctl;
  if (f) {
    F.k32 = (f->flags & DCC_KEYS_U32) != 0;
    F.a2 = (f->flags & DCC_ACCTYPE_2BIT) != 0;
    const uint8_t* fk = nullptr;
    CR(stage(wc_foff, f->offsets, (nf + 1) * 4, dev, "carry fresh offsets", F.off));
    CR(stage(wc_fts, a->fresh_ts, nf * 8, dev, "carry fresh timestamps", F.ts));
    CR(stage(wc_fkeys, (const uint8_t*)f->keys, mf * (F.k32 ? 4 : 8), dev, "carry fresh keys", fk));
    CR(stage(wc_fat, f->acctype, F.a2 ? (mf + 3) / 4 : mf, dev, "carry fresh access types", F.at));
    F.keys = fk;
  }
  // the most the call can write: the capacities, and no more than both batches hold
  const uint64_t room_n = std::min(out->cap_txn, n + nf), room_m = std::min(out->cap_nnz, m + mf);
  HostOut H(nullptr, 0, 0);
  if (dev) {
    A.M.o_off = out->offsets;
    A.M.o_keys = out->keys;
    A.M.o_at = out->acctype;
    A.S.o_ts = a->out_ts;
    A.S.o_rc = a->out_rc;
    A.S.o_pos = a->out_pos;
    A.S.o_src = out->src;
  } else {
    CR(wc_out.ensure(this, HostOut::bytes(room_n, room_m), "carry outputs"));
    H = HostOut(wc_out.p, room_n, room_m);
    A.M.o_off = H.off;
    A.M.o_keys = H.keys;
    A.M.o_at = H.at;
    A.S.o_ts = H.ts;
    A.S.o_rc = H.rc;
    A.S.o_pos = H.pos;
    A.S.o_src = w_src ? H.src : nullptr;
  }
  F.o_off = A.M.o_off;
  F.o_keys = A.M.o_keys;
  F.o_at = A.M.o_at;
  F.o_ts = A.S.o_ts;
  F.o_rc = A.S.o_rc;
  F.o_pos = A.S.o_pos;
  F.o_src = A.S.o_src;

  const bool prof = profiling;
  CK(hipMemsetAsync(ctl, 0, WC_C_WORDS * 8, stream));
  CK(hipEventRecord(ev0, stream));
  if (prof) CK(hipEventRecord(pev[0], stream));
  k_wc_count<<<grid, SEL_T, 0, stream>>>(d.off, n, m, A.S.rc, A.S.pos, A.S.revive, n_tiles, part, ctl, rev_part);
  if (nf) k_wc_fresh<<<launch_grid(nf, WC_T * 4, (unsigned)n_cu * 8), WC_T, 0, stream>>>(F.off, nf, mf, ctl);
  if (prof) CK(hipEventRecord(pev[1], stream));
  k_wc_scan<<<1, SEL_T, 0, stream>>>(part, n_tiles, out->cap_txn, out->cap_nnz, nf, mf, rev_part, grid, ctl);
  if (prof) CK(hipEventRecord(pev[2], stream));
  k_wc_scatter<<<grid, SEL_T, 0, stream>>>(A);
  if (prof) CK(hipEventRecord(pev[3], stream));
  // 16 type bytes or two keys per lane and step
  if (nf) k_wc_append<<<launch_grid(std::max(nf, mf / 2), WC_T * 4, (unsigned)n_cu * 8), WC_T, 0, stream>>>(F);
  CK(hipGetLastError());
  if (prof) CK(hipEventRecord(pev[4], stream));
  CK(hipEventRecord(ev1, stream));
  CK(hipMemcpyAsync(hmisc, ctl, WC_C_WORDS * 8, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  const uint64_t* hc = (const uint64_t*)hmisc;
  const uint64_t verdict = hc[WC_C_ERR];
  if (verdict & SEL_ERR_OFF) return fail(DCC_EINVAL, "batch: malformed offsets");
  if (verdict & WC_ERR_FOFF) return fail(DCC_EINVAL, "waitdie_carry: malformed offsets of the fresh batch");
  if (verdict & WC_ERR_RC) return fail(DCC_EINVAL, "waitdie_carry: an rc byte outside the five states");
  if (verdict & WC_ERR_POS) return fail(DCC_EINVAL, "waitdie_carry: pos does not fit its txn's state");
  if (verdict & WC_ERR_REVIVE) return fail(DCC_EINVAL, "waitdie_carry: revive set on a txn that is not GONE");
  const uint64_t ns = hc[WC_C_TOTAL] & 0xFFFFFFFFull, ms = hc[WC_C_TOTAL] >> 32;
  const uint64_t nt = ns + nf, mt = ms + mf;
  if (out_n) *out_n = nt;
  if (out_nnz) *out_nnz = mt;
  if (out_kept) *out_kept = ns;
  S.n_commit = ns;
  S.n_abort = n - ns;
  S.n_survivors = hc[WC_C_REVIVED];
  if (verdict & SEL_ERR_CAP) {
    if (st) *st = S;
    return fail(DCC_ERANGE, "waitdie_carry: %llu txns / %llu accesses (%llu stayers), room for %llu / %llu",
                (unsigned long long)nt, (unsigned long long)mt, (unsigned long long)ns,
                (unsigned long long)out->cap_txn, (unsigned long long)out->cap_nnz);
  }
  if (!dev) {
    CK(hipMemcpyAsync(out->offsets, H.off, (nt + 1) * 4, hipMemcpyDeviceToHost, stream));
    if (mt) {
      CK(hipMemcpyAsync(out->keys, H.keys, mt * 8, hipMemcpyDeviceToHost, stream));
      CK(hipMemcpyAsync(out->acctype, H.at, mt, hipMemcpyDeviceToHost, stream));
    }
    if (nt) {
      CK(hipMemcpyAsync(a->out_ts, H.ts, nt * 8, hipMemcpyDeviceToHost, stream));
      CK(hipMemcpyAsync(a->out_rc, H.rc, nt, hipMemcpyDeviceToHost, stream));
      CK(hipMemcpyAsync(a->out_pos, H.pos, nt * 4, hipMemcpyDeviceToHost, stream));
      if (w_src) CK(hipMemcpyAsync(out->src, H.src, nt * 4, hipMemcpyDeviceToHost, stream));
    }
    CK(hipStreamSynchronize(stream));
  }
  S.alg_bytes = dcc_waitdie_carry_alg_bytes(n, ns, ms, nf, mf, a->revive != nullptr, w_src);
  CR(es.finish(this, 4));
  if (st) *st = S;
  return DCC_OK;
}

extern "C" uint64_t dcc_waitdie_carry_alg_bytes(uint64_t n_txn, uint64_t n_kept, uint64_t nnz_kept, uint64_t n_fresh,
                                                uint64_t nnz_fresh, int with_revive, int with_src) {
  // offsets, rc (and revive) of the input read; per stayer ts and pos read,
  // ts, rc, pos written; (key, type) of every access read and written; the
  // fresh offsets and ts read, their ts, rc, pos written; the output offsets
  return 4 * (n_txn + 1) + n_txn * (1 + (with_revive ? 1u : 0u)) + 25 * n_kept + 18 * nnz_kept +
         4 * (n_fresh + 1) + 8 * n_fresh + 13 * n_fresh + 18 * nnz_fresh + 4 * (n_kept + n_fresh + 1) +
         (with_src ? 8 * n_kept + 4 * n_fresh : 0);
}

extern "C" int dcc_waitdie_carry(dcc_ctx* ctx, const dcc_waitdie_carry_args* a, uint64_t* out_n, uint64_t* out_nnz,
                                 uint64_t* out_kept, dcc_stats* out_stats) {
  if (!ctx) return DCC_EINVAL;
  if (a && (((a->batch ? a->batch->flags : 0u) | (a->fresh ? a->fresh->flags : 0u)) &
            (DCC_ISO_READ_COMMITTED | DCC_ISO_READ_UNCOMMITTED)))
    return ctx->fail(DCC_ENOTSUP, "waitdie: an isolation level below SERIALIZABLE");
  dcc_pipe_drain(ctx);  // pipelined OCC epochs in flight complete first
  // a local data movement: rank 0's GPU, its communicator left alone
  return dcc_on_device(ctx, false,
                       [&](dcc_ctx* s) { return s->waitdie_carry(a, out_n, out_nnz, out_kept, out_stats); });
}
