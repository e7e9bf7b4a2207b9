// The skeleton that the engines with txns in flight share: WAIT_DIE
// (waitdie.hip) and the in-flight MVCC calls (mvcc_live.hip); DESIGN.md §8s.
// Both keep the caller's state in two per-txn arrays (rc, pos), decide the RUN
// txns in an epoch (the fixed point of seg_rounds.h) and take the txns the
// caller names away in a second call that promotes waiters.  What both run
// unchanged is written once here: the state's rule, the txn word, the check,
// the epoch's prep / advance / final kernels, the leavers' pass and the host
// side up to ev0.  What differs is an engine type E:
//
//   E::T          threads per workgroup of the engine's kernels
//   E::name       the engine, for messages
//   E::TS_RANGE   a ts of 0 or UINT64_MAX is rejected (MVCC: they are its
//                 "none" values)
//   E::WAIT_STAYS a WAIT txn that leaves is rejected (MVCC)
//   E::ROW_BIT    the second call's sort key holds a bit below the packed row,
//                 as the epoch's does, so that 64 varying key bits are too many
//   E::ABORT_POS  an aborted txn's pos becomes its stop (MVCC; WAIT_DIE leaves it)
//   E::record     an access of the epoch: the record word above the position,
//                 whether it is dynamic and whether it is a counted request
//   E::STOP, E::CERTAIN  the bits of a dynamic access's flag byte (four
//                 bits) that make it a possible stop / a certain stop
//   E::verdict    the flag byte of a txn's first possible stop as LS_ABORT,
//                 LS_WAIT or LS_UND
//
// Elements, operators, the sorted records and every scan stay the engine's.
// The state rule alone is also what waitdie_carry.hip's counting pass applies.
#pragma once
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

namespace dcc {
namespace {

// ----------------------------------------------------------- state rule
// rc is one of the five states; pos fits it: never past len, at len for RCOK,
// below it for WAIT (the access waited at); a GONE txn's pos is free.
__device__ inline bool live_state_ok(uint8_t rc) {
  return rc == DCC_WD_RUN || rc == DCC_RC_RCOK || rc == DCC_RC_WAIT || rc == DCC_RC_ABORT || rc == DCC_WD_GONE;
}
__device__ inline bool live_pos_ok(uint8_t rc, uint32_t pos, uint32_t len) {
  return rc == DCC_WD_GONE || !(pos > len || (rc == DCC_RC_RCOK && pos != len) || (rc == DCC_RC_WAIT && pos >= len));
}

// error bits next to CHK_ERR_* (4 is tso_kernels.h's full row table, 8 its and
// this file's inconsistent decisions)
constexpr uint32_t LV_ERR_STATE = 8, LV_ERR_TS = 16, LV_ERR_RC = 32, LV_ERR_POS = 64, LV_ERR_LEAVE = 128;
// counter words next to SEG_C_*: requests of the counted type, RUN txns
// without one, RCOK / aborted / waiting txns of an epoch.  Words 5 and 6 are
// k_ts_seed's (heads, rows), 12 and 13 the engine's.  The second call has no
// rounds and keeps its words in the ring: the timestamp bits that vary (u64
// each, stored only with `leave`), the leavers that were not GONE, a word of
// the engine's, the promoted txns
constexpr uint32_t LV_C_NREQ = 2, LV_C_RO = 3, LV_C_OK = 4, LV_C_ABORT = 7, LV_C_WAIT = 14, LV_C_RING = 16,
                   LV_C_TOR = LV_C_RING, LV_C_TNOR = LV_C_RING + 2, LV_C_LEFT = LV_C_RING + 4,
                   LV_C_ENGINE = LV_C_RING + 5, LV_C_PROM = LV_C_RING + 6, LV_C_WORDS = LV_C_RING + SEG_RING;
static_assert(LV_C_WORDS <= SegWork::C_WORDS && LV_C_PROM < LV_C_WORDS, "the shared workspace's counter words");
// a word below the ring that neither seg_rounds.h nor this file uses: an engine's own lie there
constexpr bool lv_word_free(uint32_t w) {
  return w > SEG_C_MAXLEN && w < LV_C_RING && (w < SEG_C_KOR || w > SEG_C_KNOR + 1) && w != LV_C_NREQ &&
         w != LV_C_RO && w != LV_C_OK && w != LV_C_ABORT && w != LV_C_WAIT;
}

// txn word: state << 16 | cap << 8 | progress.  cap: the first access at or
// past the progress of an undecided txn with a certain stop (LS_NOCAP: none
// known): it passes nothing from there on and waits there at the latest
constexpr uint32_t LS_UND = 0, LS_OK = 1, LS_WAIT = 2, LS_ABORT = 3, LS_STATIC = 4, LS_NOCAP = 0xFFu;
__host__ __device__ constexpr uint32_t ls_word(uint32_t state, uint32_t cap, uint32_t prog) {
  return (state << 16) | (cap << 8) | prog;
}
__device__ inline uint32_t ls_state(uint32_t w) { return w >> 16; }
__device__ inline uint32_t ls_cap(uint32_t w) { return (w >> 8) & 0xFFu; }
__device__ inline uint32_t ls_prog(uint32_t w) { return w & 0xFFu; }

struct LiveArgs {
  uint64_t n, m;
  const uint32_t* off;
  const uint64_t* keys;
  const uint8_t* at;
  const uint64_t* ts;
  uint8_t* rc;       // the state, updated in place behind the decisions
  uint32_t* pos;
  uint32_t lp;       // log2 lanes per txn
  uint4* arec;       // [m] {txn, record word, ts lo, ts hi} of every access
  uint32_t* stp;     // [n] txn words
  uint8_t* flg;      // [m] flag byte of every dynamic access, batch order
  uint32_t* cnt;
};

// ---------------------------------------------------------------- check
// The batch's and the state's validity before anything indexes with them and
// before anything is written; the key bits that vary; the RUN txns (epoch,
// `leave` null: the ring word round 1 reads) or, for the second call, the
// leavers that were not GONE and the timestamp bits that vary.
template <class E>
__global__ __launch_bounds__(E::T) void k_live_check(const uint32_t* __restrict__ off, uint64_t n,
                                                     const uint64_t* __restrict__ keys, uint64_t nnz,
                                                     const uint64_t* __restrict__ ts,
                                                     const uint8_t* __restrict__ rc,
                                                     const uint32_t* __restrict__ pos,
                                                     const uint8_t* __restrict__ leave, uint32_t* __restrict__ cnt) {
  constexpr uint32_t T = E::T;
  __shared__ uint64_t s_a[T / 64], s_b[T / 64], s_e[T / 64], s_f[T / 64];
  __shared__ uint32_t s_c[T / 64], s_d[T / 64];
  uint32_t len = 0, err = 0, count = 0;
  uint64_t kor = 0, knor = 0, tor = 0, tnor = 0;
  const uint64_t tid = (uint64_t)blockIdx.x * T + threadIdx.x, stride = (uint64_t)gridDim.x * T;
  for (uint64_t t = tid; t < n; t += stride) {
    uint32_t l;
    if (!check_span(off, t, n, nnz, err, len, l)) continue;
    const uint8_t r = rc[t];
    const uint32_t p = pos[t];
    const uint64_t v = ts[t];
    if (!live_state_ok(r)) err |= LV_ERR_RC;
    else if (!live_pos_ok(r, p, l)) err |= LV_ERR_POS;
    if (E::TS_RANGE && r != DCC_WD_GONE && (v == 0 || v == ~0ull)) err |= LV_ERR_TS;
    if (E::WAIT_STAYS && leave && leave[t] != 0 && r == DCC_RC_WAIT) err |= LV_ERR_LEAVE;
    tor |= v;
    tnor |= ~v;
    count += leave ? (leave[t] != 0 && r != DCC_WD_GONE) : (r == DCC_WD_RUN);
  }
  for (uint64_t x = tid; x < nnz; x += stride) check_key(keys[x], err, kor, knor);
  kor = block_reduce<T / 64, OrOp<uint64_t>>(kor, s_a);
  knor = block_reduce<T / 64, OrOp<uint64_t>>(knor, s_b);
  tor = block_reduce<T / 64, OrOp<uint64_t>>(tor, s_e);
  tnor = block_reduce<T / 64, OrOp<uint64_t>>(tnor, s_f);
  len = block_reduce<T / 64, MaxOp<uint32_t>>(len, s_c);
  err = block_reduce<T / 64, OrOp<uint32_t>>(err, s_d);
  if (threadIdx.x == 0) {
    if (kor) atomicOr((unsigned long long*)&cnt[SEG_C_KOR], (unsigned long long)kor);
    if (knor) atomicOr((unsigned long long*)&cnt[SEG_C_KNOR], (unsigned long long)knor);
    if (leave && tor) atomicOr((unsigned long long*)&cnt[LV_C_TOR], (unsigned long long)tor);
    if (leave && tnor) atomicOr((unsigned long long*)&cnt[LV_C_TNOR], (unsigned long long)tnor);
    if (len) atomicMax(&cnt[SEG_C_MAXLEN], len);
    if (err) atomicOr(&cnt[SEG_C_ERR], err);
  }
  block_add<T / 64>(count, leave ? &cnt[LV_C_LEFT] : &cnt[LV_C_RING + 1]);
}

// ---------------------------------------------------------------- epoch
// P lanes per txn (nowait_lanes.h): the sort key (packed row, dynamic) and the
// record of every access; a RUN txn undecided at progress pos; the requests of
// the counted type and the RUN txns without one counted.
template <class E>
__global__ __launch_bounds__(E::T) void k_live_prep(LiveArgs A, KeyPack kp, uint64_t* __restrict__ ak,
                                                    uint32_t* __restrict__ av) {
  const Seg g = seg_of(A.lp);
  const uint32_t gpb = E::T >> A.lp;
  uint32_t ro = 0, nreq = 0;
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
    bool req = false;
    if (v) {
      bool dyn;
      const uint32_t rec = E::record(r, p, g.a, A.at[x] & 3u, dyn, req);
      ak[x] = (keypack_apply(kp, A.keys[x]) << 1) | (dyn ? 1ull : 0ull);
      av[x] = (uint32_t)x;
      A.arec[x] = make_uint4((uint32_t)t, g.a | rec, (uint32_t)tsv, (uint32_t)(tsv >> 32));
    }
    const uint64_t rb = ballot64(req) & g.mask;
    if (tv && g.a == 0) {
      A.stp[t] = run ? ls_word(LS_UND, LS_NOCAP, p) : ls_word(LS_STATIC, 0, 0);
      if (run) {
        ro += rb ? 0u : 1u;
        nreq += (uint32_t)__popcll(rb);
      }
    }
  }
  block_add<E::T / 64>(ro, &A.cnt[LV_C_RO]);
  __syncthreads();  // block_add's LDS words are read before the next call writes them
  block_add<E::T / 64>(nreq, &A.cnt[LV_C_NREQ]);
}

// One round of decisions.  P lanes per txn, one access per lane: the first
// access at or past the progress with a possible stop is where the txn aborts,
// waits or stays undecided.  Counts the txns it leaves undecided.
template <class E>
__global__ __launch_bounds__(E::T) void k_live_advance(LiveArgs A, const uint32_t* __restrict__ left,
                                                       uint32_t* left_out) {
  if (*left == 0) return;
  const Seg g = seg_of(A.lp);
  const uint32_t gpb = E::T >> A.lp;
  uint32_t und_left = 0;
  for (uint64_t g0 = (uint64_t)blockIdx.x * gpb; g0 < A.n; g0 += (uint64_t)gridDim.x * gpb) {
    const uint64_t t = g0 + g.gl;
    const bool tv = t < A.n;
    const uint32_t st = tv ? A.stp[t] : ls_word(LS_STATIC, 0, 0);
    const bool und = tv && ls_state(st) == LS_UND;
    if (!ballot64(und)) continue;  // the wave's txns are decided
    uint32_t o0 = 0, len = 0;
    if (und) {
      o0 = A.off[t];
      len = A.off[t + 1] - o0;
    }
    const bool v = und && g.a < len && g.a >= ls_prog(st);
    const uint32_t f = v ? A.flg[(uint64_t)o0 + g.a] : 0u;
    // one ballot per flag bit, so that the leader lane (g.a == 0) can read any
    // lane's byte: bit l of b[k] is bit k of the byte that lane l loaded.  A
    // b[k] that neither the engine's masks nor its verdict use folds away
    const uint64_t b[4] = {ballot64((f & 1u) != 0), ballot64((f & 2u) != 0), ballot64((f & 4u) != 0),
                           ballot64((f & 8u) != 0)};
    const auto any = [&](uint32_t bits) {
      uint64_t r = 0;
      for (uint32_t k = 0; k < 4; k++) r |= ((bits >> k) & 1u) ? b[k] : 0ull;
      return r;
    };
    const uint64_t sb = any(E::STOP) & g.mask;
    if (und && g.a == 0) {
      uint32_t w;
      if (!sb) {
        w = ls_word(LS_OK, 0, len);
      } else {
        const uint32_t l = (uint32_t)__builtin_ctzll(sb);
        // the verdict sees exactly the four bits that the lane at l, the first possible stop, loaded
        const uint32_t s = E::verdict((uint32_t)(((b[0] >> l) & 1ull) | (((b[1] >> l) & 1ull) << 1) |
                                                 (((b[2] >> l) & 1ull) << 2) | (((b[3] >> l) & 1ull) << 3)));
        const uint64_t cf = any(E::CERTAIN) & g.mask;  // certain stops at or past the progress: they stay certain
        w = ls_word(s, cf ? (uint32_t)__builtin_ctzll(cf) - g.seg0 : LS_NOCAP, l - g.seg0);
        und_left += s == LS_UND ? 1u : 0u;
      }
      A.stp[t] = w;
    }
  }
  block_add<E::T / 64>(und_left, left_out);
}

// The new state of the RUN txns: (RCOK, len), (WAIT, stop) or (ABORT, stop --
// the input pos without E::ABORT_POS); the conflict ordinals; the counts.
template <class E>
__global__ __launch_bounds__(E::T) void k_live_final(uint64_t n, const uint32_t* __restrict__ stp,
                                                     uint8_t* __restrict__ rc, uint32_t* __restrict__ pos,
                                                     uint32_t* __restrict__ conflict, uint32_t* __restrict__ cnt) {
  uint32_t ok = 0, ab = 0, wait = 0, bad = 0;
  for (uint64_t t = (uint64_t)blockIdx.x * E::T + threadIdx.x; t < n; t += (uint64_t)gridDim.x * E::T) {
    const uint32_t st = stp[t], s = ls_state(st), p = ls_prog(st);
    uint32_t c = DCC_ACCESS_NONE;
    if (s == LS_OK) {
      rc[t] = DCC_RC_RCOK;
      pos[t] = p;
      ok++;
    } else if (s == LS_WAIT || s == LS_ABORT) {
      rc[t] = s == LS_WAIT ? DCC_RC_WAIT : DCC_RC_ABORT;
      if (E::ABORT_POS || s == LS_WAIT) pos[t] = p;
      c = p;
      wait += s == LS_WAIT;
      ab += s == LS_ABORT;
    } else if (s == LS_UND) {
      bad = 1;
    }
    if (conflict) conflict[t] = c;
  }
  if (bad) atomicOr(&cnt[SEG_C_ERR], LV_ERR_STATE);
  block_add<E::T / 64>(ok, &cnt[LV_C_OK]);
  __syncthreads();
  block_add<E::T / 64>(ab, &cnt[LV_C_ABORT]);
  __syncthreads();
  block_add<E::T / 64>(wait, &cnt[LV_C_WAIT]);
}

// The leavers become GONE; nothing if the error word (null: none) is set.
template <class E>
__global__ __launch_bounds__(E::T) void k_live_gone(uint64_t n, const uint8_t* __restrict__ leave,
                                                    uint8_t* __restrict__ rc, const uint32_t* __restrict__ err) {
  if (err && *err) return;
  for (uint64_t t = (uint64_t)blockIdx.x * E::T + threadIdx.x; t < n; t += (uint64_t)gridDim.x * E::T)
    if (leave[t]) rc[t] = DCC_WD_GONE;
}

// ------------------------------------------------------------------ host
// What an epoch and the second call (`second`: a release, a finish) share up
// to ev0: the stats' clock, the call's arguments checked, the batch and the
// state arrays on the device, the check and its rejections, the key pack and
// the lanes' geometry.  A.n == 0 behind a DCC_OK: the empty batch.
struct LiveOpen {
  EpochStats es;
  uint64_t per_block = 0, tiles = 0, tvar = 0;  // tvar: the timestamp bits that vary (second call)
  uint32_t count = 0;                           // the RUN txns, or the leavers that were not GONE
  bool dev = false;
  const uint8_t* leave_dev = nullptr;
  unsigned max_grid = 1;
  BatchShape c;
  KeyPack kp{};
  LiveArgs A{};  // rc, pos, cnt: the state and the counters on the device
};
template <class E>
int live_open(dcc_ctx* ctx, const dcc_batch* b, const uint64_t* ts_in, uint8_t* rc_io, uint32_t* pos_io, bool second,
              const uint8_t* leave_in, uint64_t* out_left, uint64_t* out_promoted, LiveOpen& O) {
  hipStream_t stream = ctx->stream;
  if (!ts_in || !rc_io || !pos_io) return ctx->fail(DCC_EINVAL, "%s: null ts / rc / pos", E::name);
  if (second && !leave_in) return ctx->fail(DCC_EINVAL, "%s: null leave", E::name);
  CR(ctx->check_batch(b, false));  // the offsets are checked on the device (k_live_check)
  if (ctx->comm_ranks() > 1) return ctx->fail(DCC_ENOTSUP, "%s: single-GPU engine", E::name);
  O.dev = (b->flags & DCC_DEVICE_PTRS) != 0;
  if (out_left) *out_left = 0;
  if (out_promoted) *out_promoted = 0;
  if (b->n_txn == 0) return DCC_OK;
  DevBatch d;
  CR(ctx->stage_batch(b, d));
  const uint64_t n = d.n, m = d.nnz;
  CR(ctx->live_reserve(n, m, !O.dev));
  const uint64_t* ts_dev;
  uint8_t* rc_dev;
  uint32_t* pos_dev;
  CR(ctx->live_stage(n, O.dev, ts_in, rc_io, pos_io, leave_in, ts_dev, rc_dev, pos_dev, O.leave_dev));
  SegWork& W = ctx->seg;
  uint32_t* cnt = (uint32_t*)W.misc.p;
  O.max_grid = (unsigned)ctx->n_cu * 16;

  // reject a malformed batch or state before anything indexes with it: rc,
  // pos, the outputs and whatever the engine keeps are untouched by a rejected
  // call.  All of the workspace's counter words are cleared, the engine's own
  // behind the ring among them
  CK(hipMemsetAsync(cnt, 0, SegWork::C_WORDS * 4, stream));
  k_live_check<E><<<launch_grid(std::max(n, m), E::T * 4, O.max_grid), E::T, 0, stream>>>(
      d.off, n, d.keys, m, ts_dev, rc_dev, pos_dev, O.leave_dev, cnt);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(ctx->hmisc, cnt, SegWork::C_WORDS * 4, hipMemcpyDeviceToHost, stream));
  CK(hipStreamSynchronize(stream));
  const uint32_t* hc = (const uint32_t*)ctx->hmisc;
  const uint32_t err = hc[SEG_C_ERR];
  CR(batch_checked(ctx, hc, m, true, O.c));
  if (err & LV_ERR_RC) return ctx->fail(DCC_EINVAL, "%s: an rc byte is none of the five states", E::name);
  if (err & LV_ERR_POS)
    return ctx->fail(DCC_EINVAL, "%s: a pos does not fit its state (pos > len, RCOK below len, WAIT at len)", E::name);
  if (err & LV_ERR_TS) return ctx->fail(DCC_EINVAL, "%s: a timestamp is 0 or UINT64_MAX", E::name);
  if (err & LV_ERR_LEAVE) return ctx->fail(DCC_EINVAL, "%s: a WAIT txn cannot leave", E::name);
  if (second) {
    uint64_t a, o;
    memcpy(&a, hc + LV_C_TOR, 8);
    memcpy(&o, hc + LV_C_TNOR, 8);
    O.tvar = a & o;
  }
  O.count = hc[second ? LV_C_LEFT : LV_C_RING + 1];
  O.kp = make_keypack(O.c.varying);
  if ((!second || E::ROW_BIT) && O.kp.bits > 63)
    return ctx->fail(DCC_ENOTSUP, "%s: the keys vary in all 64 bits", E::name);
  O.per_block = E::T >> O.c.lp;
  O.tiles = (m + SegWork::TILE - 1) / SegWork::TILE;
  O.A = LiveArgs{n,      m,  d.off, d.keys, d.acctype, ts_dev, rc_dev, pos_dev,
                 O.c.lp, (uint4*)W.arec.p, (uint32_t*)W.stp.p, (uint8_t*)ctx->lv_flg.p, cnt};
  return DCC_OK;
}

// The second call's two stable sorts: `prep(keys, values)` writes the first
// key of every access, its txn's packed ts; behind that sort `key(values,
// keys)` writes the second, the packed row, in the order the first left.  The
// sorted keys and access indices come back in sk / sv.
template <class Prep, class Key>
int live_sort_ts_row(dcc_ctx* ctx, uint64_t m, uint32_t ts_bits, uint32_t row_bits, Prep prep, Key key,
                     const uint64_t*& sk, const uint32_t*& sv) {
  SegWork& W = ctx->seg;
  uint64_t* kb[2] = {(uint64_t*)W.k[0].p, (uint64_t*)W.k[1].p};
  uint32_t* vb[2] = {(uint32_t*)W.v[0].p, (uint32_t*)W.v[1].p};
  prep(kb[0], vb[0]);
  CK(hipGetLastError());
  const int c1 = radix_sort_u64(kb, vb, m, ts_bits, (uint32_t*)ctx->cv_scratch.p, ctx->stream);
  uint64_t* kb2[2] = {kb[c1], kb[c1 ^ 1]};
  uint32_t* vb2[2] = {vb[c1], vb[c1 ^ 1]};
  key(vb2[0], kb2[0]);
  CK(hipGetLastError());
  const int c2 = radix_sort_u64(kb2, vb2, m, row_bits, (uint32_t*)ctx->cv_scratch.p, ctx->stream);
  sk = kb2[c2];
  sv = vb2[c2];
  return DCC_OK;
}

// A host call's state, and its conflict ordinals if wanted, copied back from
// the staged arrays; the caller synchronises.
inline int live_copy_back(dcc_ctx* ctx, const LiveOpen& O, uint8_t* rc_io, uint32_t* pos_io,
                          uint32_t* out_conflict = nullptr) {
  if (O.dev) return DCC_OK;
  const uint64_t n = O.A.n;
  CK(hipMemcpyAsync(rc_io, O.A.rc, n, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipMemcpyAsync(pos_io, O.A.pos, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_conflict) CK(hipMemcpyAsync(out_conflict, ctx->lv_conf.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  return DCC_OK;
}

}  // namespace
}  // namespace dcc
