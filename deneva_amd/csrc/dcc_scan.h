// Wave and workgroup scans / reductions shared by the gfx950 kernels: the
// only place the shuffle loops are written.
//
// An operator is a type with
//   T                 the element type
//   identity()
//   combine(a, b)     a is the EARLIER element (lower lane, lower wave).  GlOp
//                     (calvin_gl.h) and MsOp (maat.hip) are not commutative:
//                     every template below keeps combine(earlier, later)
//   shfl_up(v, d)     the element of lane - d (scans)
//   shfl_xor(v, d)    the element of lane ^ d (wave_reduce / block_reduce;
//                     commutative operators only, the others do not have it)
//   has_inverse       the exclusive prefix is incl - v (sums) instead of one
//                     more shuffle
// Two u32 sums that go together (k_fin's commits and writes) are scanned as
// one u64, low and high word: one loop, both shuffles of a step back to back.
//
// Barrier contract of block_excl / block_reduce (s_w: one LDS element per
// wave, the caller's, so no kernel's LDS size depends on them):
//   on entry   no wave still reads s_w from an earlier use.  True for the
//              first use in a kernel; a caller that reuses s_w (a loop, two
//              scans in a row) puts a barrier before the call;
//   inside     exactly one barrier, between the waves' writes of their
//              totals and every thread's reads of them;
//   on return  the other waves may still be reading s_w: the caller puts a
//              barrier before anything writes s_w again.
// The *_reuse forms are the same behind that entry barrier, for a call in a
// loop or straight after another scan through the same s_w.
// Sync chooses that barrier: SyncThreads (__syncthreads()) or SyncLds
// (lds_barrier(), for kernels that keep global loads in flight across it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcc_device.h"

namespace dcc {

template <typename V>
struct ScalarOp {
  using T = V;
  static constexpr bool has_inverse = false;
  __device__ static T shfl_up(T v, uint32_t d) { return (T)__shfl_up(v, d); }
  __device__ static T shfl_xor(T v, uint32_t d) { return (T)__shfl_xor(v, d); }
};
template <typename V>
struct AddOp : ScalarOp<V> {
  static constexpr bool has_inverse = true;
  __device__ static V identity() { return 0; }
  __device__ static V combine(V a, V b) { return a + b; }
  __device__ static V remove(V incl, V v) { return incl - v; }
};
template <typename V>
struct MaxOp : ScalarOp<V> {
  __device__ static V identity() { return 0; }
  __device__ static V combine(V a, V b) { return max(a, b); }
};
template <typename V>
struct OrOp : ScalarOp<V> {
  __device__ static V identity() { return 0; }
  __device__ static V combine(V a, V b) { return a | b; }
};
template <typename V>
struct AndOp : ScalarOp<V> {
  __device__ static V identity() { return ~(V)0; }
  __device__ static V combine(V a, V b) { return a & b; }
};
struct SyncThreads {
  __device__ static void sync() { __syncthreads(); }
};
struct SyncLds {
  __device__ static void sync() { lds_barrier(); }
};

// ------------------------------------------------------------------- wave
// xor butterfly: every lane gets the wave's result
template <typename Op>
__device__ inline typename Op::T wave_reduce(typename Op::T v) {
#pragma unroll
  for (uint32_t d = 32; d > 0; d >>= 1) v = Op::combine(v, Op::shfl_xor(v, d));
  return v;
}
// inclusive scan (Hillis-Steele): lane l gets v_0 (x) ... (x) v_l
template <typename Op>
__device__ inline typename Op::T wave_incl(typename Op::T x) {
  const uint32_t lane = lane_id();
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const typename Op::T y = Op::shfl_up(x, d);
    if (lane >= d) x = Op::combine(y, x);
  }
  return x;
}
// lane l's exclusive prefix v_0 (x) ... (x) v_{l-1}, from its inclusive one
template <typename Op>
__device__ inline typename Op::T excl_of_incl(typename Op::T incl, typename Op::T v) {
  if constexpr (Op::has_inverse) {
    return Op::remove(incl, v);
  } else {
    const typename Op::T up = Op::shfl_up(incl, 1);
    return lane_id() ? up : Op::identity();
  }
}
// exclusive scan; total: the wave's, in every lane (scalar elements)
template <typename Op>
__device__ inline typename Op::T wave_excl(typename Op::T v, typename Op::T& total) {
  const typename Op::T x = wave_incl<Op>(v);
  total = __shfl(x, 63);
  return excl_of_incl<Op>(x, v);
}

// ------------------------------------------------------------------ block
// Exclusive scan over the workgroup's threads in thread order, and the
// workgroup's total; nw waves (blockDim.x / 64).  Barriers: see the top.
template <typename Op, typename Sync = SyncThreads>
__device__ inline typename Op::T block_excl(typename Op::T v, typename Op::T* s_w, uint32_t nw,
                                            typename Op::T& total) {
  using T = typename Op::T;
  const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
  const T x = wave_incl<Op>(v);
  if (lane == 63) s_w[w] = x;
  Sync::sync();
  T wp = Op::identity();
  total = Op::identity();
  for (uint32_t q = 0; q < nw; q++) {
    const T s = s_w[q];
    if (q < w) wp = Op::combine(wp, s);
    total = Op::combine(total, s);
  }
  return Op::combine(wp, excl_of_incl<Op>(x, v));
}
// the same with a compile-time wave count (the loop over the waves unrolls)
template <uint32_t NW, typename Op, typename Sync = SyncThreads>
__device__ inline typename Op::T block_excl(typename Op::T v, typename Op::T* s_w,
                                            typename Op::T& total) {
  return block_excl<Op, Sync>(v, s_w, NW, total);
}

template <typename Op, typename Sync = SyncThreads>
__device__ inline typename Op::T block_excl_reuse(typename Op::T v, typename Op::T* s_w, uint32_t nw,
                                                  typename Op::T& total) {
  Sync::sync();
  return block_excl<Op, Sync>(v, s_w, nw, total);
}
template <uint32_t NW, typename Op, typename Sync = SyncThreads>
__device__ inline typename Op::T block_excl_reuse(typename Op::T v, typename Op::T* s_w,
                                                  typename Op::T& total) {
  return block_excl_reuse<Op, Sync>(v, s_w, NW, total);
}

// Reduction over the workgroup with a commutative operator: every thread gets
// the result.  (A non-commutative one takes block_excl's total.)
template <typename Op, typename Sync = SyncThreads>
__device__ inline typename Op::T block_reduce(typename Op::T v, typename Op::T* s_w, uint32_t nw) {
  using T = typename Op::T;
  v = wave_reduce<Op>(v);
  if (lane_id() == 0) s_w[threadIdx.x >> 6] = v;
  Sync::sync();
  T t = Op::identity();
  for (uint32_t q = 0; q < nw; q++) t = Op::combine(t, s_w[q]);
  return t;
}
template <uint32_t NW, typename Op, typename Sync = SyncThreads>
__device__ inline typename Op::T block_reduce(typename Op::T v, typename Op::T* s_w) {
  return block_reduce<Op, Sync>(v, s_w, NW);
}

template <typename Op, typename Sync = SyncThreads>
__device__ inline typename Op::T block_reduce_reuse(typename Op::T v, typename Op::T* s_w,
                                                    uint32_t nw) {
  Sync::sync();
  return block_reduce<Op, Sync>(v, s_w, nw);
}

// One atomic per workgroup (NW waves) for a per-thread count.  The one
// template here with LDS words of its own (NW, per kernel that calls it): a
// second call in a kernel comes behind a barrier.
template <uint32_t NW>
__device__ inline void block_add(uint32_t c, uint32_t* ctr) {
  __shared__ uint32_t s_c[NW];
  const uint32_t v = block_reduce<NW, AddOp<uint32_t>>(c, s_c);
  if (threadIdx.x == 0 && v) atomicAdd(ctr, v);
}

}  // namespace dcc
