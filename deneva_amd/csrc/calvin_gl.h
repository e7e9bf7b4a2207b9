// The one-word grant-group scan state shared by the Calvin kernels
// (calvin.hip's global scan, calvin_bucket.hip's per-bucket scan).
//
// Over requests sorted by (row, sequence position), the grant group of a
// request is the number of group boundaries before it on its row, where two
// consecutive requests of a row are in different groups iff either is EX
// (row_lock.cpp:78-81, 152-170: an SH run shares the lock, every EX is alone).
// State of an interval: segment start (bit 0: the interval holds a row's first
// request), first and last lock type of its requests (2 bits each: SH, EX,
// NONE) and the boundaries since the segment's start (27 bits).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcc_scan.h"

namespace dcc {

constexpr uint32_t CV_SH = 0, CV_EX = 1, CV_NONE = 2;

__host__ __device__ constexpr uint32_t gl_pack(uint32_t flag, uint32_t ft, uint32_t lt, uint32_t cnt) {
  return flag | (ft << 1) | (lt << 3) | (cnt << 5);
}
constexpr uint32_t GL_ID = gl_pack(0, CV_NONE, CV_NONE, 0);

__device__ inline uint32_t gl_combine(uint32_t A, uint32_t B) {
  if (B & 1u) return B;
  const uint32_t aft = (A >> 1) & 3u, alt = (A >> 3) & 3u, bft = (B >> 1) & 3u, blt = (B >> 3) & 3u;
  const bool bnd = alt != CV_NONE && bft != CV_NONE && (alt == CV_EX || bft == CV_EX);
  const uint32_t ft = aft != CV_NONE ? aft : bft;
  const uint32_t lt = blt != CV_NONE ? blt : alt;
  return (A & 1u) | (ft << 1) | (lt << 3) | (((A >> 5) + (B >> 5) + (bnd ? 1u : 0u)) << 5);
}

// the state as a scan operator (dcc_scan.h); not commutative, so it has no
// shfl_xor and the butterfly reductions do not take it
struct GlOp {
  using T = uint32_t;
  static constexpr bool has_inverse = false;
  __device__ static uint32_t identity() { return GL_ID; }
  __device__ static uint32_t combine(uint32_t a, uint32_t b) { return gl_combine(a, b); }
  __device__ static uint32_t shfl_up(uint32_t v, uint32_t d) { return __shfl_up(v, d); }
};

}  // namespace dcc
