// The lane layout of the NO_WAIT kernels (nowait.hip, locktab.hip): a txn takes
// P = 2^lp consecutive lanes of a wave, one access per lane, so adjacent lanes
// load adjacent accesses and per-txn reductions are ballots masked to the
// txn's lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcc.h"
#include "dcc_device.h"

namespace dcc {

constexpr uint32_t NW_T = 256;  // threads per workgroup
// the epoch's error word (next to CHK_ERR_*): the per-epoch table is full
constexpr uint32_t NW_ERR_FULL = 4;
// the level of an epoch (DCC_ISO_*): LtEpoch::level, a template parameter of the rounds' kernels
constexpr int ISO_SER = 0, ISO_RC = 1, ISO_RU = 2;

__device__ inline uint32_t is_ex(uint8_t t) { return (t == DCC_RD || t == DCC_SCAN) ? 0u : 1u; }

// The P = 2^lp lanes of a txn inside the wave.
struct Seg {
  uint32_t a;     // access ordinal of this lane
  uint32_t gl;    // txn of this lane within the workgroup's step
  uint32_t seg0;  // first lane of the txn
  uint64_t mask;  // the txn's lanes
};
__device__ inline Seg seg_of(uint32_t lp) {
  const uint32_t P = 1u << lp;
  Seg s;
  s.a = threadIdx.x & (P - 1);
  s.gl = threadIdx.x >> lp;
  s.seg0 = lane_id() & ~(P - 1);
  s.mask = (P == 64 ? ~0ull : ((1ull << P) - 1ull)) << s.seg0;
  return s;
}

}  // namespace dcc
