// group.h — reductions over a group of G consecutive lanes (G = 4, 8, 16 or 64) for the
// kernels that give one loaded state to one group (sync.hip, standby.hip).
//
// A butterfly of DPP moves inside a 16-lane row (pairs, quads, half-row mirror, row mirror) and,
// for G = 64, two ds_bpermute steps across rows.  The moves read lanes of the group only, so the
// groups of one wavefront may diverge from one another as long as the G lanes of a group stay
// together: every branch and trip count around a call must depend on the group's state and
// request alone.  After a reduction every lane of the group holds the result.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cdr/cdr.h"

namespace cdr_group {

// the value of lane (lane ^ OFF)'s — for OFF 4 and 8 of the mirrored lane's, which is in the
// other half of the 8 / 16 lanes and holds that half's reduction already
template <int OFF>
__device__ __forceinline__ uint32_t xlane(uint32_t v) {
  if constexpr (OFF == 1) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
  else if constexpr (OFF == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);
  else if constexpr (OFF == 4) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);
  else if constexpr (OFF == 8) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false);
  else return (uint32_t)__shfl_xor((int)v, OFF, 64);
}
template <int OFF>
__device__ __forceinline__ uint64_t xlane64(uint64_t v) {
  return (uint64_t)xlane<OFF>((uint32_t)v) | ((uint64_t)xlane<OFF>((uint32_t)(v >> 32)) << 32);
}

// the head of the activity timers a lane has seen: smallest (t, sched, order); `info` packs
// order << 4 | timeout type << 1 | bit already set, row = CDR_SYNC_NO_ROW when there is none.
// Only what the comparison needs travels through the reduction: the head row's attempt stays
// with the row.
struct head {
  int64_t t, sched;
  uint32_t info, row;
};
__device__ __forceinline__ bool before(const head& a, const head& b) {
  if (b.row == CDR_SYNC_NO_ROW) return a.row != CDR_SYNC_NO_ROW;
  if (a.row == CDR_SYNC_NO_ROW) return false;
  if (a.t != b.t) return a.t < b.t;
  if (a.sched != b.sched) return a.sched < b.sched;
  return a.info < b.info;
}
template <int OFF>
__device__ __forceinline__ void head_step(head& h) {
  head o;
  o.t = (int64_t)xlane64<OFF>((uint64_t)h.t);
  o.sched = (int64_t)xlane64<OFF>((uint64_t)h.sched);
  o.info = xlane<OFF>(h.info);
  o.row = xlane<OFF>(h.row);
  if (before(o, h)) h = o;
}
template <int G>
__device__ __forceinline__ void group_head(head& h) {
  head_step<1>(h);
  head_step<2>(h);
  if constexpr (G >= 8) head_step<4>(h);
  if constexpr (G >= 16) head_step<8>(h);
  if constexpr (G >= 64) {
    head_step<16>(h);
    head_step<32>(h);
  }
}
template <int OFF>
__device__ __forceinline__ void min_step(uint64_t& m) {
  const uint64_t o = xlane64<OFF>(m);
  m = o < m ? o : m;
}
template <int G>
__device__ __forceinline__ uint64_t group_min(uint64_t m) {
  min_step<1>(m);
  min_step<2>(m);
  if constexpr (G >= 8) min_step<4>(m);
  if constexpr (G >= 16) min_step<8>(m);
  if constexpr (G >= 64) {
    min_step<16>(m);
    min_step<32>(m);
  }
  return m;
}

}  // namespace cdr_group
