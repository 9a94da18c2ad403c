// lane_group.hpp — W lanes of one wave that work on the same small dense problem (W = 8, 16, 32 or 64): the group that the
// per-problem statements oadp_step.hpp and qp_step.hpp are written for.  The group's lanes run in lockstep; its sums are
// butterflies of __shfl_xor inside the group (every lane receives the same bits); where a lane reads what another lane of
// its group wrote, a wave-scope fence keeps the compiler from moving the accesses (the LDS serves one wave's accesses in
// order).  The workgroup is ONE wave: nothing waits for another wave and no workgroup barrier is needed.
#pragma once
#include <hip/hip_runtime.h>

namespace bsn {

constexpr int kLaneGroupWave = 64;

template <int W>
struct LaneGroup {
  static constexpr int width = W;
  int lane;
  __device__ __forceinline__ double sum(double x) const {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, W);
    return x;
  }
  __device__ __forceinline__ void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
};

}  // namespace bsn
