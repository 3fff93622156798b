// dexr_tip_inst.hip -- the float32 tip solve kernel (dexr_tip_solve.hpp) in a translation unit of its own.
#include "dexr_launch.hpp"
#include "dexr_tip_solve.hpp"

namespace dexr {
hipError_t launch_tip32(const KernelParams& kp, dim3 grid, dim3 block, size_t lds, hipStream_t st) {
  hipLaunchKernelGGL(dexr_tip32_kernel, grid, block, lds, st, kp, kp.comps);
  return hipGetLastError();
}
}  // namespace dexr
