// The fixed shuffle tree that adds the 64 lanes of a wavefront, for the MD kernels (md_device.h) and the FIRE kernels
// (fire_device.h): the order of the additions is a property of the tree alone, so the same inputs give the same bits.
#pragma once

#include <hip/hip_runtime.h>

namespace nqa {

// lane 0 ends with the 64 values added by a fixed tree
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
  return v;
}

}  // namespace nqa
