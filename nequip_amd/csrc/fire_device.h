// The device functions that the FIRE kernels of relax.hip (fixed cell) and relax_cell.hip (variable cell) share: the fixed shuffle
// trees, the partial row of a workgroup, the merge of a system's rows by one wavefront and the lane-0 decision.  One statement of
// the FIRE arithmetic: CellFIRE is the fixed-cell definition because both files call fire_decide, not because two texts agree.
// Every file that includes this one sets `#pragma clang fp contract(off)` itself as well; the pragma below covers the functions
// defined here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "nequip_amd.h"
#include "wave_sum.h"

#pragma clang fp contract(off)

namespace nqa {

constexpr int FIRE_CHUNK = NQA_FIRE_CHUNK;
constexpr int FIRE_WAVES = FIRE_CHUNK / 64;
static_assert(FIRE_CHUNK % 64 == 0 && FIRE_CHUNK <= 1024, "one atom per lane of a workgroup of whole wavefronts");

// the larger of two, a NaN on either side kept (a NaN force or stress must reach fmax, not vanish in a max)
__device__ __forceinline__ double fire_max(double a, double b) { return (a > b || a != a) ? a : b; }

// lane 0 ends with the largest of the 64 values, by the tree of wave_sum
__device__ __forceinline__ double fire_wave_max(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fire_max(v, __shfl_down(v, off));
  return v;
}

// The row (P, FF, VV, M) of a workgroup of FIRE_CHUNK lanes, lane i holding p, ff, vv of its atom (M is the largest ff): the lanes
// of a wavefront by the trees, the wavefronts in wavefront order.  Every lane of the workgroup must call it (it holds a barrier).
__device__ __forceinline__ void fire_block_partials(double p, double ff, double vv, double* __restrict__ row) {
  __shared__ double waves[FIRE_WAVES][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double m = fire_wave_max(ff);
  p = wave_sum(p);
  ff = wave_sum(ff);
  vv = wave_sum(vv);
  if (lane == 0) {
    waves[wave][0] = p;
    waves[wave][1] = ff;
    waves[wave][2] = vv;
    waves[wave][3] = m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = waves[0][0], b = waves[0][1], c = waves[0][2], d = waves[0][3];
#pragma unroll
    for (int k = 1; k < FIRE_WAVES; ++k) {
      a += waves[k][0];
      b += waves[k][1];
      c += waves[k][2];
      d = fire_max(d, waves[k][3]);
    }
    row[0] = a;
    row[1] = b;
    row[2] = c;
    row[3] = d;
  }
}

// One wavefront over the rows begin .. end of `partials`: the rows are dealt to the lanes in contiguous ascending runs of
// ceil(n / 64) and the lanes are merged by the trees; lane 0 holds the result.
__device__ __forceinline__ void fire_sum_rows(const double* __restrict__ partials, int64_t begin, int64_t end, double& P,
                                              double& FF, double& VV, double& M) {
  const int lane = threadIdx.x;
  const int64_t n = end > begin ? end - begin : 0;
  const int64_t per = (n + 63) / 64;
  const int64_t lo = begin + lane * per, hi = lo + per < begin + n ? lo + per : begin + n;
  P = 0.0, FF = 0.0, VV = 0.0, M = 0.0;
  for (int64_t k = lo; k < hi; ++k) {
    P += partials[4 * k];
    FF += partials[4 * k + 1];
    VV += partials[4 * k + 2];
    M = fire_max(M, partials[4 * k + 3]);
  }
  P = wave_sum(P);
  FF = wave_sum(FF);
  VV = wave_sum(VV);
  M = fire_wave_max(M);
}

// The decision of one system from its four sums, by one lane; Record is nqa_fire_system or nqa_cellfire_system (the same first
// seventeen fields).  Writes fmax and converged; unless converged, takes the FIRE branch and writes scale, cv, cf, dt, a, npos and
// nsteps += 1.  Returns whether the system is active (not converged): its record then holds the coefficients of this step's move.
template <typename Record>
__device__ __forceinline__ bool fire_decide(Record* __restrict__ s, double P, double FF, double VV, double M) {
  const bool converged = M < s->fmax_target * s->fmax_target;
  s->fmax = sqrt(M);
  s->converged = converged ? 1 : 0;
  if (converged) return false;
  double dt = s->dt, a = s->a, cv = 0.0, cf = 0.0;
  int64_t npos = s->npos;
  if (s->nsteps == 0) {
    // the first step: the velocities are zero by construction, no branch is taken
  } else if (P > 0.0) {
    cv = 1.0 - a;
    cf = a * sqrt(VV) / sqrt(FF);
    if (npos > (int64_t)s->nmin) {
      const double grown = dt * s->finc;
      dt = grown < s->dtmax ? grown : s->dtmax;
      a = a * s->fa;
    }
    npos += 1;
  } else {  // downhill no more, or a NaN
    a = s->astart;
    dt = dt * s->fdec;
    npos = 0;
  }
  const double c = cf + dt;
  const double vvn = cv * cv * VV + 2.0 * cv * c * P + c * c * FF;
  const double normdr = dt * sqrt(vvn);
  s->scale = normdr > s->maxstep ? s->maxstep / normdr : 1.0;
  s->cv = cv;
  s->cf = cf;
  s->dt = dt;
  s->a = a;
  s->npos = npos;
  s->nsteps += 1;
  return true;
}

}  // namespace nqa
