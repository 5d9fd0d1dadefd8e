// The device functions that the MD kernels of md.hip (one system) and md_batched.hip (a batch of systems) share: the fixed
// shuffle tree, the noise generator, the BAOAB arithmetic of one component, the partial row of a workgroup, the sum of the partial
// rows by one wavefront and the lane-0 arithmetic of the bath and NPT-bath launches.  One statement of every equation: a system
// takes the same steps, bit for bit, through either file.  Every file that includes this one sets `#pragma clang fp contract(off)`
// itself as well; the pragma below covers the functions defined here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "nequip_amd.h"
#include "wave_sum.h"

#pragma clang fp contract(off)

namespace nqa {

constexpr int MD_THREADS = NQA_MD_THREADS;
constexpr int MD_WAVES = MD_THREADS / 64;

__device__ __forceinline__ double md_wave_sum(double v) { return wave_sum(v); }  // (the tree of wave_sum.h)

// The row of a workgroup of MD_THREADS lanes: the lanes of a wavefront by the tree, the four wavefronts in wavefront order.
// Every lane of the workgroup must call it (it holds a barrier).
__device__ __forceinline__ void md_block_partials(double s_full, double s_half, double* __restrict__ row) {
  __shared__ double waves[MD_WAVES][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  s_full = md_wave_sum(s_full);
  s_half = md_wave_sum(s_half);
  if (lane == 0) {
    waves[wave][0] = s_full;
    waves[wave][1] = s_half;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = waves[0][0], b = waves[0][1];
#pragma unroll
    for (int k = 1; k < MD_WAVES; ++k) {
      a += waves[k][0];
      b += waves[k][1];
    }
    row[0] = a;
    row[1] = b;
  }
}

// One wavefront over `num_partials` rows: lane b adds a contiguous run of ceil(num_partials / 64) rows in ascending order, the
// lanes are merged by the tree; lane 0 holds the sums.
__device__ __forceinline__ void md_sum_rows(const double* __restrict__ partials, int64_t num_partials, bool with_half,
                                            double& s_full, double& s_half) {
  const int lane = threadIdx.x;
  const int64_t per = (num_partials + 63) / 64;
  const int64_t lo = lane * per, hi = lo + per < num_partials ? lo + per : num_partials;
  s_full = 0.0, s_half = 0.0;
  for (int64_t k = lo; k < hi; ++k) {
    s_full += partials[2 * k];
    if (with_half) s_half += partials[2 * k + 1];
  }
  s_full = md_wave_sum(s_full);
  if (with_half) s_half = md_wave_sum(s_half);
}

// lane 0 of the bath launch
__device__ __forceinline__ void md_bath_update(nqa_md_state* __restrict__ state, double s_full, double s_half, int finish_only,
                                               int thermostat) {
  if (finish_only) {
    state->observed_kinetic_energy = 0.5 * s_full;
    return;
  }
  if (thermostat) {
    const double hdt = 0.5 * state->dt, g = state->g, q = state->q;
    const double xi_half = state->xi + hdt * (0.5 * (s_full - g)) / q;
    state->xi = xi_half + hdt * (0.5 * (s_half - g)) / q;
  }
  state->kinetic_energy = 0.5 * s_full;
  state->nsteps += 1;
  state->fresh = 0;
}

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

// Philox4x32-10 (Salmon et al., Random123): counter (i lo, i hi, step lo, step hi), key (seed lo, seed hi)
__device__ __forceinline__ void md_philox(uint64_t seed, uint64_t step, uint64_t i, uint32_t w[4]) {
  uint32_t c0 = (uint32_t)i, c1 = (uint32_t)(i >> 32), c2 = (uint32_t)step, c3 = (uint32_t)(step >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
    const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// u1 in (0, 1] and u2 in [0, 1) from 53 bits each (every operation up to the product with 2 pi is exact), then Box-Muller
__device__ __forceinline__ double md_normal(const uint32_t w[4]) {
  const double u1 = ((double)(w[0] >> 5) * 67108864.0 + (double)(w[1] >> 6) + 1.0) * 0x1p-53;
  const double u2 = ((double)(w[2] >> 5) * 67108864.0 + (double)(w[3] >> 6)) * 0x1p-53;
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

// The BAOAB arithmetic of one flat component: `i` is its place in forces / positions / velocities (atom i / 3), `j` the index its
// noise is drawn for (the same number for one system; the component's index inside its own system in a batch).
template <typename F>
__device__ __forceinline__ void md_langevin_component(const F* __restrict__ forces, const double* __restrict__ masses,
                                                      double* __restrict__ positions, double* __restrict__ velocities,
                                                      double* __restrict__ vel_out, int64_t i, uint64_t j,
                                                      const nqa_md_state* __restrict__ state,
                                                      const nqa_md_langevin_params* __restrict__ params, int finish_only,
                                                      double& s_full, double& s_half) {
  const double dt = state->dt;
  const bool fresh = state->fresh != 0;
  const uint64_t step = (uint64_t)state->nsteps;
  const double hdt = 0.5 * dt;
  const double m = masses[i / 3];
  const double fm = (double)forces[i] / m;
  double v = velocities[i];
  if (!fresh) v = v + hdt * fm;
  s_full = m * v * v;
  if (finish_only) {
    vel_out[i] = v;
  } else {
    const double c1 = params->c1, c2 = params->c2, kT = params->kT;
    uint32_t w[4];
    md_philox(params->seed, step, j, w);
    const double z = md_normal(w);
    const double v1 = v + hdt * fm;
    double x = positions[i] + hdt * v1;
    const double v2 = c1 * v1 + (c2 * sqrt(kT / m)) * z;
    x = x + hdt * v2;
    positions[i] = x;
    velocities[i] = v2;
    s_half = m * v2 * v2;
  }
}

// lane 0 of the NPT bath launch: the pressure of the start of the step from K = s_full / 2 and the stress, one normal, the cell
// scaled and mu left in the record; `stress` and `cell` are the [3, 3] of this system.
template <typename S>
__device__ __forceinline__ void md_npt_bath_update(double s_full, nqa_md_state* __restrict__ state,
                                                   const nqa_md_langevin_params* __restrict__ params,
                                                   nqa_md_npt_state* __restrict__ npt, const S* __restrict__ stress,
                                                   double* __restrict__ cell) {
  const double ekin = 0.5 * s_full;
  double c[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) c[k] = cell[k];
  const double det = c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6]);
  const double vol = fabs(det);
  const double p = (2.0 * ekin) / (3.0 * vol) - ((double)stress[0] + (double)stress[4] + (double)stress[8]) / 3.0;
  uint32_t w[4];
  md_philox(params->seed, (uint64_t)state->nsteps, (uint64_t)npt->noise_index, w);
  const double xi = md_normal(w);
  const double a = npt->a;
  const double d_eps = -a * (npt->p0 - p) + sqrt((2.0 * params->kT * a) / vol) * xi;
  double mu = exp(d_eps / 3.0);
  if (!isfinite(mu) || !(vol > 0.0)) {
    mu = 1.0;
    npt->failed = 1;
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) cell[k] = mu * c[k];
  npt->mu = mu;
  npt->pressure = p;
  npt->kinetic_energy = ekin;
  npt->volume = vol;
  state->kinetic_energy = ekin;
  state->nsteps += 1;
  state->fresh = 0;
}

}  // namespace nqa
