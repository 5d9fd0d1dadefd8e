// Nose-Hoover / velocity-Verlet molecular dynamics (the scheme of nequip/ase/nosehoover.py) with the state in device memory.
//
// The reference integrates in numpy on the host: every step uploads the positions and downloads energy and forces.  Here
// positions, velocities, masses and the bath variable stay on the device and are advanced between two force evaluations by two
// launches, so that a step moves nothing to the host.
//
// One step of the scheme, with F(t) the force at the positions of the start of the step and F(t+dt) the one at the new positions:
//   a = F(t)/m - xi v;  x += dt v + dt^2/2 a;  v_half = v + dt/2 a
//   xi_half = xi + dt/2 (sum m v^2 - g)/(2Q);  xi_new = xi_half + dt/2 (sum m v_half^2 - g)/(2Q)
//   v(t+dt) = (v_half + dt/2 F(t+dt)/m) / (1 + dt/2 xi_new)
// The last line needs the force of the NEXT step, so it is deferred: the velocity buffer holds v_half between two steps and the
// launch of the next step finishes it with the force it was handed anyway (`fresh` in the state record says that the buffer holds
// completed velocities: after construction and after a state was loaded).
//
// Layout: flat over the 3N components, one component per lane, component i of atom i / 3: consecutive lanes read consecutive
// addresses of positions, velocities and forces (no 24-byte row stride per lane).
//   md_step_kernel   finishes v with F and xi, then advances x and v_half; or, in the finish-only mode, writes the completed
//                    velocities to a buffer of their own and changes nothing (the `velocities` reader).  Every workgroup writes
//                    (sum m v^2, sum m v_half^2) over its components to its own row of `partials`: the lanes of a wavefront by a
//                    fixed shuffle tree, the four wavefronts in wavefront order.
//   md_bath_kernel   one wavefront: lane b adds a contiguous run of the rows in ascending order, the lanes are merged by the same
//                    tree, lane 0 forms xi_half and xi_new and writes xi, the kinetic energy of the completed velocities, the
//                    step count and fresh = 0.  In the finish-only mode it writes the observed kinetic energy and nothing else.
// The record hazard is the one ema.hip describes: no workgroup of md_step_kernel may see the new xi, so the record is rewritten
// by a SECOND launch on the same stream; launches of one stream run in order.  No ticket, no atomics, no fence.
// No floating-point atomics and a fixed order of every sum: the same inputs give the same bits.  No contraction into fused
// multiply-adds either, so that the finish of a velocity is the same arithmetic in both modes (a saved and reloaded run
// continues bit for bit) and the steps are the ones a float64 restatement takes.
// LDS: the eight wavefront sums of md_step_kernel.  Nothing is read by the host.
//
// Langevin (BAOAB) dynamics, further down, takes the same two launches: md_langevin_step_kernel, with its noise made on the
// device from a counter-based generator, then md_bath_kernel with the thermostat off.
//
// The generator, the arithmetic of a Langevin component, the partial row of a workgroup, the sum of the rows and the lane-0
// arithmetic of the bath launches are device functions of md_device.h, which md_batched.hip (a batch of systems) calls too.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "launch_status.h"
#include "md_device.h"
#include "nequip_amd.h"

#pragma clang fp contract(off)

namespace nqa {

// MD_THREADS, MD_WAVES, md_wave_sum, md_block_partials, md_sum_rows and md_bath_update: md_device.h (shared with md_batched.hip)
static_assert(sizeof(nqa_md_state) == 64, "the host writes the record as eight 8-byte words");

template <typename F>
__global__ __launch_bounds__(MD_THREADS) void md_step_kernel(const F* __restrict__ forces, const double* __restrict__ masses,
                                                              double* __restrict__ positions, double* __restrict__ velocities,
                                                              double* __restrict__ vel_out, int64_t n3,
                                                              const nqa_md_state* __restrict__ state,
                                                              double* __restrict__ partials, int finish_only) {
  const int64_t i = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
  const double dt = state->dt, xi = state->xi;
  const bool fresh = state->fresh != 0;
  const double hdt = 0.5 * dt;
  double s_full = 0.0, s_half = 0.0;
  if (i < n3) {
    const double m = masses[i / 3];
    const double fm = (double)forces[i] / m;
    double v = velocities[i];
    if (!fresh) v = (v + hdt * fm) / (1.0 + hdt * xi);
    s_full = m * v * v;
    if (finish_only) {
      vel_out[i] = v;
    } else {
      const double a = fm - xi * v;
      positions[i] = positions[i] + dt * v + (0.5 * (dt * dt)) * a;
      const double vh = v + hdt * a;
      velocities[i] = vh;
      s_half = m * vh * vh;
    }
  }
  md_block_partials(s_full, s_half, partials + 2 * (int64_t)blockIdx.x);
}

__global__ __launch_bounds__(64) void md_bath_kernel(const double* __restrict__ partials, int64_t num_partials,
                                                     nqa_md_state* __restrict__ state, int finish_only, int thermostat) {
  double s_full, s_half;
  md_sum_rows(partials, num_partials, true, s_full, s_half);
  if (threadIdx.x != 0) return;
  md_bath_update(state, s_full, s_half, finish_only, thermostat);
}

inline int64_t md_num_partials(int64_t num_atoms) { return (3 * num_atoms + MD_THREADS - 1) / MD_THREADS; }

// ---- Langevin dynamics: BAOAB (Leimkuhler-Matthews) with one force evaluation per step ------------------------------------------
//   B  v1 = v + dt/2 F/m;   A  x += dt/2 v1;   O  v2 = c1 v1 + (c2 sqrt(kT/m)) z;   A  x += dt/2 v2;   B  v' = v2 + dt/2 F'/m
// with c1 = exp(-friction dt) and c2 = sqrt(1 - c1^2) from the host's parameter record and z a standard normal per component.
// The closing B needs the next step's force and is deferred exactly as above: the velocity buffer holds v2 between two steps.
// The noise is a pure function of (seed, step, component): Philox4x32-10 with counter (i, step) and key seed, one call per
// component, Box-Muller on two 53-bit uniforms, the second normal dropped.  `step` is the record's nsteps, which md_bath_kernel
// increments in the second launch (no workgroup here sees the incremented count: the hazard argument of xi), so a captured pair of
// launches draws fresh noise at every replay.  Nothing depends on the grid: a run of N atoms and the noise entry draw the same z.
static_assert(sizeof(nqa_md_langevin_params) == 32, "the host writes the parameters as four 8-byte words");

// md_philox, md_normal and md_langevin_component (the arithmetic of one component): md_device.h

// The layout, the partial rows and the order of every sum are md_step_kernel's.  partials[2b] = sum m v^2 over the completed
// velocities, partials[2b + 1] = sum m v2^2 (0 in the finish-only mode); md_bath_kernel without the thermostat bit reads only
// the first.
template <typename F>
__global__ __launch_bounds__(MD_THREADS) void md_langevin_step_kernel(
    const F* __restrict__ forces, const double* __restrict__ masses, double* __restrict__ positions,
    double* __restrict__ velocities, double* __restrict__ vel_out, int64_t n3, const nqa_md_state* __restrict__ state,
    const nqa_md_langevin_params* __restrict__ params, double* __restrict__ partials, int finish_only) {
  const int64_t i = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
  double s_full = 0.0, s_half = 0.0;
  if (i < n3)
    md_langevin_component(forces, masses, positions, velocities, vel_out, i, (uint64_t)i, state, params, finish_only, s_full,
                          s_half);
  md_block_partials(s_full, s_half, partials + 2 * (int64_t)blockIdx.x);
}

// the generator on its own: the Philox words and / or the normal of components 0 .. count - 1
__global__ __launch_bounds__(MD_THREADS) void md_noise_kernel(uint64_t seed, uint64_t step, int64_t count,
                                                               uint32_t* __restrict__ words, double* __restrict__ normals) {
  const int64_t i = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
  if (i >= count) return;
  uint32_t w[4];
  md_philox(seed, step, (uint64_t)i, w);
  if (words) {
#pragma unroll
    for (int k = 0; k < 4; ++k) words[4 * i + k] = w[k];
  }
  if (normals) normals[i] = md_normal(w);
}

// ---- isotropic NPT: the Langevin step, then stochastic cell rescaling (Bernetti-Bussi, first order in the volume) ---------------
//   md_langevin_step_kernel (unchanged), md_npt_bath_kernel in place of md_bath_kernel, md_npt_scale_kernel.
// The bath launch adds the partial rows exactly as md_bath_kernel does (the kinetic energy has the bits of a Langevin run), and
// lane 0 forms the pressure of the start of the step from it and the stress, draws ONE normal (component 3N of the step's noise,
// one past the atoms'), scales the cell and leaves mu in the record; the third launch scales positions and stored velocities.
// mu is written by the second launch and read by the third; nsteps and fresh are written by the second and read by the first
// of the NEXT step: the ordering argument of the top of this file, no launch sees a word that a launch of its own step rewrites.
static_assert(sizeof(nqa_md_npt_state) == 64, "the host writes the record as eight 8-byte words");

template <typename S>
__global__ __launch_bounds__(64) void md_npt_bath_kernel(const double* __restrict__ partials, int64_t num_partials,
                                                         nqa_md_state* __restrict__ state,
                                                         const nqa_md_langevin_params* __restrict__ params,
                                                         nqa_md_npt_state* __restrict__ npt, const S* __restrict__ stress,
                                                         double* __restrict__ cell) {
  double s_full, s_half;
  md_sum_rows(partials, num_partials, false, s_full, s_half);
  if (threadIdx.x != 0) return;
  md_npt_bath_update(s_full, state, params, npt, stress, cell);
}

__global__ __launch_bounds__(MD_THREADS) void md_npt_scale_kernel(double* __restrict__ positions, double* __restrict__ velocities,
                                                                   int64_t n3, const nqa_md_npt_state* __restrict__ npt) {
  const int64_t i = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
  if (i >= n3) return;
  const double mu = npt->mu;
  positions[i] = mu * positions[i];
  velocities[i] = velocities[i] / mu;
}

}  // namespace nqa

extern "C" {

int64_t nqa_md_num_partials(int64_t num_atoms) { return num_atoms > 0 ? nqa::md_num_partials(num_atoms) : 0; }

int nqa_md_step(int32_t force_dtype, const void* forces, const double* masses, double* positions, double* velocities,
                double* vel_out, int64_t num_atoms, const nqa_md_state* state, double* partials, int32_t mode, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_md_step";
  const bool finish_only = (mode & NQA_MD_FINISH_ONLY) != 0;
  if (num_atoms <= 0 || num_atoms > INT32_MAX) {
    set_error(std::string(name) + ": 0 < num_atoms < 2^31");
    return NQA_ERR_INVALID;
  }
  if (force_dtype != NQA_F32 && force_dtype != NQA_F64) {
    set_error(std::string(name) + ": forces are float32 or float64");
    return NQA_ERR_UNSUPPORTED;
  }
  if ((mode & ~(NQA_MD_FINISH_ONLY | NQA_MD_THERMOSTAT)) != 0) {
    set_error(std::string(name) + ": unknown mode bits");
    return NQA_ERR_INVALID;
  }
  if (!forces || !masses || !velocities || !state || !partials || (finish_only ? !vel_out : !positions)) {
    set_error(std::string(name) + ": forces, masses, velocities, state and partials are required, and positions (or, in the "
                                  "finish-only mode, the output buffer)");
    return NQA_ERR_INVALID;
  }
  const int64_t n3 = 3 * num_atoms;
  const dim3 grid((unsigned)md_num_partials(num_atoms));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (force_dtype == NQA_F64)
    hipLaunchKernelGGL(md_step_kernel<double>, grid, dim3(MD_THREADS), 0, s, (const double*)forces, masses, positions, velocities,
                       vel_out, n3, state, partials, (int)finish_only);
  else
    hipLaunchKernelGGL(md_step_kernel<float>, grid, dim3(MD_THREADS), 0, s, (const float*)forces, masses, positions, velocities,
                       vel_out, n3, state, partials, (int)finish_only);
  return launch_status(name);
}

int nqa_md_bath(const double* partials, int64_t num_partials, nqa_md_state* state, int32_t mode, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_md_bath";
  if (num_partials <= 0 || !partials || !state || (mode & ~(NQA_MD_FINISH_ONLY | NQA_MD_THERMOSTAT)) != 0) {
    set_error(std::string(name) + ": partials (num_partials > 0) and state are required, and known mode bits");
    return NQA_ERR_INVALID;
  }
  hipLaunchKernelGGL(md_bath_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), partials, num_partials, state,
                     (int)((mode & NQA_MD_FINISH_ONLY) != 0), (int)((mode & NQA_MD_THERMOSTAT) != 0));
  return launch_status(name);
}

int nqa_md_langevin_step(int32_t force_dtype, const void* forces, const double* masses, double* positions, double* velocities,
                         double* vel_out, int64_t num_atoms, const nqa_md_state* state, const nqa_md_langevin_params* params,
                         double* partials, int32_t mode, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_md_langevin_step";
  const bool finish_only = (mode & NQA_MD_FINISH_ONLY) != 0;
  if (num_atoms <= 0 || num_atoms > INT32_MAX) {
    set_error(std::string(name) + ": 0 < num_atoms < 2^31");
    return NQA_ERR_INVALID;
  }
  if (force_dtype != NQA_F32 && force_dtype != NQA_F64) {
    set_error(std::string(name) + ": forces are float32 or float64");
    return NQA_ERR_UNSUPPORTED;
  }
  if ((mode & ~NQA_MD_FINISH_ONLY) != 0) {
    set_error(std::string(name) + ": unknown mode bits (the thermostat bit belongs to nqa_md_step)");
    return NQA_ERR_INVALID;
  }
  if (!forces || !masses || !velocities || !state || !params || !partials || (finish_only ? !vel_out : !positions)) {
    set_error(std::string(name) + ": forces, masses, velocities, state, params and partials are required, and positions (or, in "
                                  "the finish-only mode, the output buffer)");
    return NQA_ERR_INVALID;
  }
  const int64_t n3 = 3 * num_atoms;
  const dim3 grid((unsigned)md_num_partials(num_atoms));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (force_dtype == NQA_F64)
    hipLaunchKernelGGL(md_langevin_step_kernel<double>, grid, dim3(MD_THREADS), 0, s, (const double*)forces, masses, positions,
                       velocities, vel_out, n3, state, params, partials, (int)finish_only);
  else
    hipLaunchKernelGGL(md_langevin_step_kernel<float>, grid, dim3(MD_THREADS), 0, s, (const float*)forces, masses, positions,
                       velocities, vel_out, n3, state, params, partials, (int)finish_only);
  return launch_status(name);
}

int nqa_md_noise(uint64_t seed, uint64_t step, int64_t count, uint32_t* words, double* normals, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_md_noise";
  if (count <= 0 || count > 3 * (int64_t)INT32_MAX) {
    set_error(std::string(name) + ": 0 < count <= 3 (2^31 - 1), the components of nqa_md_langevin_step");
    return NQA_ERR_INVALID;
  }
  if (!words && !normals) {
    set_error(std::string(name) + ": words or normals (or both) are required");
    return NQA_ERR_INVALID;
  }
  const dim3 grid((unsigned)((count + MD_THREADS - 1) / MD_THREADS));
  hipLaunchKernelGGL(md_noise_kernel, grid, dim3(MD_THREADS), 0, static_cast<hipStream_t>(stream), seed, step, count, words,
                     normals);
  return launch_status(name);
}

int nqa_md_npt_bath(const double* partials, int64_t num_partials, nqa_md_state* state, const nqa_md_langevin_params* params,
                    nqa_md_npt_state* npt, int32_t stress_dtype, const void* stress, double* cell, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_md_npt_bath";
  if (stress_dtype != NQA_F32 && stress_dtype != NQA_F64) {
    set_error(std::string(name) + ": the stress is float32 or float64");
    return NQA_ERR_UNSUPPORTED;
  }
  if (num_partials <= 0 || !partials || !state || !params || !npt) {
    set_error(std::string(name) + ": partials (num_partials > 0), state, params and the npt record are required");
    return NQA_ERR_INVALID;
  }
  if (!stress || !cell) {
    set_error(std::string(name) + ": stress and cell ([3, 3] each) are required");
    return NQA_ERR_INVALID;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (stress_dtype == NQA_F64)
    hipLaunchKernelGGL(md_npt_bath_kernel<double>, dim3(1), dim3(64), 0, s, partials, num_partials, state, params, npt,
                       (const double*)stress, cell);
  else
    hipLaunchKernelGGL(md_npt_bath_kernel<float>, dim3(1), dim3(64), 0, s, partials, num_partials, state, params, npt,
                       (const float*)stress, cell);
  return launch_status(name);
}

int nqa_md_npt_scale(double* positions, double* velocities, int64_t num_atoms, const nqa_md_npt_state* npt, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_md_npt_scale";
  if (num_atoms <= 0 || num_atoms > INT32_MAX) {
    set_error(std::string(name) + ": 0 < num_atoms < 2^31");
    return NQA_ERR_INVALID;
  }
  if (!positions || !velocities || !npt) {
    set_error(std::string(name) + ": positions, velocities and the npt record are required");
    return NQA_ERR_INVALID;
  }
  const dim3 grid((unsigned)md_num_partials(num_atoms));
  hipLaunchKernelGGL(md_npt_scale_kernel, grid, dim3(MD_THREADS), 0, static_cast<hipStream_t>(stream), positions, velocities,
                     3 * num_atoms, npt);
  return launch_status(name);
}

}  // extern "C"
