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
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "launch_status.h"
#include "nequip_amd.h"

#pragma clang fp contract(off)

namespace nqa {

constexpr int MD_THREADS = NQA_MD_THREADS;
constexpr int MD_WAVES = MD_THREADS / 64;
static_assert(sizeof(nqa_md_state) == 64, "the host writes the record as eight 8-byte words");

// lane 0 ends with the 64 values added by a fixed tree
__device__ __forceinline__ double md_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
  return v;
}

template <typename F>
__global__ __launch_bounds__(MD_THREADS) void md_step_kernel(const F* __restrict__ forces, const double* __restrict__ masses,
                                                              double* __restrict__ positions, double* __restrict__ velocities,
                                                              double* __restrict__ vel_out, int64_t n3,
                                                              const nqa_md_state* __restrict__ state,
                                                              double* __restrict__ partials, int finish_only) {
  __shared__ double waves[MD_WAVES][2];
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
    partials[2 * (int64_t)blockIdx.x] = a;
    partials[2 * (int64_t)blockIdx.x + 1] = b;
  }
}

__global__ __launch_bounds__(64) void md_bath_kernel(const double* __restrict__ partials, int64_t num_partials,
                                                     nqa_md_state* __restrict__ state, int finish_only, int thermostat) {
  const int lane = threadIdx.x;
  const int64_t per = (num_partials + 63) / 64;
  const int64_t lo = lane * per, hi = lo + per < num_partials ? lo + per : num_partials;
  double s_full = 0.0, s_half = 0.0;
  for (int64_t k = lo; k < hi; ++k) {
    s_full += partials[2 * k];
    s_half += partials[2 * k + 1];
  }
  s_full = md_wave_sum(s_full);
  s_half = md_wave_sum(s_half);
  if (lane != 0) return;
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

inline int64_t md_num_partials(int64_t num_atoms) { return (3 * num_atoms + MD_THREADS - 1) / MD_THREADS; }

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

}  // extern "C"
