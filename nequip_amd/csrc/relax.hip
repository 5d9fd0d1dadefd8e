// FIRE structural relaxation (Bitzek et al. 2006, with ASE's defaults and step cap) with the state in device memory, for one
// system or a batch of independent systems concatenated along the atom axis.
//
// A user of a calculator relaxes on the host: every step uploads the positions, downloads energy and forces and runs the
// optimizer in numpy.  Here positions, velocities and one record per system (time step, mixing factor, counters, verdict) stay on
// the device and are advanced between two force evaluations by three launches, so that a step moves nothing to the host.
//
// One step of a system, with F the force at the current positions (components of fixed atoms count as zero):
//   reduce   P = sum F.v,  FF = sum F.F,  VV = sum v.v,  M = max over atoms of |F|^2
//   decide   fmax = sqrt(M), converged = M < fmax_target^2; unless converged: the FIRE branch on P > 0 (none at the first step,
//            where v = 0), which gives the mixing coefficients cv, cf, the new dt and a; then the step cap from the three sums:
//            c = cf + dt,  VVn = cv^2 VV + 2 cv c P + c^2 FF  (= |v_new|^2 up to rounding, every term non-negative),
//            normdr = dt sqrt(VVn),  scale = normdr > maxstep ? maxstep / normdr : 1
//   move     v = cv v + cf F;  v = v + dt F;  x = x + scale (dt v)        (skipped for converged systems and fixed atoms)
// Forming the step length from the sums of the OLD velocities spares a third reduction; it is the one deliberate difference from
// the textbook loop, which takes the norm of the new displacements directly.
//
// Layout: the atoms are cut into chunks of at most NQA_FIRE_CHUNK atoms, none of which straddles two systems (the host builds the
// table once from system_idx).
//   fire_reduce_kernel   one workgroup per chunk, one atom per lane (so |F|^2 of an atom needs no cross-lane work); row b of
//                        `partials` holds (P, FF, VV, M) of chunk b (fire_block_partials).
//   fire_decide_kernel   one wavefront per system merges its rows (fire_sum_rows); lane 0 decides and rewrites the record
//                        (fire_decide).  The three are the device functions of fire_device.h, which relax_cell.hip calls too.
//   fire_move_kernel     one workgroup per chunk, flat over the chunk's 3 * count components.
// The record hazard is the one md.hip describes: no workgroup of the reduction or of the move may see a half-written record, so
// the three are three launches on one stream; launches of one stream run in order.  No ticket, no atomics, no fence.
// No floating-point atomics, a fixed order of every sum, no contraction into fused multiply-adds: the same inputs give the same
// bits, a system relaxes to the same bits alone and inside a batch, and the steps are the ones a float64 restatement takes.
// LDS: the sixteen wavefront partials of fire_reduce_kernel.  Nothing is read by the host.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "fire_device.h"
#include "launch_status.h"
#include "nequip_amd.h"

#pragma clang fp contract(off)

namespace nqa {

// FIRE_CHUNK, FIRE_WAVES, fire_block_partials, fire_sum_rows and fire_decide: fire_device.h (shared with relax_cell.hip)
static_assert(sizeof(nqa_fire_system) == 128, "the host writes the record as sixteen 8-byte words");
static_assert(sizeof(nqa_fire_chunk) == 16, "the host writes a chunk as two 8-byte words");

template <typename F>
__global__ __launch_bounds__(FIRE_CHUNK) void fire_reduce_kernel(const F* __restrict__ forces,
                                                                  const double* __restrict__ velocities,
                                                                  const uint8_t* __restrict__ fixed,
                                                                  const nqa_fire_chunk* __restrict__ chunks,
                                                                  double* __restrict__ partials) {
  const nqa_fire_chunk chunk = chunks[blockIdx.x];
  const int count = chunk.count < FIRE_CHUNK ? chunk.count : FIRE_CHUNK;
  double p = 0.0, ff = 0.0, vv = 0.0;
  if ((int)threadIdx.x < count) {
    const int64_t atom = chunk.atom0 + threadIdx.x;
    if (!(fixed && fixed[atom])) {
      const double fx = (double)forces[3 * atom], fy = (double)forces[3 * atom + 1], fz = (double)forces[3 * atom + 2];
      const double vx = velocities[3 * atom], vy = velocities[3 * atom + 1], vz = velocities[3 * atom + 2];
      p = fx * vx + fy * vy + fz * vz;
      ff = fx * fx + fy * fy + fz * fz;
      vv = vx * vx + vy * vy + vz * vz;
    }
  }
  fire_block_partials(p, ff, vv, partials + 4 * (int64_t)blockIdx.x);
}

__global__ __launch_bounds__(64) void fire_decide_kernel(const double* __restrict__ partials,
                                                         const int64_t* __restrict__ chunk_begin,
                                                         nqa_fire_system* __restrict__ systems) {
  double P, FF, VV, M;
  fire_sum_rows(partials, chunk_begin[blockIdx.x], chunk_begin[blockIdx.x + 1], P, FF, VV, M);
  if (threadIdx.x == 0) fire_decide(systems + blockIdx.x, P, FF, VV, M);
}

template <typename F>
__global__ __launch_bounds__(FIRE_CHUNK) void fire_move_kernel(const F* __restrict__ forces, double* __restrict__ positions,
                                                                double* __restrict__ velocities,
                                                                const uint8_t* __restrict__ fixed,
                                                                const nqa_fire_chunk* __restrict__ chunks,
                                                                const nqa_fire_system* __restrict__ systems) {
  const nqa_fire_chunk chunk = chunks[blockIdx.x];
  const nqa_fire_system* s = systems + chunk.system;
  if (s->converged != 0) return;
  const int count = chunk.count < FIRE_CHUNK ? chunk.count : FIRE_CHUNK;
  const double cv = s->cv, cf = s->cf, dt = s->dt, scale = s->scale;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int j = k * FIRE_CHUNK + (int)threadIdx.x;  // component j of the chunk belongs to its atom j / 3
    if (j >= 3 * count) break;
    if (fixed && fixed[chunk.atom0 + j / 3]) continue;
    const int64_t i = 3 * chunk.atom0 + j;
    const double f = (double)forces[i];
    double v = cv * velocities[i] + cf * f;
    v = v + dt * f;
    velocities[i] = v;
    positions[i] = positions[i] + scale * (dt * v);
  }
}

}  // namespace nqa

extern "C" {

int32_t nqa_fire_chunk_atoms(void) { return NQA_FIRE_CHUNK; }

int nqa_fire_reduce(int32_t force_dtype, const void* forces, const double* velocities, const uint8_t* fixed,
                    const nqa_fire_chunk* chunks, int64_t n_chunks, double* partials, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_fire_reduce";
  if (n_chunks <= 0 || n_chunks > INT32_MAX) {
    set_error(std::string(name) + ": 0 < n_chunks < 2^31");
    return NQA_ERR_INVALID;
  }
  if (force_dtype != NQA_F32 && force_dtype != NQA_F64) {
    set_error(std::string(name) + ": forces are float32 or float64");
    return NQA_ERR_UNSUPPORTED;
  }
  if (!forces || !velocities || !chunks || !partials) {
    set_error(std::string(name) + ": forces, velocities, chunks and partials are required (fixed may be null)");
    return NQA_ERR_INVALID;
  }
  const dim3 grid((unsigned)n_chunks);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (force_dtype == NQA_F64)
    hipLaunchKernelGGL(fire_reduce_kernel<double>, grid, dim3(FIRE_CHUNK), 0, s, (const double*)forces, velocities, fixed, chunks,
                       partials);
  else
    hipLaunchKernelGGL(fire_reduce_kernel<float>, grid, dim3(FIRE_CHUNK), 0, s, (const float*)forces, velocities, fixed, chunks,
                       partials);
  return launch_status(name);
}

int nqa_fire_decide(const double* partials, const int64_t* chunk_begin, nqa_fire_system* systems, int64_t n_systems,
                    nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_fire_decide";
  if (n_systems <= 0 || n_systems > INT32_MAX) {
    set_error(std::string(name) + ": 0 < n_systems < 2^31");
    return NQA_ERR_INVALID;
  }
  if (!partials || !chunk_begin || !systems) {
    set_error(std::string(name) + ": partials, chunk_begin ([n_systems + 1]) and systems are required");
    return NQA_ERR_INVALID;
  }
  hipLaunchKernelGGL(fire_decide_kernel, dim3((unsigned)n_systems), dim3(64), 0, static_cast<hipStream_t>(stream), partials,
                     chunk_begin, systems);
  return launch_status(name);
}

int nqa_fire_move(int32_t force_dtype, const void* forces, double* positions, double* velocities, const uint8_t* fixed,
                  const nqa_fire_chunk* chunks, int64_t n_chunks, const nqa_fire_system* systems, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_fire_move";
  if (n_chunks <= 0 || n_chunks > INT32_MAX) {
    set_error(std::string(name) + ": 0 < n_chunks < 2^31");
    return NQA_ERR_INVALID;
  }
  if (force_dtype != NQA_F32 && force_dtype != NQA_F64) {
    set_error(std::string(name) + ": forces are float32 or float64");
    return NQA_ERR_UNSUPPORTED;
  }
  if (!forces || !positions || !velocities || !chunks || !systems) {
    set_error(std::string(name) + ": forces, positions, velocities, chunks and systems are required (fixed may be null)");
    return NQA_ERR_INVALID;
  }
  const dim3 grid((unsigned)n_chunks);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (force_dtype == NQA_F64)
    hipLaunchKernelGGL(fire_move_kernel<double>, grid, dim3(FIRE_CHUNK), 0, s, (const double*)forces, positions, velocities, fixed,
                       chunks, systems);
  else
    hipLaunchKernelGGL(fire_move_kernel<float>, grid, dim3(FIRE_CHUNK), 0, s, (const float*)forces, positions, velocities, fixed,
                       chunks, systems);
  return launch_status(name);
}

}  // extern "C"
