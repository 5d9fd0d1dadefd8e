// Langevin NVT and NPT dynamics of a batch of independent systems concatenated along the atom axis, each with its own records:
// nqa_md_state[S], nqa_md_langevin_params[S], nqa_md_npt_state[S], cells [S, 3, 3].  The whole batch advances by the two (NVT) or
// three (NPT) launches that one system takes in md.hip, and system s of the batch takes, bit for bit, the steps that md.hip takes
// for it alone with the same seed, forces and stress.  Three things make that so:
//
//   The arithmetic is md.hip's: both files call the device functions of md_device.h (the BAOAB arithmetic of a component, the
//   generator, the partial row of a workgroup, the sum of the rows by one wavefront, lane 0 of the bath and the NPT bath).
//
//   The noise index is local.  The noise of a component is a function of (seed of its system, nsteps of its system, j), j the
//   component's index INSIDE its system, 0 .. 3 n_s - 1; the barostat's normal is component 3 n_s (the record's noise_index).
//   The global index decides only which addresses a lane reads and writes.
//
//   The partition is md.hip's.  Chunk k of system s covers its local components [256 k, min(256 (k + 1), 3 n_s)), one workgroup
//   per chunk, one component per lane: the workgroups md_langevin_step_kernel would launch for n_s atoms, so a chunk may straddle
//   two atoms but never two systems (nqa_md_chunk, built by the host once).  Row c of `partials` belongs to chunk c; the rows
//   of system s are chunk_begin[s] .. chunk_begin[s + 1], P_s = nqa_md_num_partials(n_s) of them.  The bath launches run one
//   wavefront PER SYSTEM (grid S): lane b adds the contiguous run of ceil(P_s / 64) rows of its system in ascending order, the
//   lanes are merged by the same tree: the order of md_bath_kernel for P_s rows.
//
// The record hazard is the one md.hip states: the records are rewritten only by the second launch (no workgroup of the first sees
// an incremented nsteps or a cleared `fresh`), mu is written by the second launch and read by the third; launches of one stream
// run in order.  No atomics, no contraction into fused multiply-adds, no allocation, no host synchronisation: the launches
// capture into a hipGraph, and a replay draws fresh noise since the step counts live in the records.
// A 64-atom system fills 192 of the 256 lanes of its only chunk: these are streaming kernels of a few loads per lane.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "launch_status.h"
#include "md_device.h"
#include "nequip_amd.h"

#pragma clang fp contract(off)

namespace nqa {

static_assert(sizeof(nqa_md_chunk) == 24, "the host writes a chunk as three 8-byte words");

template <typename F>
__global__ __launch_bounds__(MD_THREADS) void md_batched_langevin_step_kernel(
    const F* __restrict__ forces, const double* __restrict__ masses, double* __restrict__ positions,
    double* __restrict__ velocities, double* __restrict__ vel_out, const nqa_md_chunk* __restrict__ chunks,
    const nqa_md_state* __restrict__ states, const nqa_md_langevin_params* __restrict__ params, double* __restrict__ partials,
    int finish_only) {
  const nqa_md_chunk chunk = chunks[blockIdx.x];
  double s_full = 0.0, s_half = 0.0;
  if ((int)threadIdx.x < chunk.count)
    md_langevin_component(forces, masses, positions, velocities, vel_out, chunk.component0 + threadIdx.x,
                          (uint64_t)(chunk.local0 + threadIdx.x), states + chunk.system, params + chunk.system, finish_only,
                          s_full, s_half);
  md_block_partials(s_full, s_half, partials + 2 * (int64_t)blockIdx.x);
}

__global__ __launch_bounds__(64) void md_batched_bath_kernel(const double* __restrict__ partials,
                                                             const int64_t* __restrict__ chunk_begin,
                                                             nqa_md_state* __restrict__ states, int finish_only) {
  const int64_t s = blockIdx.x, begin = chunk_begin[s], end = chunk_begin[s + 1];
  double s_full, s_half;
  md_sum_rows(partials + 2 * begin, end - begin, true, s_full, s_half);
  if (threadIdx.x != 0) return;
  md_bath_update(states + s, s_full, s_half, finish_only, 0);
}

template <typename S>
__global__ __launch_bounds__(64) void md_batched_npt_bath_kernel(const double* __restrict__ partials,
                                                                 const int64_t* __restrict__ chunk_begin,
                                                                 nqa_md_state* __restrict__ states,
                                                                 const nqa_md_langevin_params* __restrict__ params,
                                                                 nqa_md_npt_state* __restrict__ npt,
                                                                 const S* __restrict__ stress, double* __restrict__ cell) {
  const int64_t s = blockIdx.x, begin = chunk_begin[s], end = chunk_begin[s + 1];
  double s_full, s_half;
  md_sum_rows(partials + 2 * begin, end - begin, false, s_full, s_half);
  if (threadIdx.x != 0) return;
  md_npt_bath_update(s_full, states + s, params + s, npt + s, stress + 9 * s, cell + 9 * s);
}

__global__ __launch_bounds__(MD_THREADS) void md_batched_npt_scale_kernel(double* __restrict__ positions,
                                                                           double* __restrict__ velocities,
                                                                           const nqa_md_chunk* __restrict__ chunks,
                                                                           const nqa_md_npt_state* __restrict__ npt) {
  const nqa_md_chunk chunk = chunks[blockIdx.x];
  if ((int)threadIdx.x >= chunk.count) return;
  const int64_t i = chunk.component0 + threadIdx.x;
  const double mu = npt[chunk.system].mu;
  positions[i] = mu * positions[i];
  velocities[i] = velocities[i] / mu;
}

inline int refuse(const char* name, const char* what, int code = NQA_ERR_INVALID) {
  set_error(std::string(name) + ": " + what);
  return code;
}

}  // namespace nqa

extern "C" {

int nqa_md_batched_langevin_step(int32_t force_dtype, const void* forces, const double* masses, double* positions,
                                 double* velocities, double* vel_out, const nqa_md_chunk* chunks, int64_t num_chunks,
                                 const nqa_md_state* states, const nqa_md_langevin_params* params, double* partials, int32_t mode,
                                 nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_md_batched_langevin_step";
  const bool finish_only = (mode & NQA_MD_FINISH_ONLY) != 0;
  if (num_chunks <= 0 || num_chunks > INT32_MAX) return refuse(name, "0 < num_chunks < 2^31");
  if (force_dtype != NQA_F32 && force_dtype != NQA_F64)
    return refuse(name, "force_dtype: forces are float32 or float64", NQA_ERR_UNSUPPORTED);
  if ((mode & ~NQA_MD_FINISH_ONLY) != 0) return refuse(name, "mode: unknown mode bits (NQA_MD_FINISH_ONLY is the only one)");
  if (!forces) return refuse(name, "forces is required");
  if (!masses) return refuse(name, "masses is required");
  if (!velocities) return refuse(name, "velocities is required");
  if (!chunks) return refuse(name, "chunks is required");
  if (!states) return refuse(name, "states is required");
  if (!params) return refuse(name, "params is required");
  if (!partials) return refuse(name, "partials is required");
  if (finish_only && !vel_out) return refuse(name, "vel_out is required in the finish-only mode");
  if (!finish_only && !positions) return refuse(name, "positions is required");
  const dim3 grid((unsigned)num_chunks);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (force_dtype == NQA_F64)
    hipLaunchKernelGGL(md_batched_langevin_step_kernel<double>, grid, dim3(MD_THREADS), 0, s, (const double*)forces, masses,
                       positions, velocities, vel_out, chunks, states, params, partials, (int)finish_only);
  else
    hipLaunchKernelGGL(md_batched_langevin_step_kernel<float>, grid, dim3(MD_THREADS), 0, s, (const float*)forces, masses,
                       positions, velocities, vel_out, chunks, states, params, partials, (int)finish_only);
  return launch_status(name);
}

int nqa_md_batched_bath(const double* partials, const int64_t* chunk_begin, nqa_md_state* states, int64_t num_systems,
                        int32_t mode, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_md_batched_bath";
  if (num_systems <= 0 || num_systems > INT32_MAX) return refuse(name, "0 < num_systems < 2^31");
  if ((mode & ~NQA_MD_FINISH_ONLY) != 0)
    return refuse(name, "mode: unknown mode bits (there is no thermostat bit: Langevin dynamics only)");
  if (!partials) return refuse(name, "partials is required");
  if (!chunk_begin) return refuse(name, "chunk_begin is required");
  if (!states) return refuse(name, "states is required");
  hipLaunchKernelGGL(md_batched_bath_kernel, dim3((unsigned)num_systems), dim3(64), 0, static_cast<hipStream_t>(stream), partials,
                     chunk_begin, states, (int)((mode & NQA_MD_FINISH_ONLY) != 0));
  return launch_status(name);
}

int nqa_md_batched_npt_bath(const double* partials, const int64_t* chunk_begin, nqa_md_state* states,
                            const nqa_md_langevin_params* params, nqa_md_npt_state* npt, int32_t stress_dtype, const void* stress,
                            double* cell, int64_t num_systems, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_md_batched_npt_bath";
  if (num_systems <= 0 || num_systems > INT32_MAX) return refuse(name, "0 < num_systems < 2^31");
  if (stress_dtype != NQA_F32 && stress_dtype != NQA_F64)
    return refuse(name, "stress_dtype: the stress is float32 or float64", NQA_ERR_UNSUPPORTED);
  if (!partials) return refuse(name, "partials is required");
  if (!chunk_begin) return refuse(name, "chunk_begin is required");
  if (!states) return refuse(name, "states is required");
  if (!params) return refuse(name, "params is required");
  if (!npt) return refuse(name, "the npt records are required");
  if (!stress) return refuse(name, "stress ([S, 3, 3]) is required");
  if (!cell) return refuse(name, "cell ([S, 3, 3]) is required");
  const dim3 grid((unsigned)num_systems);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (stress_dtype == NQA_F64)
    hipLaunchKernelGGL(md_batched_npt_bath_kernel<double>, grid, dim3(64), 0, s, partials, chunk_begin, states, params, npt,
                       (const double*)stress, cell);
  else
    hipLaunchKernelGGL(md_batched_npt_bath_kernel<float>, grid, dim3(64), 0, s, partials, chunk_begin, states, params, npt,
                       (const float*)stress, cell);
  return launch_status(name);
}

int nqa_md_batched_npt_scale(double* positions, double* velocities, const nqa_md_chunk* chunks, int64_t num_chunks,
                             const nqa_md_npt_state* npt, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_md_batched_npt_scale";
  if (num_chunks <= 0 || num_chunks > INT32_MAX) return refuse(name, "0 < num_chunks < 2^31");
  if (!positions) return refuse(name, "positions is required");
  if (!velocities) return refuse(name, "velocities is required");
  if (!chunks) return refuse(name, "chunks is required");
  if (!npt) return refuse(name, "the npt records are required");
  hipLaunchKernelGGL(md_batched_npt_scale_kernel, dim3((unsigned)num_chunks), dim3(MD_THREADS), 0,
                     static_cast<hipStream_t>(stream), positions, velocities, chunks, npt);
  return launch_status(name);
}

}  // extern "C"
