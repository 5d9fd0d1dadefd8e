// Variable-cell FIRE: the FIRE of relax.hip over the atoms and the cell together, as ASE's UnitCellFilter under opt.fire.FIRE, with
// the state in device memory, for one system or a batch of independent systems concatenated along the atom axis.
//
// Per system: n atoms, the reference cell C0 (rows = lattice vectors), the deformation gradient D with C = C0 D^T, cell_factor.
// Generalised coordinates (n + 3 rows of 3): q_i = x_i D^-T, carried as state and never re-solved, and Q = cell_factor D.
// Generalised forces, with F the force and sigma the stress at (x, C), V = |det C|:
//   atoms  g_i = F_i D                      (rows of fixed atoms count as zero; a fixed atom keeps q_i, so x_i = q_i D^T follows the cell)
//   cell   W = -V (sigma + pressure I);  G = W D^-T;  hydrostatic: G = (tr G / 3) I;  mask: G = G * mask;
//          constant_volume: tr G / 3 off the diagonal;  G = G / cell_factor
// One step:
//   reduce   over the atoms of a chunk, with the D at which F was evaluated (d_new of the record):
//            P = sum g.v,  FF = sum g.g,  VV = sum v.v,  M = max |g_i|^2
//   decide   merges the chunks in the fixed order; lane 0 forms G, adds its nine components to P, FF, VV (against the cell velocity
//            vd) and its three row norms to M;  then fire_decide of fire_device.h, the decision relax.hip takes (fmax, converged;
//            unless converged cv, cf, dt, a, npos, scale, nsteps += 1), then the cell move by the same lane:
//            d_old = d_new;  vd = cv vd + cf G;  vd = vd + dt G;  Q = cell_factor d_old + scale (dt vd);  d_new = Q / cell_factor
//            C = C0 d_new^T into the [S, 3, 3] float64 cell buffer that the force step reads
//   move     g = F d_old;  v = cv v + cf g;  v = v + dt g;  q = q + scale (dt v);  x = q d_new^T
//
// Layout: the chunks of relax.hip (nqa_fire_chunk, none straddles two systems), one workgroup per chunk and one atom per lane in
// the reduction and in the move (an atom's three components meet in g and in x), one wavefront per system in the decision.  The
// reduction and the move read the nine words of D from the record into registers once per workgroup; the 3 x 3 work (det, D^-T by
// cofactors, the constraints) is plain C++ on lane 0 of the deciding wavefront.
// The record hazard is the one of relax.hip: the second launch rewrites the record, the first and the third read it, so the three
// are three launches on one stream.  No ticket, no atomics, no fence.  No floating-point atomics, a fixed order of every sum, no
// contraction into fused multiply-adds: the same inputs give the same bits, alone and inside a batch.
// LDS: the sixteen wavefront partials of the reduction.  Nothing is read by the host.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "fire_device.h"
#include "launch_status.h"
#include "nequip_amd.h"

#pragma clang fp contract(off)

namespace nqa {

// FIRE_CHUNK, fire_max, fire_block_partials, fire_sum_rows and fire_decide: fire_device.h (shared with relax.hip)
static_assert(sizeof(nqa_cellfire_system) == 512, "the host writes the record as sixty-four 8-byte words");
static_assert(sizeof(nqa_cellfire_system) % 8 == 0, "the record is whole 8-byte words");
static_assert(sizeof(nqa_fire_chunk) == 16, "the host writes a chunk as two 8-byte words");

// row vector times matrix: out_j = a_0 m[0][j] + a_1 m[1][j] + a_2 m[2][j], added left to right
__device__ __forceinline__ void row_times(const double a[3], const double m[9], double out[3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) out[j] = a[0] * m[j] + a[1] * m[3 + j] + a[2] * m[6 + j];
}

// row vector times the transpose: out_j = a_0 m[j][0] + a_1 m[j][1] + a_2 m[j][2], added left to right
__device__ __forceinline__ void row_times_transposed(const double a[3], const double m[9], double out[3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) out[j] = a[0] * m[3 * j] + a[1] * m[3 * j + 1] + a[2] * m[3 * j + 2];
}

template <typename F>
__global__ __launch_bounds__(FIRE_CHUNK) void cellfire_reduce_kernel(const F* __restrict__ forces,
                                                                          const double* __restrict__ velocities,
                                                                          const uint8_t* __restrict__ fixed,
                                                                          const nqa_fire_chunk* __restrict__ chunks,
                                                                          const nqa_cellfire_system* __restrict__ systems,
                                                                          double* __restrict__ partials) {
  const nqa_fire_chunk chunk = chunks[blockIdx.x];
  const int count = chunk.count < FIRE_CHUNK ? chunk.count : FIRE_CHUNK;
  double D[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) D[k] = systems[chunk.system].d_new[k];
  double p = 0.0, ff = 0.0, vv = 0.0;
  if ((int)threadIdx.x < count) {
    const int64_t atom = chunk.atom0 + threadIdx.x;
    if (!(fixed && fixed[atom])) {
      const double f[3] = {(double)forces[3 * atom], (double)forces[3 * atom + 1], (double)forces[3 * atom + 2]};
      double g[3];
      row_times(f, D, g);
      const double vx = velocities[3 * atom], vy = velocities[3 * atom + 1], vz = velocities[3 * atom + 2];
      p = g[0] * vx + g[1] * vy + g[2] * vz;
      ff = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
      vv = vx * vx + vy * vy + vz * vz;
    }
  }
  fire_block_partials(p, ff, vv, partials + 4 * (int64_t)blockIdx.x);
}

template <typename T>
__global__ __launch_bounds__(64) void cellfire_decide_kernel(const double* __restrict__ partials,
                                                             const int64_t* __restrict__ chunk_begin,
                                                             const T* __restrict__ stress,
                                                             nqa_cellfire_system* __restrict__ systems,
                                                             double* __restrict__ cell) {
  double P, FF, VV, M;
  fire_sum_rows(partials, chunk_begin[blockIdx.x], chunk_begin[blockIdx.x + 1], P, FF, VV, M);
  if (threadIdx.x != 0) return;
  nqa_cellfire_system* s = systems + blockIdx.x;

  // the generalised force of the cell, at the D the stress was evaluated at
  double D[9], C0[9], vd[9], G[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    D[k] = s->d_new[k];
    C0[k] = s->c0[k];
    vd[k] = s->vd[k];
  }
  double C[9];  // C = C0 D^T
#pragma unroll
  for (int i = 0; i < 3; ++i) row_times_transposed(C0 + 3 * i, D, C + 3 * i);
  const double detC = C[0] * (C[4] * C[8] - C[5] * C[7]) - C[1] * (C[3] * C[8] - C[5] * C[6]) + C[2] * (C[3] * C[7] - C[4] * C[6]);
  const double V = fabs(detC);
  // cof[i][j] is the cofactor of D[i][j]; D^-1 = cof^T / det D, so D^-T = cof / det D
  double cof[9];
  cof[0] = D[4] * D[8] - D[5] * D[7];
  cof[1] = D[5] * D[6] - D[3] * D[8];
  cof[2] = D[3] * D[7] - D[4] * D[6];
  cof[3] = D[2] * D[7] - D[1] * D[8];
  cof[4] = D[0] * D[8] - D[2] * D[6];
  cof[5] = D[1] * D[6] - D[0] * D[7];
  cof[6] = D[1] * D[5] - D[2] * D[4];
  cof[7] = D[2] * D[3] - D[0] * D[5];
  cof[8] = D[0] * D[4] - D[1] * D[3];
  const double detD = D[0] * cof[0] + D[1] * cof[1] + D[2] * cof[2];
  double DinvT[9], W[9];
  const T* sig = stress + 9 * (int64_t)blockIdx.x;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    DinvT[k] = cof[k] / detD;
    W[k] = (double)sig[k];
  }
  W[0] = W[0] + s->pressure;
  W[4] = W[4] + s->pressure;
  W[8] = W[8] + s->pressure;
#pragma unroll
  for (int k = 0; k < 9; ++k) W[k] = -V * W[k];
  // G = W D^-T:  G[i][j] = sum_k W[i][k] DinvT[k][j]
#pragma unroll
  for (int i = 0; i < 3; ++i) row_times(W + 3 * i, DinvT, G + 3 * i);
  if (s->hydrostatic != 0) {
    const double third = (G[0] + G[4] + G[8]) / 3.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) G[k] = (k % 4 == 0) ? third : 0.0;
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) G[k] = G[k] * s->mask[k];
  if (s->constant_volume != 0) {
    const double third = (G[0] + G[4] + G[8]) / 3.0;
    G[0] = G[0] - third;
    G[4] = G[4] - third;
    G[8] = G[8] - third;
  }
  const double cell_factor = s->cell_factor;
#pragma unroll
  for (int k = 0; k < 9; ++k) G[k] = G[k] / cell_factor;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    P += G[k] * vd[k];
    FF += G[k] * G[k];
    VV += vd[k] * vd[k];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) M = fire_max(M, G[3 * i] * G[3 * i] + G[3 * i + 1] * G[3 * i + 1] + G[3 * i + 2] * G[3 * i + 2]);

  if (!fire_decide(s, P, FF, VV, M)) return;

  // the cell move, with the coefficients the decision just left in the record
  const double cv = s->cv, cf = s->cf, dt = s->dt, scale = s->scale;
  double Dn[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    double w = cv * vd[k] + cf * G[k];
    w = w + dt * G[k];
    double Q = cell_factor * D[k];
    Q = Q + scale * (dt * w);
    Dn[k] = Q / cell_factor;
    s->vd[k] = w;
    s->d_old[k] = D[k];
    s->d_new[k] = Dn[k];
  }
  double* out = cell + 9 * (int64_t)blockIdx.x;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double r[3];
    row_times_transposed(C0 + 3 * i, Dn, r);
    out[3 * i] = r[0];
    out[3 * i + 1] = r[1];
    out[3 * i + 2] = r[2];
  }
}

template <typename F>
__global__ __launch_bounds__(FIRE_CHUNK) void cellfire_move_kernel(const F* __restrict__ forces, double* __restrict__ positions,
                                                                        double* __restrict__ coords,
                                                                        double* __restrict__ velocities,
                                                                        const uint8_t* __restrict__ fixed,
                                                                        const nqa_fire_chunk* __restrict__ chunks,
                                                                        const nqa_cellfire_system* __restrict__ systems) {
  const nqa_fire_chunk chunk = chunks[blockIdx.x];
  const nqa_cellfire_system* s = systems + chunk.system;
  if (s->converged != 0) return;
  const int count = chunk.count < FIRE_CHUNK ? chunk.count : FIRE_CHUNK;
  if ((int)threadIdx.x >= count) return;
  const double cv = s->cv, cf = s->cf, dt = s->dt, scale = s->scale;
  double Do[9], Dn[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    Do[k] = s->d_old[k];
    Dn[k] = s->d_new[k];
  }
  const int64_t atom = chunk.atom0 + threadIdx.x;
  double q[3] = {coords[3 * atom], coords[3 * atom + 1], coords[3 * atom + 2]};
  if (!(fixed && fixed[atom])) {
    const double f[3] = {(double)forces[3 * atom], (double)forces[3 * atom + 1], (double)forces[3 * atom + 2]};
    double g[3];
    row_times(f, Do, g);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double v = cv * velocities[3 * atom + k] + cf * g[k];
      v = v + dt * g[k];
      velocities[3 * atom + k] = v;
      q[k] = q[k] + scale * (dt * v);
      coords[3 * atom + k] = q[k];
    }
  }
  double x[3];
  row_times_transposed(q, Dn, x);
  positions[3 * atom] = x[0];
  positions[3 * atom + 1] = x[1];
  positions[3 * atom + 2] = x[2];
}

}  // namespace nqa

extern "C" {

int nqa_cellfire_reduce(int32_t force_dtype, const void* forces, const double* velocities, const uint8_t* fixed,
                        const nqa_fire_chunk* chunks, int64_t n_chunks, const nqa_cellfire_system* systems, double* partials,
                        nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_cellfire_reduce";
  if (n_chunks <= 0 || n_chunks > INT32_MAX) {
    set_error(std::string(name) + ": 0 < n_chunks < 2^31");
    return NQA_ERR_INVALID;
  }
  if (force_dtype != NQA_F32 && force_dtype != NQA_F64) {
    set_error(std::string(name) + ": forces are float32 or float64");
    return NQA_ERR_UNSUPPORTED;
  }
  if (!forces || !velocities || !chunks || !systems || !partials) {
    set_error(std::string(name) + ": forces, velocities, chunks, systems and partials are required (fixed may be null)");
    return NQA_ERR_INVALID;
  }
  const dim3 grid((unsigned)n_chunks);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (force_dtype == NQA_F64)
    hipLaunchKernelGGL(cellfire_reduce_kernel<double>, grid, dim3(FIRE_CHUNK), 0, s, (const double*)forces, velocities, fixed,
                       chunks, systems, partials);
  else
    hipLaunchKernelGGL(cellfire_reduce_kernel<float>, grid, dim3(FIRE_CHUNK), 0, s, (const float*)forces, velocities, fixed,
                       chunks, systems, partials);
  return launch_status(name);
}

int nqa_cellfire_decide(const double* partials, const int64_t* chunk_begin, int32_t stress_dtype, const void* stress,
                        nqa_cellfire_system* systems, double* cell, int64_t n_systems, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_cellfire_decide";
  if (n_systems <= 0 || n_systems > INT32_MAX) {
    set_error(std::string(name) + ": 0 < n_systems < 2^31");
    return NQA_ERR_INVALID;
  }
  if (stress_dtype != NQA_F32 && stress_dtype != NQA_F64) {
    set_error(std::string(name) + ": the stress is float32 or float64");
    return NQA_ERR_UNSUPPORTED;
  }
  if (!partials || !chunk_begin || !stress || !systems || !cell) {
    set_error(std::string(name) + ": partials, chunk_begin ([n_systems + 1]), stress, systems and cell are required");
    return NQA_ERR_INVALID;
  }
  const dim3 grid((unsigned)n_systems);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (stress_dtype == NQA_F64)
    hipLaunchKernelGGL(cellfire_decide_kernel<double>, grid, dim3(64), 0, s, partials, chunk_begin, (const double*)stress, systems,
                       cell);
  else
    hipLaunchKernelGGL(cellfire_decide_kernel<float>, grid, dim3(64), 0, s, partials, chunk_begin, (const float*)stress, systems,
                       cell);
  return launch_status(name);
}

int nqa_cellfire_move(int32_t force_dtype, const void* forces, double* positions, double* coords, double* velocities,
                      const uint8_t* fixed, const nqa_fire_chunk* chunks, int64_t n_chunks, const nqa_cellfire_system* systems,
                      nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_cellfire_move";
  if (n_chunks <= 0 || n_chunks > INT32_MAX) {
    set_error(std::string(name) + ": 0 < n_chunks < 2^31");
    return NQA_ERR_INVALID;
  }
  if (force_dtype != NQA_F32 && force_dtype != NQA_F64) {
    set_error(std::string(name) + ": forces are float32 or float64");
    return NQA_ERR_UNSUPPORTED;
  }
  if (!forces || !positions || !coords || !velocities || !chunks || !systems) {
    set_error(std::string(name) + ": forces, positions, coords, velocities, chunks and systems are required (fixed may be null)");
    return NQA_ERR_INVALID;
  }
  const dim3 grid((unsigned)n_chunks);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (force_dtype == NQA_F64)
    hipLaunchKernelGGL(cellfire_move_kernel<double>, grid, dim3(FIRE_CHUNK), 0, s, (const double*)forces, positions, coords,
                       velocities, fixed, chunks, systems);
  else
    hipLaunchKernelGGL(cellfire_move_kernel<float>, grid, dim3(FIRE_CHUNK), 0, s, (const float*)forces, positions, coords,
                       velocities, fixed, chunks, systems);
  return launch_status(name);
}

}  // extern "C"
