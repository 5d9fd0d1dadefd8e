// Generic (any irreps, l <= NQA_LMAX) fused gather -> 'uvu' tensor product -> scatter kernels for gfx950.
//
// Replaces TensorProductScatter.forward (nequip/nn/_tp_scatter_base.py:35-38:
//   edge_features = tp(x[edge_src], edge_attr, edge_weight); scatter(edge_features, edge_dst, N))
// and its autograd (tests/unit/nn/test_tp_scatter_kernel.py:160-177) without ever materialising the
// [E, D_in] gather or the [E, D_mid] per-edge product in HBM.
//
// Work decomposition (CDNA4, wave64):
//   * one wavefront per (node, instruction, 64-channel chunk); lanes = channels u, so the per-edge
//     weight row segment w[e, p, u0:u0+64] is one coalesced 256 B read and every lane owns its output
//     accumulators acc[2*l3+1] in VGPRs for the whole neighbour loop;
//   * edges are visited through a CSR built by nqa_csr_build, so the per-node sum is an ordered,
//     atomics-free register accumulation followed by a single store (deterministic);
//   * the Clebsch-Gordan contraction is the generated, fully unrolled sparse code CGT<l1,l2,l3>
//     (literal coefficients; the switch on the path type is wave-uniform);
//   * Y[e,:] and all indices are wave-uniform -> scalar loads / SGPR operands.
// The per-edge operands (w: E*W*4 B) are streamed from HBM exactly once; node rows (x, grad_out) are
// re-read through L2/MALL.  Roofline: HBM-bound.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "generated/cg_generated.h"
#include "plan.h"
#include "tp_spec.h"

namespace nqa {

constexpr int kWavesPerBlock = 4;
constexpr int kBlock = 64 * kWavesPerBlock;

template <typename T>
struct TPArgs {
  // operands (any may be null depending on the kernel)
  const T* __restrict__ x;
  const T* __restrict__ y;
  const T* __restrict__ w;
  const T* __restrict__ g;  // grad_out [N, dim_out]
  T* __restrict__ out;      // fwd: out [N, dim_out]; bwd_x: gx [N, dim_in1]
  T* __restrict__ gw;       // [E, wnumel]
  T* __restrict__ ypart;    // [E, ypart_width]
  // CSR
  const int32_t* __restrict__ rowptr;
  const int32_t* __restrict__ eid;
  const int32_t* __restrict__ nbr;
  // plan tables
  const InstrDev* __restrict__ instr;
  const ChunkDev* __restrict__ chunks;
  const BlkDev* __restrict__ blks;
  const int32_t* __restrict__ blk_instr;
  const XChunkDev* __restrict__ xchunks;
  int32_t n_chunks;
  int32_t n_xchunks;
  int32_t dim_in1, dim_in2, dim_out, wnumel, ypw;
  int64_t n_items;
};

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
template <typename T, int L1, int L2, int L3>
__device__ __forceinline__ void tp_fwd_item(const TPArgs<T>& a, const InstrDev& ins, int node, int u, bool active) {
  constexpr int D1 = 2 * L1 + 1, D2 = 2 * L2 + 1, D3 = 2 * L3 + 1;
  T acc[D3];
#pragma unroll
  for (int k = 0; k < D3; ++k) acc[k] = T(0);
  const int beg = a.rowptr[node], end = a.rowptr[node + 1];
  const T* __restrict__ xb = a.x + ins.x_off + (int64_t)u * ins.x_su;
  const T* __restrict__ wb = a.w + ins.w_off + u;
  const T* __restrict__ yb = a.y + ins.y_off;
  const int x_sm = ins.x_sm;
  for (int idx = beg; idx < end; ++idx) {
    const int e = a.eid[idx];
    const int s = a.nbr[idx];
    T yv[D2];
#pragma unroll
    for (int j = 0; j < D2; ++j) yv[j] = yb[(int64_t)e * a.dim_in2 + j];
    T xv[D1];
    T wv = T(0);
    if (active) {
      const T* __restrict__ xr = xb + (int64_t)s * a.dim_in1;
#pragma unroll
      for (int i = 0; i < D1; ++i) xv[i] = xr[i * x_sm];
      wv = wb[(int64_t)e * a.wnumel];
    } else {
#pragma unroll
      for (int i = 0; i < D1; ++i) xv[i] = T(0);
    }
    T t[D3];
    CGT<L1, L2, L3>::template ab_c<T>(xv, yv, t);
#pragma unroll
    for (int k = 0; k < D3; ++k) acc[k] += wv * t[k];
  }
  if (active) {
    T* __restrict__ ob = a.out + (int64_t)node * a.dim_out + ins.o_off + (int64_t)u * ins.o_su;
    const T c = (T)ins.coeff;
    if (ins.shared_out) {
#pragma unroll
      for (int k = 0; k < D3; ++k) atomicAdd(ob + k * ins.o_sm, c * acc[k]);
    } else {
#pragma unroll
      for (int k = 0; k < D3; ++k) ob[k * ins.o_sm] = c * acc[k];
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void tp_fwd_kernel(const TPArgs<T> a) {
  const int lane = threadIdx.x & 63;
  const int64_t item =
      (int64_t)blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (item >= a.n_items) return;
  const int node = (int)(item / a.n_chunks);
  const int c = (int)(item - (int64_t)node * a.n_chunks);
  const ChunkDev ch = a.chunks[c];
  const InstrDev ins = a.instr[ch.instr];
  const int u = ch.u0 + lane;
  const bool active = u < ins.mul;
#define NQA_CALL(l1, l2, l3) tp_fwd_item<T, l1, l2, l3>(a, ins, node, u, active)
  NQA_DISPATCH_L123(ins.type, NQA_CALL)
#undef NQA_CALL
}

// ------------------------------------------------------------------------------------------------
// backward w.r.t. per-edge operands (weights, edge attributes)
// ------------------------------------------------------------------------------------------------
template <typename T, int L1, int L2, int L3>
__device__ __forceinline__ void tp_bwd_edge_item(const TPArgs<T>& a, const InstrDev& ins, const ChunkDev& ch,
                                                 int node, int u, bool active, int lane) {
  constexpr int D1 = 2 * L1 + 1, D2 = 2 * L2 + 1, D3 = 2 * L3 + 1;
  // grad_out row of this node is shared by all of its edges: keep it (pre-scaled) in registers
  T gv[D3];
  if (active) {
    const T* __restrict__ gb = a.g + (int64_t)node * a.dim_out + ins.o_off + (int64_t)u * ins.o_su;
    const T c = (T)ins.coeff;
#pragma unroll
    for (int k = 0; k < D3; ++k) gv[k] = c * gb[k * ins.o_sm];
  } else {
#pragma unroll
    for (int k = 0; k < D3; ++k) gv[k] = T(0);
  }
  const int beg = a.rowptr[node], end = a.rowptr[node + 1];
  const T* __restrict__ xb = a.x + ins.x_off + (int64_t)u * ins.x_su;
  const T* __restrict__ yb = a.y + ins.y_off;
  const bool need_gw = a.gw != nullptr;
  const bool need_gy = a.ypart != nullptr;
  const int x_sm = ins.x_sm;
  for (int idx = beg; idx < end; ++idx) {
    const int e = a.eid[idx];
    const int s = a.nbr[idx];
    T xv[D1];
    if (active) {
      const T* __restrict__ xr = xb + (int64_t)s * a.dim_in1;
#pragma unroll
      for (int i = 0; i < D1; ++i) xv[i] = xr[i * x_sm];
    } else {
#pragma unroll
      for (int i = 0; i < D1; ++i) xv[i] = T(0);
    }
    if (need_gw) {
      T yv[D2];
#pragma unroll
      for (int j = 0; j < D2; ++j) yv[j] = yb[(int64_t)e * a.dim_in2 + j];
      T t[D3];
      CGT<L1, L2, L3>::template ab_c<T>(xv, yv, t);
      T r = T(0);
#pragma unroll
      for (int k = 0; k < D3; ++k) r += t[k] * gv[k];
      if (active) a.gw[(int64_t)e * a.wnumel + ins.w_off + u] = r;
    }
    if (need_gy) {
      const T wv = active ? a.w[(int64_t)e * a.wnumel + ins.w_off + u] : T(0);
      T q[D2];
      CGT<L1, L2, L3>::template ac_b<T>(xv, gv, q);
      T* __restrict__ yp = a.ypart + (int64_t)e * a.ypw + ch.ypart_off;
#pragma unroll
      for (int j = 0; j < D2; ++j) {
        const T r = wave_sum(q[j] * wv);
        if (lane == 0) yp[j] = r;
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void tp_bwd_edge_kernel(const TPArgs<T> a) {
  const int lane = threadIdx.x & 63;
  const int64_t item =
      (int64_t)blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (item >= a.n_items) return;
  const int node = (int)(item / a.n_chunks);
  const int c = (int)(item - (int64_t)node * a.n_chunks);
  const ChunkDev ch = a.chunks[c];
  const InstrDev ins = a.instr[ch.instr];
  const int u = ch.u0 + lane;
  const bool active = u < ins.mul;
#define NQA_CALL(l1, l2, l3) tp_bwd_edge_item<T, l1, l2, l3>(a, ins, ch, node, u, active, lane)
  NQA_DISPATCH_L123(ins.type, NQA_CALL)
#undef NQA_CALL
}

// gy[e, s] = sum of the per-(instruction, chunk) partial columns mapped to component s
template <typename T>
__global__ __launch_bounds__(256) void tp_ypart_reduce_kernel(const T* __restrict__ ypart, T* __restrict__ gy,
                                                              const int32_t* __restrict__ ycol_ptr,
                                                              const int32_t* __restrict__ ycol_idx, int32_t dim_in2,
                                                              int32_t ypw, int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int64_t e = t / dim_in2;
  const int s = (int)(t - e * dim_in2);
  T r = T(0);
  for (int c = ycol_ptr[s]; c < ycol_ptr[s + 1]; ++c) r += ypart[e * ypw + ycol_idx[c]];
  gy[t] = r;
}

// ------------------------------------------------------------------------------------------------
// backward w.r.t. node features: scatter over src (transposed CSR)
// ------------------------------------------------------------------------------------------------
template <typename T, int L1, int L2, int L3>
__device__ __forceinline__ void tp_bwd_x_path(const TPArgs<T>& a, const InstrDev& ins, int node, int u, bool active,
                                              T* __restrict__ acc) {
  constexpr int D1 = 2 * L1 + 1, D2 = 2 * L2 + 1, D3 = 2 * L3 + 1;
  const int beg = a.rowptr[node], end = a.rowptr[node + 1];
  const T* __restrict__ yb = a.y + ins.y_off;
  const T* __restrict__ gb = a.g + ins.o_off + (int64_t)u * ins.o_su;
  const T* __restrict__ wb = a.w + ins.w_off + u;
  const T c = (T)ins.coeff;
  const int o_sm = ins.o_sm;
  for (int idx = beg; idx < end; ++idx) {
    const int e = a.eid[idx];
    const int d = a.nbr[idx];
    T yv[D2];
#pragma unroll
    for (int j = 0; j < D2; ++j) yv[j] = yb[(int64_t)e * a.dim_in2 + j];
    T gv[D3];
    T wv = T(0);
    if (active) {
      const T* __restrict__ gr = gb + (int64_t)d * a.dim_out;
#pragma unroll
      for (int k = 0; k < D3; ++k) gv[k] = gr[k * o_sm];
      wv = c * wb[(int64_t)e * a.wnumel];
    } else {
#pragma unroll
      for (int k = 0; k < D3; ++k) gv[k] = T(0);
    }
    T t[D1];
    CGT<L1, L2, L3>::template bc_a<T>(yv, gv, t);
#pragma unroll
    for (int i = 0; i < D1; ++i) acc[i] += wv * t[i];
  }
}

template <typename T, int L1>
__device__ __forceinline__ void tp_bwd_x_store(const TPArgs<T>& a, const BlkDev& b, int node, int u, bool active,
                                               const T* __restrict__ acc) {
  if (!active) return;
  T* __restrict__ ob = a.out + (int64_t)node * a.dim_in1 + b.x_off + (int64_t)u * b.x_su;
#pragma unroll
  for (int i = 0; i < 2 * L1 + 1; ++i) ob[i * b.x_sm] = acc[i];
}

template <typename T>
__global__ __launch_bounds__(kBlock) void tp_bwd_x_kernel(const TPArgs<T> a) {
  const int lane = threadIdx.x & 63;
  const int64_t item =
      (int64_t)blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (item >= a.n_items) return;
  const int node = (int)(item / a.n_xchunks);
  const int c = (int)(item - (int64_t)node * a.n_xchunks);
  const XChunkDev xc = a.xchunks[c];
  const BlkDev b = a.blks[xc.blk];
  const int u = xc.u0 + lane;
  const bool active = u < b.mul;
  T acc[2 * NQA_LMAX + 1];
#pragma unroll
  for (int i = 0; i < 2 * NQA_LMAX + 1; ++i) acc[i] = T(0);
  for (int q = b.instr_begin; q < b.instr_end; ++q) {
    const InstrDev ins = a.instr[a.blk_instr[q]];
#define NQA_CALL(l1, l2, l3) tp_bwd_x_path<T, l1, l2, l3>(a, ins, node, u, active, acc)
    NQA_DISPATCH_L123(ins.type, NQA_CALL)
#undef NQA_CALL
  }
#define NQA_CALL(l1) tp_bwd_x_store<T, l1>(a, b, node, u, active, acc)
  NQA_DISPATCH_L(b.l, NQA_CALL)
#undef NQA_CALL
}

// ------------------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------------------
static int check_launch(const char* what) {
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    set_error(std::string(what) + ": " + hipGetErrorString(err));
    return NQA_ERR_LAUNCH;
  }
  return NQA_OK;
}

static int grid_for(int64_t items, unsigned* grid) {
  const int64_t blocks = (items + kWavesPerBlock - 1) / kWavesPerBlock;
  if (blocks > 2147483647LL) {
    set_error("problem too large for a single launch");
    return NQA_ERR_UNSUPPORTED;
  }
  *grid = (unsigned)blocks;
  return NQA_OK;
}

// The operands of one call as the C ABI hands them over; a kernel family reads the ones it needs, the rest stay NULL.
struct Values {
  const void *x, *y, *w, *g;
};
struct EdgeCsr {  // edges grouped by node: nqa_csr_build's (rowptr, edge id per slot, the other node per slot)
  const int32_t *rowptr, *eid, *nbr;
};
struct PairedRows {  // nqa_tp_scatter_*_paired: the weight row of every CSR slot, w has num_pairs rows
  const int32_t* rows;
  int64_t num_pairs;
};
struct OwnerCsr {  // nqa_pair_owner_lists: pairs grouped by their owner node
  const int32_t *rowptr, *other, *row, *edge_in, *edge_out;
};

// ---- generic (any irreps) kernels ----
template <typename T>
static TPArgs<T> generic_args(const nqa_plan* P, const void* image, const Values& v, const EdgeCsr& c) {
  TPArgs<T> a{};
  const char* base = static_cast<const char*>(image);
  a.instr = reinterpret_cast<const InstrDev*>(base + P->layout.off_instr);
  a.chunks = reinterpret_cast<const ChunkDev*>(base + P->layout.off_chunks);
  a.blks = reinterpret_cast<const BlkDev*>(base + P->layout.off_blks);
  a.blk_instr = reinterpret_cast<const int32_t*>(base + P->layout.off_blk_instr);
  a.xchunks = reinterpret_cast<const XChunkDev*>(base + P->layout.off_xchunks);
  a.n_chunks = (int32_t)P->chunks.size();
  a.n_xchunks = (int32_t)P->xchunks.size();
  a.dim_in1 = P->dim_in1;
  a.dim_in2 = P->dim_in2;
  a.dim_out = P->dim_out;
  a.wnumel = P->weight_numel;
  a.ypw = P->ypart_width;
  a.x = static_cast<const T*>(v.x);
  a.y = static_cast<const T*>(v.y);
  a.w = static_cast<const T*>(v.w);
  a.g = static_cast<const T*>(v.g);
  a.rowptr = c.rowptr;
  a.eid = c.eid;
  a.nbr = c.nbr;
  return a;
}

// f(T{}) with T the element type of `dtype` (checked by check_common)
template <typename F>
static int by_dtype(int32_t dtype, F&& f) {
  return dtype == NQA_F32 ? f(float{}) : f(double{});
}

template <typename T>
static int launch_fwd(TPArgs<T> a, void* out, int64_t N, hipStream_t stream) {
  a.out = static_cast<T*>(out);
  a.n_items = N * (int64_t)a.n_chunks;
  if (a.n_items == 0) return NQA_OK;
  unsigned grid;
  int rc = grid_for(a.n_items, &grid);
  if (rc != NQA_OK) return rc;
  hipLaunchKernelGGL(tp_fwd_kernel<T>, dim3(grid), dim3(kBlock), 0, stream, a);
  return check_launch("nqa_tp_scatter_fwd");
}

template <typename T>
static int launch_bwd_edge(TPArgs<T> a, const nqa_plan* P, const void* image, void* gw, void* gy, void* workspace,
                           int64_t N, int64_t E, hipStream_t stream) {
  a.gw = static_cast<T*>(gw);
  a.ypart = gy ? static_cast<T*>(workspace) : nullptr;
  a.n_items = N * (int64_t)a.n_chunks;
  if (a.n_items > 0 && E > 0) {
    unsigned grid;
    int rc = grid_for(a.n_items, &grid);
    if (rc != NQA_OK) return rc;
    hipLaunchKernelGGL(tp_bwd_edge_kernel<T>, dim3(grid), dim3(kBlock), 0, stream, a);
    rc = check_launch("nqa_tp_scatter_bwd_edge");
    if (rc != NQA_OK) return rc;
  }
  if (gy && E > 0 && P->dim_in2 > 0) {
    const char* base = static_cast<const char*>(image);
    const int64_t total = E * (int64_t)P->dim_in2;
    const int64_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(tp_ypart_reduce_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, stream,
                       static_cast<const T*>(workspace), static_cast<T*>(gy),
                       reinterpret_cast<const int32_t*>(base + P->layout.off_ycol_ptr),
                       reinterpret_cast<const int32_t*>(base + P->layout.off_ycol_idx), P->dim_in2,
                       P->ypart_width, total);
    return check_launch("nqa_tp_scatter_bwd_edge(reduce)");
  }
  return NQA_OK;
}

template <typename T>
static int launch_bwd_x(TPArgs<T> a, void* gx, int64_t N, hipStream_t stream) {
  a.out = static_cast<T*>(gx);
  a.n_items = N * (int64_t)a.n_xchunks;
  if (a.n_items == 0) return NQA_OK;
  unsigned grid;
  int rc = grid_for(a.n_items, &grid);
  if (rc != NQA_OK) return rc;
  hipLaunchKernelGGL(tp_bwd_x_kernel<T>, dim3(grid), dim3(kBlock), 0, stream, a);
  return check_launch("nqa_tp_scatter_bwd_x");
}

// ---- structure-specialised ("edge-outer") kernels: used for float32 when prebuilt for the plan's structure ----
// Switches (env_flag / env_int of plan.h).  Each one's policy:
//   NQA_FORCE_GENERIC     once per process: the tests and the Python side's cached queries rely on one answer per plan
//                         (env_set: on for any value but "" or a leading '0', as the tests' own reading of it)
//   NQA_SPEC_MASKED=1     once per process: the exec-masked instantiations for partial channel chunks
//   NQA_SPEC_WPN=1|4      every call: a test forces the large-box launch shape on a box the oracle can evaluate
//   NQA_PAIR_RING=0       every call: the tests switch between the pair kernels within one process (pair_form)
//   NQA_PAIR_GX_ATOMIC=0  every call: likewise (pair_form)
static bool force_generic() {
  static const bool v = env_set("NQA_FORCE_GENERIC");
  return v;
}
static bool spec_masked() {
  static const bool v = env_flag("NQA_SPEC_MASKED", false);
  return v;
}

static bool use_spec(const nqa_plan* P, int32_t dtype) {
  return P->spec != nullptr && dtype == NQA_F32 && !force_generic();
}

static int spec_chunks(const nqa_plan* P) { return (P->uniform_mul + 63) / 64; }

static int spec_wpn(const nqa_plan* P, int64_t N) {
  // few (node, chunk) items -> split each node's edges over 4 wavefronts to fill the 256 CUs
  const int64_t items = N * (int64_t)spec_chunks(P);
  // experiment / test switch: 1 or 4 wavefronts per (node, chunk); measured: 4 wins at cfg-3 (2 was tried: slower)
  const int forced = env_int("NQA_SPEC_WPN", 0);
  if (forced == 1 || forced == 4) return forced;
  return items < 49152 ? 4 : 1;
}

// The structure's launcher with this call's choices; `ring` is pair_form's (only BwdPairs reads it).
static int spec_launch(const nqa_plan* P, SpecKernel which, const SpecArgs<float>& a, hipStream_t stream, bool ring = false) {
  const bool sums = which == SpecKernel::RowsSumSrc || which == SpecKernel::RowsSumPairs || which == SpecKernel::AccFinish;
  return P->spec->launch(which, SpecLaunchOpts{sums ? 1 : spec_wpn(P, a.N), ring, spec_masked()}, a, stream);
}

__global__ __launch_bounds__(256) void spec_gy_reduce_kernel(const float* __restrict__ part, float* __restrict__ gy,
                                                             int32_t S, int32_t nchunk, int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int64_t e = t / S;
  const int j = (int)(t - e * S);
  float r = 0.f;
  for (int c = 0; c < nchunk; ++c) r += part[e * (int64_t)(nchunk * S) + c * S + j];
  gy[t] = r;
}

static SpecArgs<float> spec_node_operands(const nqa_plan* P, int64_t N) {
  SpecArgs<float> a{};
  a.N = (int32_t)N;
  a.mul = P->uniform_mul;
  a.din = P->dim_in1;
  a.dout = P->dim_out;
  a.wn = P->weight_numel;
  a.gy_stride = P->dim_in2;
  return a;
}

// The operands every edge kernel reads.  The only place that decides which row of w / grad_w a CSR slot uses: its own
// edge's, or with paired weights the row `paired->rows` names (SpecArgs::wid / wP).
static SpecArgs<float> spec_edge_operands(const nqa_plan* P, int64_t N, const Values& v, const EdgeCsr& c,
                                          const PairedRows* paired) {
  SpecArgs<float> a = spec_node_operands(P, N);
  a.x = static_cast<const float*>(v.x);
  a.y = static_cast<const float*>(v.y);
  a.w = static_cast<const float*>(v.w);
  a.g = static_cast<const float*>(v.g);
  a.rowptr = c.rowptr;
  a.eid = c.eid;
  a.nbr = c.nbr;
  a.wid = paired ? paired->rows : c.eid;
  a.wP = paired ? (int32_t)paired->num_pairs : INT32_MAX;
  return a;
}

// Owner-CSR variant (pair-centric kernels): a slot is a pair, its weight row is the pair's own (no second half: wP stays
// INT32_MAX), eid / eid2 are its two directed edges.
static SpecArgs<float> spec_owner_operands(const nqa_plan* P, int64_t N, const Values& v, const OwnerCsr& c) {
  const PairedRows own_rows{c.row, INT32_MAX};
  SpecArgs<float> a = spec_edge_operands(P, N, v, EdgeCsr{c.rowptr, c.edge_in, c.other}, &own_rows);
  a.eid2 = c.edge_out;
  return a;
}

// ---- workspace: [grad_y partial rows | pad to 256 B | per-edge (fused) or per-pair (pairs) grad_x rows] ----
enum class TpWs { Edge, Fused, Pairs };
struct TpWsLayout {
  int64_t total;      // bytes; -1: this plan / dtype / edge count has no such kernel
  int32_t nchunk;     // grad_y partials per edge that the specialised kernels write (1: straight into grad_y)
  int32_t gy_stride;  // floats per edge of the partial rows
  int64_t gxe_off;    // byte offset of the grad_x rows (Fused, Pairs)
};

static TpWsLayout tp_ws_layout(const nqa_plan* plan, int32_t dtype, TpWs kind, int64_t num_edges) {
  TpWsLayout l{-1, 1, 0, 0};
  if (plan == nullptr || num_edges < 0) return l;
  const bool spec = use_spec(plan, dtype);
  if (kind != TpWs::Edge && !spec) return l;
  if (kind == TpWs::Pairs && ((num_edges & 1) || !plan->spec->pair)) return l;
  if (spec) {
    // (the split pair kernel: one partial per channel chunk and input-block part)
    l.nchunk = spec_chunks(plan) * (kind == TpWs::Pairs ? plan->spec->pair : 1);
    l.gy_stride = plan->dim_in2 * l.nchunk;
  }
  if (kind == TpWs::Edge) {
    // generic kernels: one partial per (instruction, 64-channel chunk) and component of its in2 irrep (ypart_width);
    // structure-specialised kernels: dim_in2 partials per channel chunk.  The larger of the two: for a structure with few
    // paths the second exceeds the first (one 0e x 0e path, l_max = 1 harmonics, 128 channels: 8 floats per edge against
    // 2) -- found when the truncated-input structures of the channel segments were added; no round-2 structure hit it.
    const int64_t per_edge = std::max<int64_t>(plan->ypart_width, spec ? l.gy_stride : 0);
    l.total = num_edges * per_edge * (dtype == NQA_F64 ? 8 : 4);
    return l;
  }
  const int64_t ypart = l.nchunk > 1 ? num_edges * (int64_t)l.gy_stride * 4 : 0;
  const int64_t rows = kind == TpWs::Pairs ? num_edges / 2 : num_edges;
  l.gxe_off = (ypart + 255) & ~(int64_t)255;
  l.total = l.gxe_off + rows * (int64_t)plan->dim_in1 * 4;
  return l;
}

struct TpWsView {
  float* ypart;
  float* gxe;
};
static TpWsView tp_ws_view(void* workspace, const TpWsLayout& l) {
  return {static_cast<float*>(workspace), reinterpret_cast<float*>(static_cast<char*>(workspace) + l.gxe_off)};
}

// ---- grad_y of the specialised kernels ----
enum class GyMode {
  Direct,   // one partial per edge: the kernel writes grad_y itself
  Partial,  // nchunk partial rows per edge in the workspace, summed by spec_gy_reduce_kernel (finish_gy)
  Atomic,   // the ring pair kernels add every partial to the zeroed grad_y
};

static void route_gy(SpecArgs<float>& a, const TpWsLayout& l, void* grad_y, void* workspace, GyMode mode) {
  if (mode == GyMode::Partial) {
    a.gy = tp_ws_view(workspace, l).ypart;
    a.gy_stride = l.gy_stride;
  } else {
    a.gy = static_cast<float*>(grad_y);
    a.gy_atomic = mode == GyMode::Atomic;
  }
}

static int finish_gy(const nqa_plan* plan, const TpWsLayout& l, void* grad_y, void* workspace, GyMode mode,
                     int64_t num_edges, const char* label, hipStream_t s) {
  if (mode != GyMode::Partial || num_edges == 0) return NQA_OK;
  const int64_t total = num_edges * (int64_t)plan->dim_in2;
  hipLaunchKernelGGL(spec_gy_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                     tp_ws_view(workspace, l).ypart, static_cast<float*>(grad_y), plan->dim_in2, l.nchunk, total);
  return check_launch(label);
}

// ---- which pair-centric backward runs ----
// Decided here, once per call, for the host (the two memsets, SpecArgs::gx_atomic / gy_atomic) AND the launcher
// (SpecLaunchOpts::ring), so the accumulator forms cannot be asked of a kernel that was not selected.
//   R = NQA_PAIR_RING is not 0, A = NQA_PAIR_GX_ATOMIC is not 0, ring = the structure's SpecEntry::ring
//   fits = (mul & 63) == 0 && E / 2 >= N    (ring kernels take whole 64-channel chunks; the accumulator [N, dim_in1] lives in
//                                            the rows' workspace [E / 2, dim_in1] -- every list this is worth running on)
//   ring  R  A  fits | grad_x accumulator (when grad_x is wanted)       | grad_y accumulated (when nchunk > 1 and E > 0)
//    0    .  .   .   | no                                               | no
//    1    1  1   1   | yes (LDS-ring kernel)                            | yes
//    2    1  1   1   | yes (split ring kernel)                          | yes when grad_x is wanted (else the plain split
//                    |                                                  |   kernel runs: partial rows)
//    2    0  1   1   | yes (the plain split kernel has the form itself) | no
//    otherwise       | no (rows, summed in a fixed order)               | no (partial rows + reduce, or direct)
struct PairForm {
  bool ring, gx_atomic, gy_atomic;
};
static PairForm pair_form(const nqa_plan* plan, const TpWsLayout& l, int64_t N, int64_t E, bool want_gx) {
  const bool R = env_flag("NQA_PAIR_RING", true), A = env_flag("NQA_PAIR_GX_ATOMIC", true);
  const int ring = plan->spec->ring;
  const bool fits = (plan->uniform_mul & 63) == 0 && E / 2 >= N;
  const bool acc = A && fits && (ring == 2 || (ring == 1 && R));
  const bool many = l.nchunk > 1 && E > 0;  // (the caller's layout: the nchunk that route_gy uses)
  return {R, acc && want_gx, acc && R && many && (ring == 1 || want_gx)};
}

static int check_common(const nqa_plan* P, const void* image, int32_t dtype, const char* fn) {
  if (P == nullptr || image == nullptr) {
    set_error(std::string(fn) + ": NULL plan or plan image");
    return NQA_ERR_INVALID;
  }
  if (dtype != NQA_F32 && dtype != NQA_F64) {
    set_error(std::string(fn) + ": unsupported dtype");
    return NQA_ERR_UNSUPPORTED;
  }
  return NQA_OK;
}

static int fail(int code, const char* fn, const char* what) {
  set_error(std::string(fn) + what);
  return code;
}
static const char kNullOperand[] = ": NULL operand";
static const char kNoSpec[] = ": no structure-specialised float32 kernel for this plan";
static const char kNoSpecPaired[] = "_paired: no structure-specialised float32 kernel for this plan";
static const char kWorkspace[] = ": workspace missing or too small";

static int check_paired(const char* fn, const int32_t* rows, int64_t num_pairs) {
  if (rows == nullptr || num_pairs <= 0 || num_pairs > 1073741823)
    return fail(NQA_ERR_INVALID, fn, "_paired: weight_rows / num_pairs missing or out of range");
  return NQA_OK;
}

// ---- one driver per family; `paired` is NULL for the per-edge weights ----
static int tp_fwd(const nqa_plan* plan, const void* image, int32_t dtype, const Values& v, const EdgeCsr& dst, void* out,
                  int64_t N, int64_t E, const PairedRows* paired, hipStream_t s) {
  const char* fn = "nqa_tp_scatter_fwd";
  int rc = check_common(plan, image, dtype, fn);
  if (rc != NQA_OK) return rc;
  if (N < 0 || E < 0 || (N > 0 && (!out || !dst.rowptr)) || (E > 0 && (!v.x || !v.y || !v.w || !dst.eid || !dst.nbr)))
    return fail(NQA_ERR_INVALID, fn, kNullOperand);
  if (use_spec(plan, dtype)) {
    if (N == 0) return NQA_OK;
    SpecArgs<float> a = spec_edge_operands(plan, N, v, dst, paired);
    a.out = static_cast<float*>(out);
    spec_launch(plan, SpecKernel::Fwd, a, s);
    return check_launch("nqa_tp_scatter_fwd(spec)");
  }
  if (paired != nullptr) return fail(NQA_ERR_UNSUPPORTED, fn, kNoSpecPaired);
  return by_dtype(dtype, [&](auto t) { return launch_fwd(generic_args<decltype(t)>(plan, image, v, dst), out, N, s); });
}

static int tp_bwd_edge(const nqa_plan* plan, const void* image, int32_t dtype, const Values& v, const EdgeCsr& dst,
                       void* grad_w, void* grad_y, void* workspace, int64_t workspace_bytes, int64_t N, int64_t E,
                       const PairedRows* paired, hipStream_t s) {
  const char* fn = "nqa_tp_scatter_bwd_edge";
  int rc = check_common(plan, image, dtype, fn);
  if (rc != NQA_OK) return rc;
  if (grad_w == nullptr && grad_y == nullptr) return NQA_OK;
  if (E > 0 && (!v.x || !v.y || !v.w || !v.g || !dst.rowptr || !dst.eid || !dst.nbr))
    return fail(NQA_ERR_INVALID, fn, kNullOperand);
  const TpWsLayout l = tp_ws_layout(plan, dtype, TpWs::Edge, E);
  if (grad_y != nullptr && E > 0 && (workspace == nullptr || workspace_bytes < l.total))
    return fail(NQA_ERR_WORKSPACE, fn, kWorkspace);
  if (use_spec(plan, dtype)) {
    if (N == 0 || E == 0) return NQA_OK;
    SpecArgs<float> a = spec_edge_operands(plan, N, v, dst, paired);
    a.gw = static_cast<float*>(grad_w);
    const GyMode mode = l.nchunk == 1 || grad_y == nullptr ? GyMode::Direct : GyMode::Partial;
    route_gy(a, l, grad_y, workspace, mode);
    spec_launch(plan, SpecKernel::BwdEdge, a, s);
    rc = check_launch("nqa_tp_scatter_bwd_edge(spec)");
    if (rc != NQA_OK) return rc;
    return finish_gy(plan, l, grad_y, workspace, mode, E, "nqa_tp_scatter_bwd_edge(spec reduce)", s);
  }
  if (paired != nullptr) return fail(NQA_ERR_UNSUPPORTED, fn, kNoSpecPaired);
  return by_dtype(dtype, [&](auto t) {
    return launch_bwd_edge(generic_args<decltype(t)>(plan, image, v, dst), plan, image, grad_w, grad_y, workspace, N, E, s);
  });
}

static int tp_bwd_fused(const nqa_plan* plan, const void* image, int32_t dtype, const Values& v, const EdgeCsr& dst,
                        const EdgeCsr& src, void* grad_w, void* grad_y, void* grad_x, void* workspace,
                        int64_t workspace_bytes, int64_t N, int64_t E, const PairedRows* paired, hipStream_t s) {
  const char* fn = "nqa_tp_scatter_bwd_fused";
  int rc = check_common(plan, image, dtype, fn);
  if (rc != NQA_OK) return rc;
  if (!use_spec(plan, dtype)) return fail(NQA_ERR_UNSUPPORTED, fn, kNoSpec);
  if ((N > 0 && (!grad_x || !dst.rowptr || !src.rowptr)) ||
      (E > 0 && (!v.x || !v.y || !v.w || !v.g || !dst.eid || !dst.nbr || !src.eid || !grad_w || !grad_y)))
    return fail(NQA_ERR_INVALID, fn, kNullOperand);
  const TpWsLayout l = tp_ws_layout(plan, dtype, TpWs::Fused, E);
  if (E > 0 && (workspace == nullptr || workspace_bytes < l.total)) return fail(NQA_ERR_WORKSPACE, fn, kWorkspace);
  if (N == 0) return NQA_OK;
  float* gxe = tp_ws_view(workspace, l).gxe;
  if (E > 0) {
    SpecArgs<float> a = spec_edge_operands(plan, N, v, dst, paired);
    a.gw = static_cast<float*>(grad_w);
    a.gxe = gxe;
    const GyMode mode = l.nchunk == 1 ? GyMode::Direct : GyMode::Partial;
    route_gy(a, l, grad_y, workspace, mode);
    spec_launch(plan, SpecKernel::BwdEdge, a, s);
    rc = check_launch("nqa_tp_scatter_bwd_fused(edge)");
    if (rc != NQA_OK) return rc;
    rc = finish_gy(plan, l, grad_y, workspace, mode, E, "nqa_tp_scatter_bwd_fused(reduce)", s);
    if (rc != NQA_OK) return rc;
  }
  SpecArgs<float> b = spec_node_operands(plan, N);
  b.gxe = gxe;
  b.out = static_cast<float*>(grad_x);
  b.rowptr = src.rowptr;
  b.eid = src.eid;
  spec_launch(plan, SpecKernel::RowsSumSrc, b, s);
  return check_launch("nqa_tp_scatter_bwd_fused(sum)");
}

static int tp_bwd_x(const nqa_plan* plan, const void* image, int32_t dtype, const Values& v, const EdgeCsr& src,
                    void* grad_x, int64_t N, int64_t E, const PairedRows* paired, hipStream_t s) {
  const char* fn = "nqa_tp_scatter_bwd_x";
  int rc = check_common(plan, image, dtype, fn);
  if (rc != NQA_OK) return rc;
  if ((N > 0 && (!grad_x || !src.rowptr)) || (E > 0 && (!v.y || !v.w || !v.g || !src.eid || !src.nbr)))
    return fail(NQA_ERR_INVALID, fn, kNullOperand);
  if (use_spec(plan, dtype)) {
    if (N == 0) return NQA_OK;
    SpecArgs<float> a = spec_edge_operands(plan, N, v, src, paired);
    a.out = static_cast<float*>(grad_x);
    spec_launch(plan, SpecKernel::BwdX, a, s);
    return check_launch("nqa_tp_scatter_bwd_x(spec)");
  }
  if (paired != nullptr) return fail(NQA_ERR_UNSUPPORTED, fn, kNoSpecPaired);
  return by_dtype(dtype, [&](auto t) { return launch_bwd_x(generic_args<decltype(t)>(plan, image, v, src), grad_x, N, s); });
}

}  // namespace nqa

using namespace nqa;

extern "C" {

int64_t nqa_tp_bwd_edge_workspace_bytes(const nqa_plan* plan, int32_t dtype, int64_t num_edges) {
  return tp_ws_layout(plan, dtype, TpWs::Edge, num_edges).total;
}

int64_t nqa_tp_bwd_fused_workspace_bytes(const nqa_plan* plan, int32_t dtype, int64_t num_edges) {
  return tp_ws_layout(plan, dtype, TpWs::Fused, num_edges).total;
}

int64_t nqa_tp_bwd_pairs_workspace_bytes(const nqa_plan* plan, int32_t dtype, int64_t num_edges) {
  return tp_ws_layout(plan, dtype, TpWs::Pairs, num_edges).total;
}

int nqa_tp_scatter_fwd(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x, const void* y,
                       const void* w, const int32_t* rowptr_dst, const int32_t* edge_id_dst,
                       const int32_t* src_sorted, void* out, int64_t num_nodes, int64_t num_edges,
                       nqa_stream stream) {
  return tp_fwd(plan, plan_image, dtype, {x, y, w, nullptr}, {rowptr_dst, edge_id_dst, src_sorted}, out, num_nodes,
                num_edges, nullptr, static_cast<hipStream_t>(stream));
}

int nqa_tp_scatter_fwd_paired(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x, const void* y,
                              const void* w, const int32_t* rowptr_dst, const int32_t* edge_id_dst,
                              const int32_t* src_sorted, void* out, int64_t num_nodes, int64_t num_edges,
                              const int32_t* weight_rows, int64_t num_pairs, nqa_stream stream) {
  const PairedRows paired{weight_rows, num_pairs};
  int rc = check_paired("nqa_tp_scatter_fwd", weight_rows, num_pairs);
  if (rc != NQA_OK) return rc;
  return tp_fwd(plan, plan_image, dtype, {x, y, w, nullptr}, {rowptr_dst, edge_id_dst, src_sorted}, out, num_nodes,
                num_edges, &paired, static_cast<hipStream_t>(stream));
}

int nqa_tp_scatter_bwd_edge(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x,
                            const void* y, const void* w, const void* grad_out, const int32_t* rowptr_dst,
                            const int32_t* edge_id_dst, const int32_t* src_sorted, void* grad_w, void* grad_y,
                            void* workspace, int64_t workspace_bytes, int64_t num_nodes, int64_t num_edges,
                            nqa_stream stream) {
  return tp_bwd_edge(plan, plan_image, dtype, {x, y, w, grad_out}, {rowptr_dst, edge_id_dst, src_sorted}, grad_w, grad_y,
                     workspace, workspace_bytes, num_nodes, num_edges, nullptr, static_cast<hipStream_t>(stream));
}

int nqa_tp_scatter_bwd_edge_paired(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x,
                                   const void* y, const void* w, const void* grad_out, const int32_t* rowptr_dst,
                                   const int32_t* edge_id_dst, const int32_t* src_sorted, void* grad_w, void* grad_y,
                                   void* workspace, int64_t workspace_bytes, int64_t num_nodes, int64_t num_edges,
                                   const int32_t* weight_rows, int64_t num_pairs, nqa_stream stream) {
  const PairedRows paired{weight_rows, num_pairs};
  int rc = check_paired("nqa_tp_scatter_bwd_edge", weight_rows, num_pairs);
  if (rc != NQA_OK) return rc;
  return tp_bwd_edge(plan, plan_image, dtype, {x, y, w, grad_out}, {rowptr_dst, edge_id_dst, src_sorted}, grad_w, grad_y,
                     workspace, workspace_bytes, num_nodes, num_edges, &paired, static_cast<hipStream_t>(stream));
}

int nqa_tp_scatter_bwd_fused(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x,
                             const void* y, const void* w, const void* grad_out, const int32_t* rowptr_dst,
                             const int32_t* edge_id_dst, const int32_t* src_sorted, const int32_t* rowptr_src,
                             const int32_t* edge_id_src, void* grad_w, void* grad_y, void* grad_x, void* workspace,
                             int64_t workspace_bytes, int64_t num_nodes, int64_t num_edges, nqa_stream stream) {
  return tp_bwd_fused(plan, plan_image, dtype, {x, y, w, grad_out}, {rowptr_dst, edge_id_dst, src_sorted},
                      {rowptr_src, edge_id_src, nullptr}, grad_w, grad_y, grad_x, workspace, workspace_bytes, num_nodes,
                      num_edges, nullptr, static_cast<hipStream_t>(stream));
}

int nqa_tp_scatter_bwd_fused_paired(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x,
                                    const void* y, const void* w, const void* grad_out, const int32_t* rowptr_dst,
                                    const int32_t* edge_id_dst, const int32_t* src_sorted, const int32_t* rowptr_src,
                                    const int32_t* edge_id_src, void* grad_w, void* grad_y, void* grad_x, void* workspace,
                                    int64_t workspace_bytes, int64_t num_nodes, int64_t num_edges,
                                    const int32_t* weight_rows, int64_t num_pairs, nqa_stream stream) {
  const PairedRows paired{weight_rows, num_pairs};
  int rc = check_paired("nqa_tp_scatter_bwd_fused", weight_rows, num_pairs);
  if (rc != NQA_OK) return rc;
  return tp_bwd_fused(plan, plan_image, dtype, {x, y, w, grad_out}, {rowptr_dst, edge_id_dst, src_sorted},
                      {rowptr_src, edge_id_src, nullptr}, grad_w, grad_y, grad_x, workspace, workspace_bytes, num_nodes,
                      num_edges, &paired, static_cast<hipStream_t>(stream));
}

int nqa_tp_scatter_bwd_x(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* y, const void* w,
                         const void* grad_out, const int32_t* rowptr_src, const int32_t* edge_id_src,
                         const int32_t* dst_sorted, void* grad_x, int64_t num_nodes, int64_t num_edges,
                         nqa_stream stream) {
  return tp_bwd_x(plan, plan_image, dtype, {nullptr, y, w, grad_out}, {rowptr_src, edge_id_src, dst_sorted}, grad_x,
                  num_nodes, num_edges, nullptr, static_cast<hipStream_t>(stream));
}

int nqa_tp_scatter_bwd_x_paired(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* y, const void* w,
                                const void* grad_out, const int32_t* rowptr_src, const int32_t* edge_id_src,
                                const int32_t* dst_sorted, void* grad_x, int64_t num_nodes, int64_t num_edges,
                                const int32_t* weight_rows, int64_t num_pairs, nqa_stream stream) {
  const PairedRows paired{weight_rows, num_pairs};
  int rc = check_paired("nqa_tp_scatter_bwd_x", weight_rows, num_pairs);
  if (rc != NQA_OK) return rc;
  return tp_bwd_x(plan, plan_image, dtype, {nullptr, y, w, grad_out}, {rowptr_src, edge_id_src, dst_sorted}, grad_x,
                  num_nodes, num_edges, &paired, static_cast<hipStream_t>(stream));
}

int nqa_tp_scatter_bwd_pairs(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x, const void* y,
                             const void* w, const void* grad_out, const int32_t* owner_rowptr,
                             const int32_t* pair_other, const int32_t* pair_row, const int32_t* pair_edge_in,
                             const int32_t* pair_edge_out, const int32_t* other_rowptr, const int32_t* other_slot,
                             void* grad_w, void* grad_y, void* grad_x, void* workspace, int64_t workspace_bytes,
                             int64_t num_nodes, int64_t num_edges, nqa_stream stream) {
  const char* fn = "nqa_tp_scatter_bwd_pairs";
  int rc = check_common(plan, plan_image, dtype, fn);
  if (rc != NQA_OK) return rc;
  const TpWsLayout l = tp_ws_layout(plan, dtype, TpWs::Pairs, num_edges);
  if (l.total < 0)
    return fail(NQA_ERR_UNSUPPORTED, fn, ": no pair-centric float32 kernel for this plan (or an odd edge count)");
  if ((num_nodes > 0 && (!owner_rowptr || (grad_x && !other_rowptr))) ||
      (num_edges > 0 && (!x || !y || !w || !grad_out || !pair_other || !pair_row || !pair_edge_in || !pair_edge_out ||
                         (grad_x && !other_slot) || !grad_w || !grad_y)))
    return fail(NQA_ERR_INVALID, fn, kNullOperand);
  if (num_edges > 0 && (workspace == nullptr || workspace_bytes < l.total)) return fail(NQA_ERR_WORKSPACE, fn, kWorkspace);
  if (num_nodes == 0) return NQA_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const PairForm form = pair_form(plan, l, num_nodes, num_edges, grad_x != nullptr);
  float* gxe = tp_ws_view(workspace, l).gxe;  // the pair rows, or the accumulator [N, dim_in1] in their place
  SpecArgs<float> a = spec_owner_operands(plan, num_nodes, {x, y, w, grad_out},
                                          {owner_rowptr, pair_other, pair_row, pair_edge_in, pair_edge_out});
  a.gw = static_cast<float*>(grad_w);
  a.gxe = grad_x ? gxe : nullptr;
  a.out = static_cast<float*>(grad_x);  // NULL: grad_w and grad_y only
  a.gx_atomic = form.gx_atomic;
  if (form.gx_atomic && hipMemsetAsync(gxe, 0, (size_t)num_nodes * plan->dim_in1 * 4, s) != hipSuccess)
    return fail(NQA_ERR_LAUNCH, fn, ": hipMemsetAsync of the grad_x accumulator failed");
  // with more than one (channel chunk, part) per edge the ring kernels add their grad_y sums straight into the zeroed grad_y
  // (sums in arrival order, as the grad_x accumulator) -- no [E, S x chunks] partial rows, no reduce pass
  const GyMode mode = l.nchunk == 1 ? GyMode::Direct : (form.gy_atomic ? GyMode::Atomic : GyMode::Partial);
  if (mode == GyMode::Atomic && hipMemsetAsync(grad_y, 0, (size_t)num_edges * plan->dim_in2 * 4, s) != hipSuccess)
    return fail(NQA_ERR_LAUNCH, fn, ": hipMemsetAsync of grad_y failed");
  route_gy(a, l, grad_y, workspace, mode);
  if (spec_launch(plan, SpecKernel::BwdPairs, a, s, form.ring) != 0) return fail(NQA_ERR_UNSUPPORTED, fn, ": kernel not available");
  rc = check_launch("nqa_tp_scatter_bwd_pairs(pairs)");
  if (rc != NQA_OK) return rc;
  rc = finish_gy(plan, l, grad_y, workspace, mode, num_edges, "nqa_tp_scatter_bwd_pairs(reduce)", s);
  if (rc != NQA_OK) return rc;
  if (grad_x == nullptr) return NQA_OK;
  SpecArgs<float> b = spec_node_operands(plan, num_nodes);
  b.gxe = gxe;
  b.out = static_cast<float*>(grad_x);
  if (form.gx_atomic) {
    if (spec_launch(plan, SpecKernel::AccFinish, b, s) != 0)
      return fail(NQA_ERR_UNSUPPORTED, fn, ": this structure has no accumulator kernel");
    return check_launch("nqa_tp_scatter_bwd_pairs(accumulator)");
  }
  b.rowptr = other_rowptr;
  b.eid = other_slot;
  if (spec_launch(plan, SpecKernel::RowsSumPairs, b, s) != 0)
    return fail(NQA_ERR_UNSUPPORTED, fn, ": this structure has no grad_x row-sum kernel");
  return check_launch("nqa_tp_scatter_bwd_pairs(sum)");
}

int32_t nqa_tp_bwd_pairs_dual_supported(const nqa_plan* plan, int32_t dtype) {
  return (plan != nullptr && use_spec(plan, dtype) && plan->spec->pair == 1) ? 1 : 0;
}

int nqa_tp_scatter_bwd_pairs_dual(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x,
                                  const void* x_cot, const void* y, const void* y_cot, const void* w, const void* w_cot,
                                  const void* grad_out, const int32_t* owner_rowptr, const int32_t* pair_other,
                                  const int32_t* pair_row, const int32_t* pair_edge_in, const int32_t* pair_edge_out,
                                  void* grad_w, void* grad_y, void* workspace, int64_t workspace_bytes,
                                  int64_t num_nodes, int64_t num_edges, nqa_stream stream) {
  const char* fn = "nqa_tp_scatter_bwd_pairs_dual";
  int rc = check_common(plan, plan_image, dtype, fn);
  if (rc != NQA_OK) return rc;
  if (!nqa_tp_bwd_pairs_dual_supported(plan, dtype) || (num_edges & 1))
    return fail(NQA_ERR_UNSUPPORTED, fn, ": no dual pair-centric kernel for this plan (or an odd edge count)");
  const TpWsLayout l = tp_ws_layout(plan, dtype, TpWs::Pairs, num_edges);  // (pair == 1: nchunk is the channel chunks)
  if ((num_nodes > 0 && !owner_rowptr) ||
      (num_edges > 0 && (!x || !x_cot || !y || !y_cot || !w || !grad_out || !pair_other || !pair_row || !pair_edge_in ||
                         !pair_edge_out || !grad_w || !grad_y)))
    return fail(NQA_ERR_INVALID, fn, kNullOperand);
  if (num_edges > 0 && (workspace == nullptr || workspace_bytes < l.total)) return fail(NQA_ERR_WORKSPACE, fn, kWorkspace);
  if (num_nodes == 0 || num_edges == 0) return NQA_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  SpecArgs<float> a = spec_owner_operands(plan, num_nodes, {x, y, w, grad_out},
                                          {owner_rowptr, pair_other, pair_row, pair_edge_in, pair_edge_out});
  a.x2 = static_cast<const float*>(x_cot);
  a.y2 = static_cast<const float*>(y_cot);
  a.w2 = static_cast<const float*>(w_cot);  // optional: grad_y += By(x, w_cot, grad_out)
  a.gw = static_cast<float*>(grad_w);
  const GyMode mode = l.nchunk == 1 ? GyMode::Direct : GyMode::Partial;
  route_gy(a, l, grad_y, workspace, mode);
  if (spec_launch(plan, SpecKernel::BwdPairsDual, a, s) != 0) return fail(NQA_ERR_UNSUPPORTED, fn, ": kernel not available");
  rc = check_launch("nqa_tp_scatter_bwd_pairs_dual");
  if (rc != NQA_OK) return rc;
  return finish_gy(plan, l, grad_y, workspace, mode, num_edges, "nqa_tp_scatter_bwd_pairs_dual(reduce)", s);
}

int32_t nqa_tp_fwd_jvp_supported(const nqa_plan* plan, int32_t dtype) {
  return (plan != nullptr && use_spec(plan, dtype)) ? 1 : 0;
}

// (fwd_jvp, bwd_x_dual: weight_rows is optional, and its range check is part of the NULL-operand check)
static bool bad_optional_rows(const int32_t* weight_rows, int64_t num_pairs) {
  return weight_rows != nullptr && (num_pairs <= 0 || num_pairs > 1073741823);
}

int nqa_tp_scatter_fwd_jvp(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x, const void* y,
                           const void* w, const void* x_cot, const void* y_cot, const void* w_cot,
                           const int32_t* rowptr_dst, const int32_t* edge_id_dst, const int32_t* src_sorted, void* out,
                           int64_t num_nodes, int64_t num_edges, const int32_t* weight_rows, int64_t num_pairs,
                           nqa_stream stream) {
  const char* fn = "nqa_tp_scatter_fwd_jvp";
  int rc = check_common(plan, plan_image, dtype, fn);
  if (rc != NQA_OK) return rc;
  if (!use_spec(plan, dtype)) return fail(NQA_ERR_UNSUPPORTED, fn, kNoSpec);
  if (num_nodes < 0 || num_edges < 0 || (num_nodes > 0 && (!out || !rowptr_dst)) ||
      (num_edges > 0 && (!x || !y || !w || !edge_id_dst || !src_sorted || (!x_cot && !y_cot && !w_cot))) ||
      bad_optional_rows(weight_rows, num_pairs))
    return fail(NQA_ERR_INVALID, fn, ": NULL operand (at least one cotangent is required)");
  if (num_nodes == 0) return NQA_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (num_edges == 0) {  // no terms: the edge operands (cotangents included) are empty and may be NULL
    if (hipMemsetAsync(out, 0, (size_t)num_nodes * plan->dim_out * 4, s) != hipSuccess)
      return fail(NQA_ERR_LAUNCH, fn, ": hipMemsetAsync failed");
    return NQA_OK;
  }
  const PairedRows paired{weight_rows, num_pairs};
  SpecArgs<float> a = spec_edge_operands(plan, num_nodes, {x, y, w, nullptr}, {rowptr_dst, edge_id_dst, src_sorted},
                                         weight_rows ? &paired : nullptr);
  a.x2 = static_cast<const float*>(x_cot);
  a.y2 = static_cast<const float*>(y_cot);
  a.w2 = static_cast<const float*>(w_cot);
  a.out = static_cast<float*>(out);
  if (spec_launch(plan, SpecKernel::FwdJvp, a, s) != 0)
    return fail(NQA_ERR_UNSUPPORTED, fn, ": this structure has no forward-JVP kernel");
  return check_launch("nqa_tp_scatter_fwd_jvp");
}

int nqa_tp_scatter_bwd_x_dual(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* y, const void* w,
                              const void* y_cot, const void* w_cot, const void* grad_out, const int32_t* rowptr_src,
                              const int32_t* edge_id_src, const int32_t* dst_sorted, void* grad_x, int64_t num_nodes,
                              int64_t num_edges, const int32_t* weight_rows, int64_t num_pairs, nqa_stream stream) {
  const char* fn = "nqa_tp_scatter_bwd_x_dual";
  int rc = check_common(plan, plan_image, dtype, fn);
  if (rc != NQA_OK) return rc;
  if (!use_spec(plan, dtype)) return fail(NQA_ERR_UNSUPPORTED, fn, kNoSpec);
  if ((num_nodes > 0 && (!grad_x || !rowptr_src)) ||
      (num_edges > 0 && (!y || !w || !y_cot || !w_cot || !grad_out || !edge_id_src || !dst_sorted)) ||
      bad_optional_rows(weight_rows, num_pairs))
    return fail(NQA_ERR_INVALID, fn, kNullOperand);
  if (num_nodes == 0) return NQA_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (num_edges == 0) {  // no terms: the edge operands (cotangents included) are empty and may be NULL
    if (hipMemsetAsync(grad_x, 0, (size_t)num_nodes * plan->dim_in1 * 4, s) != hipSuccess)
      return fail(NQA_ERR_LAUNCH, fn, ": hipMemsetAsync failed");
    return NQA_OK;
  }
  const PairedRows paired{weight_rows, num_pairs};
  SpecArgs<float> a = spec_edge_operands(plan, num_nodes, {nullptr, y, w, grad_out}, {rowptr_src, edge_id_src, dst_sorted},
                                         weight_rows ? &paired : nullptr);
  a.y2 = static_cast<const float*>(y_cot);
  a.w2 = static_cast<const float*>(w_cot);
  a.out = static_cast<float*>(grad_x);
  if (spec_launch(plan, SpecKernel::BwdXDual, a, s) != 0) return fail(NQA_ERR_UNSUPPORTED, fn, ": kernel not available");
  return check_launch("nqa_tp_scatter_bwd_x_dual");
}

}  // extern "C"
