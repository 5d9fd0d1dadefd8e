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

#include <cstdint>

#include "generated/cg_generated.h"
#include "plan.h"
#include "tp_spec.h"

#include <cstdlib>

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
template <typename T>
static void fill_tables(TPArgs<T>& a, const nqa_plan* P, const void* image) {
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
}

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

template <typename T>
static int launch_fwd(const nqa_plan* P, const void* image, const void* x, const void* y, const void* w,
                      const int32_t* rowptr, const int32_t* eid, const int32_t* nbr, void* out, int64_t N, int64_t E,
                      hipStream_t stream) {
  (void)E;
  TPArgs<T> a{};
  fill_tables(a, P, image);
  a.x = static_cast<const T*>(x);
  a.y = static_cast<const T*>(y);
  a.w = static_cast<const T*>(w);
  a.out = static_cast<T*>(out);
  a.rowptr = rowptr;
  a.eid = eid;
  a.nbr = nbr;
  a.n_items = N * (int64_t)a.n_chunks;
  if (a.n_items == 0) return NQA_OK;
  unsigned grid;
  int rc = grid_for(a.n_items, &grid);
  if (rc != NQA_OK) return rc;
  hipLaunchKernelGGL(tp_fwd_kernel<T>, dim3(grid), dim3(kBlock), 0, stream, a);
  return check_launch("nqa_tp_scatter_fwd");
}

template <typename T>
static int launch_bwd_edge(const nqa_plan* P, const void* image, const void* x, const void* y, const void* w,
                           const void* g, const int32_t* rowptr, const int32_t* eid, const int32_t* nbr, void* gw,
                           void* gy, void* workspace, int64_t N, int64_t E, hipStream_t stream) {
  TPArgs<T> a{};
  fill_tables(a, P, image);
  a.x = static_cast<const T*>(x);
  a.y = static_cast<const T*>(y);
  a.w = static_cast<const T*>(w);
  a.g = static_cast<const T*>(g);
  a.gw = static_cast<T*>(gw);
  a.ypart = gy ? static_cast<T*>(workspace) : nullptr;
  a.rowptr = rowptr;
  a.eid = eid;
  a.nbr = nbr;
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
static int launch_bwd_x(const nqa_plan* P, const void* image, const void* y, const void* w, const void* g,
                        const int32_t* rowptr, const int32_t* eid, const int32_t* nbr, void* gx, int64_t N,
                        int64_t E, hipStream_t stream) {
  (void)E;
  TPArgs<T> a{};
  fill_tables(a, P, image);
  a.y = static_cast<const T*>(y);
  a.w = static_cast<const T*>(w);
  a.g = static_cast<const T*>(g);
  a.out = static_cast<T*>(gx);
  a.rowptr = rowptr;
  a.eid = eid;
  a.nbr = nbr;
  a.n_items = N * (int64_t)a.n_xchunks;
  if (a.n_items == 0) return NQA_OK;
  unsigned grid;
  int rc = grid_for(a.n_items, &grid);
  if (rc != NQA_OK) return rc;
  hipLaunchKernelGGL(tp_bwd_x_kernel<T>, dim3(grid), dim3(kBlock), 0, stream, a);
  return check_launch("nqa_tp_scatter_bwd_x");
}

// ---- structure-specialised ("edge-outer") kernels: used for float32 when prebuilt for the plan's structure ----
static bool force_generic() {
  static const bool v = [] {
    const char* e = std::getenv("NQA_FORCE_GENERIC");
    return e != nullptr && e[0] != '\0' && e[0] != '0';
  }();
  return v;
}

static bool use_spec(const nqa_plan* P, int32_t dtype) {
  return P->spec != nullptr && dtype == NQA_F32 && !force_generic();
}

static int spec_wpn(const nqa_plan* P, int64_t N) {
  // few (node, chunk) items -> split each node's edges over 4 wavefronts to fill the 256 CUs
  const int64_t items = N * (int64_t)((P->uniform_mul + 63) / 64);
  // experiment / test switch: 1 or 4 wavefronts per (node, chunk); measured: 4 wins at cfg-3 (2 was tried: slower).  Read at
  // every call (a getenv is ~100 ns) so that a test can force the large-box launch shape on a box the oracle can evaluate.
  const char* v = std::getenv("NQA_SPEC_WPN");
  const int forced = v ? std::atoi(v) : 0;
  if (forced == 1 || forced == 4) return forced;
  return items < 49152 ? 4 : 1;
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

static void spec_fill(SpecArgs<float>& a, const nqa_plan* P, int64_t N) {
  a.N = (int32_t)N;
  a.mul = P->uniform_mul;
  a.din = P->dim_in1;
  a.dout = P->dim_out;
  a.wn = P->weight_numel;
  a.gy_stride = P->dim_in2;
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

}  // namespace nqa

using namespace nqa;

extern "C" {

static int nqa_tp_scatter_fwd_impl(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x, const void* y,
                       const void* w, const int32_t* rowptr_dst, const int32_t* edge_id_dst,
                       const int32_t* src_sorted, void* out, int64_t num_nodes, int64_t num_edges,
                       nqa_stream stream, const int32_t* weight_rows, int64_t num_pairs) {
  int rc = check_common(plan, plan_image, dtype, "nqa_tp_scatter_fwd");
  if (rc != NQA_OK) return rc;
  if (num_nodes < 0 || num_edges < 0 || (num_nodes > 0 && (!out || !rowptr_dst)) ||
      (num_edges > 0 && (!x || !y || !w || !edge_id_dst || !src_sorted))) {
    set_error("nqa_tp_scatter_fwd: NULL operand");
    return NQA_ERR_INVALID;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (use_spec(plan, dtype)) {
    if (num_nodes == 0) return NQA_OK;
    SpecArgs<float> a{};
    spec_fill(a, plan, num_nodes);
    a.x = static_cast<const float*>(x);
    a.y = static_cast<const float*>(y);
    a.w = static_cast<const float*>(w);
    a.out = static_cast<float*>(out);
    a.rowptr = rowptr_dst;
    a.eid = edge_id_dst;
    a.nbr = src_sorted;
    a.wid = weight_rows ? weight_rows : edge_id_dst;
    a.wP = weight_rows ? (int32_t)num_pairs : 2147483647;
    plan->spec->launch(0, spec_wpn(plan, num_nodes), a, s);
    return check_launch("nqa_tp_scatter_fwd(spec)");
  }
  if (weight_rows != nullptr) {
    set_error("nqa_tp_scatter_fwd_paired: no structure-specialised float32 kernel for this plan");
    return NQA_ERR_UNSUPPORTED;
  }
  return dtype == NQA_F32
             ? launch_fwd<float>(plan, plan_image, x, y, w, rowptr_dst, edge_id_dst, src_sorted, out, num_nodes,
                                 num_edges, s)
             : launch_fwd<double>(plan, plan_image, x, y, w, rowptr_dst, edge_id_dst, src_sorted, out, num_nodes,
                                  num_edges, s);
}

int64_t nqa_tp_bwd_edge_workspace_bytes(const nqa_plan* plan, int32_t dtype, int64_t num_edges) {
  if (plan == nullptr || num_edges < 0) return -1;
  const int64_t es = dtype == NQA_F64 ? 8 : 4;
  // generic kernels: one partial per (instruction, 64-channel chunk) and component of its in2 irrep (ypart_width);
  // structure-specialised kernels: dim_in2 partials per channel chunk.  The larger of the two: for a structure with few
  // paths the second exceeds the first (one 0e x 0e path, l_max = 1 harmonics, 128 channels: 8 floats per edge against
  // 2) -- found when the truncated-input structures of the channel segments were added; no round-2 structure hit it.
  int64_t per_edge = plan->ypart_width;
  if (use_spec(plan, dtype)) {
    const int64_t spec_w = (int64_t)plan->dim_in2 * ((plan->uniform_mul + 63) / 64);
    if (spec_w > per_edge) per_edge = spec_w;
  }
  return num_edges * per_edge * es;
}

static int nqa_tp_scatter_bwd_edge_impl(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x,
                            const void* y, const void* w, const void* grad_out, const int32_t* rowptr_dst,
                            const int32_t* edge_id_dst, const int32_t* src_sorted, void* grad_w, void* grad_y,
                            void* workspace, int64_t workspace_bytes, int64_t num_nodes, int64_t num_edges,
                            nqa_stream stream, const int32_t* weight_rows, int64_t num_pairs) {
  int rc = check_common(plan, plan_image, dtype, "nqa_tp_scatter_bwd_edge");
  if (rc != NQA_OK) return rc;
  if (grad_w == nullptr && grad_y == nullptr) return NQA_OK;
  if (num_edges > 0 && (!x || !y || !w || !grad_out || !rowptr_dst || !edge_id_dst || !src_sorted)) {
    set_error("nqa_tp_scatter_bwd_edge: NULL operand");
    return NQA_ERR_INVALID;
  }
  if (grad_y != nullptr && num_edges > 0 &&
      (workspace == nullptr || workspace_bytes < nqa_tp_bwd_edge_workspace_bytes(plan, dtype, num_edges))) {
    set_error("nqa_tp_scatter_bwd_edge: workspace missing or too small");
    return NQA_ERR_WORKSPACE;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (use_spec(plan, dtype)) {
    if (num_nodes == 0 || num_edges == 0) return NQA_OK;
    SpecArgs<float> a{};
    spec_fill(a, plan, num_nodes);
    const int nchunk = (plan->uniform_mul + 63) / 64;
    a.x = static_cast<const float*>(x);
    a.y = static_cast<const float*>(y);
    a.w = static_cast<const float*>(w);
    a.g = static_cast<const float*>(grad_out);
    a.gw = static_cast<float*>(grad_w);
    a.rowptr = rowptr_dst;
    a.eid = edge_id_dst;
    a.nbr = src_sorted;
    a.wid = weight_rows ? weight_rows : edge_id_dst;
    a.wP = weight_rows ? (int32_t)num_pairs : 2147483647;
    if (grad_y != nullptr) {
      if (nchunk == 1) {
        a.gy = static_cast<float*>(grad_y);
        a.gy_stride = plan->dim_in2;
      } else {
        a.gy = static_cast<float*>(workspace);
        a.gy_stride = plan->dim_in2 * nchunk;
      }
    }
    plan->spec->launch(1, spec_wpn(plan, num_nodes), a, s);
    rc = check_launch("nqa_tp_scatter_bwd_edge(spec)");
    if (rc != NQA_OK) return rc;
    if (grad_y != nullptr && nchunk > 1) {
      const int64_t total = num_edges * (int64_t)plan->dim_in2;
      hipLaunchKernelGGL(spec_gy_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                         static_cast<const float*>(workspace), static_cast<float*>(grad_y), plan->dim_in2, nchunk,
                         total);
      return check_launch("nqa_tp_scatter_bwd_edge(spec reduce)");
    }
    return NQA_OK;
  }
  if (weight_rows != nullptr) {
    set_error("nqa_tp_scatter_bwd_edge_paired: no structure-specialised float32 kernel for this plan");
    return NQA_ERR_UNSUPPORTED;
  }
  return dtype == NQA_F32 ? launch_bwd_edge<float>(plan, plan_image, x, y, w, grad_out, rowptr_dst, edge_id_dst,
                                                   src_sorted, grad_w, grad_y, workspace, num_nodes, num_edges, s)
                          : launch_bwd_edge<double>(plan, plan_image, x, y, w, grad_out, rowptr_dst, edge_id_dst,
                                                    src_sorted, grad_w, grad_y, workspace, num_nodes, num_edges, s);
}

int64_t nqa_tp_bwd_fused_workspace_bytes(const nqa_plan* plan, int32_t dtype, int64_t num_edges) {
  if (plan == nullptr || num_edges < 0 || !use_spec(plan, dtype)) return -1;
  const int nchunk = (plan->uniform_mul + 63) / 64;
  const int64_t ypart = nchunk > 1 ? num_edges * (int64_t)plan->dim_in2 * nchunk * 4 : 0;
  return ((ypart + 255) & ~(int64_t)255) + num_edges * (int64_t)plan->dim_in1 * 4;
}

static int nqa_tp_scatter_bwd_fused_impl(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x,
                             const void* y, const void* w, const void* grad_out, const int32_t* rowptr_dst,
                             const int32_t* edge_id_dst, const int32_t* src_sorted, const int32_t* rowptr_src,
                             const int32_t* edge_id_src, void* grad_w, void* grad_y, void* grad_x, void* workspace,
                             int64_t workspace_bytes, int64_t num_nodes, int64_t num_edges, nqa_stream stream, const int32_t* weight_rows, int64_t num_pairs) {
  int rc = check_common(plan, plan_image, dtype, "nqa_tp_scatter_bwd_fused");
  if (rc != NQA_OK) return rc;
  if (!use_spec(plan, dtype)) {
    set_error("nqa_tp_scatter_bwd_fused: no structure-specialised float32 kernel for this plan");
    return NQA_ERR_UNSUPPORTED;
  }
  if ((num_nodes > 0 && (!grad_x || !rowptr_dst || !rowptr_src)) ||
      (num_edges > 0 &&
       (!x || !y || !w || !grad_out || !edge_id_dst || !src_sorted || !edge_id_src || !grad_w || !grad_y))) {
    set_error("nqa_tp_scatter_bwd_fused: NULL operand");
    return NQA_ERR_INVALID;
  }
  if (num_edges > 0 &&
      (workspace == nullptr || workspace_bytes < nqa_tp_bwd_fused_workspace_bytes(plan, dtype, num_edges))) {
    set_error("nqa_tp_scatter_bwd_fused: workspace missing or too small");
    return NQA_ERR_WORKSPACE;
  }
  if (num_nodes == 0) return NQA_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  SpecArgs<float> a{};
  spec_fill(a, plan, num_nodes);
  const int nchunk = (plan->uniform_mul + 63) / 64;
  const int64_t ypart = nchunk > 1 ? num_edges * (int64_t)plan->dim_in2 * nchunk * 4 : 0;
  float* gxe = reinterpret_cast<float*>(static_cast<char*>(workspace) + ((ypart + 255) & ~(int64_t)255));
  if (num_edges > 0) {
    a.x = static_cast<const float*>(x);
    a.y = static_cast<const float*>(y);
    a.w = static_cast<const float*>(w);
    a.g = static_cast<const float*>(grad_out);
    a.gw = static_cast<float*>(grad_w);
    a.gxe = gxe;
    a.rowptr = rowptr_dst;
    a.eid = edge_id_dst;
    a.nbr = src_sorted;
    a.wid = weight_rows ? weight_rows : edge_id_dst;
    a.wP = weight_rows ? (int32_t)num_pairs : 2147483647;
    if (grad_y != nullptr) {
      if (nchunk == 1) {
        a.gy = static_cast<float*>(grad_y);
        a.gy_stride = plan->dim_in2;
      } else {
        a.gy = static_cast<float*>(workspace);
        a.gy_stride = plan->dim_in2 * nchunk;
      }
    }
    plan->spec->launch(1, spec_wpn(plan, num_nodes), a, s);
    rc = check_launch("nqa_tp_scatter_bwd_fused(edge)");
    if (rc != NQA_OK) return rc;
    if (grad_y != nullptr && nchunk > 1) {
      const int64_t total = num_edges * (int64_t)plan->dim_in2;
      hipLaunchKernelGGL(spec_gy_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                         static_cast<const float*>(workspace), static_cast<float*>(grad_y), plan->dim_in2, nchunk,
                         total);
      rc = check_launch("nqa_tp_scatter_bwd_fused(reduce)");
      if (rc != NQA_OK) return rc;
    }
  }
  SpecArgs<float> b{};
  spec_fill(b, plan, num_nodes);
  b.gxe = gxe;
  b.out = static_cast<float*>(grad_x);
  b.rowptr = rowptr_src;
  b.eid = edge_id_src;
  plan->spec->launch(3, 1, b, s);
  return check_launch("nqa_tp_scatter_bwd_fused(sum)");
}

static int nqa_tp_scatter_bwd_x_impl(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* y, const void* w,
                         const void* grad_out, const int32_t* rowptr_src, const int32_t* edge_id_src,
                         const int32_t* dst_sorted, void* grad_x, int64_t num_nodes, int64_t num_edges,
                         nqa_stream stream, const int32_t* weight_rows, int64_t num_pairs) {
  int rc = check_common(plan, plan_image, dtype, "nqa_tp_scatter_bwd_x");
  if (rc != NQA_OK) return rc;
  if ((num_nodes > 0 && (!grad_x || !rowptr_src)) ||
      (num_edges > 0 && (!y || !w || !grad_out || !edge_id_src || !dst_sorted))) {
    set_error("nqa_tp_scatter_bwd_x: NULL operand");
    return NQA_ERR_INVALID;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (use_spec(plan, dtype)) {
    if (num_nodes == 0) return NQA_OK;
    SpecArgs<float> a{};
    spec_fill(a, plan, num_nodes);
    a.y = static_cast<const float*>(y);
    a.w = static_cast<const float*>(w);
    a.g = static_cast<const float*>(grad_out);
    a.out = static_cast<float*>(grad_x);
    a.rowptr = rowptr_src;
    a.eid = edge_id_src;
    a.nbr = dst_sorted;
    a.wid = weight_rows ? weight_rows : edge_id_src;
    a.wP = weight_rows ? (int32_t)num_pairs : 2147483647;
    plan->spec->launch(2, spec_wpn(plan, num_nodes), a, s);
    return check_launch("nqa_tp_scatter_bwd_x(spec)");
  }
  if (weight_rows != nullptr) {
    set_error("nqa_tp_scatter_bwd_x_paired: no structure-specialised float32 kernel for this plan");
    return NQA_ERR_UNSUPPORTED;
  }
  return dtype == NQA_F32 ? launch_bwd_x<float>(plan, plan_image, y, w, grad_out, rowptr_src, edge_id_src,
                                                dst_sorted, grad_x, num_nodes, num_edges, s)
                          : launch_bwd_x<double>(plan, plan_image, y, w, grad_out, rowptr_src, edge_id_src,
                                                 dst_sorted, grad_x, num_nodes, num_edges, s);
}

int nqa_tp_scatter_fwd(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x, const void* y,
                       const void* w, const int32_t* rowptr_dst, const int32_t* edge_id_dst,
                       const int32_t* src_sorted, void* out, int64_t num_nodes, int64_t num_edges,
                       nqa_stream stream) {
  return nqa_tp_scatter_fwd_impl(plan, plan_image, dtype, x, y, w, rowptr_dst, edge_id_dst, src_sorted, out, num_nodes, num_edges, stream, nullptr, 0);
}

int nqa_tp_scatter_fwd_paired(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x, const void* y,
                       const void* w, const int32_t* rowptr_dst, const int32_t* edge_id_dst,
                       const int32_t* src_sorted, void* out, int64_t num_nodes, int64_t num_edges,
                       const int32_t* weight_rows, int64_t num_pairs, nqa_stream stream) {
  if (weight_rows == nullptr || num_pairs <= 0 || num_pairs > 1073741823) {
    set_error("nqa_tp_scatter_fwd_paired: weight_rows / num_pairs missing or out of range");
    return NQA_ERR_INVALID;
  }
  return nqa_tp_scatter_fwd_impl(plan, plan_image, dtype, x, y, w, rowptr_dst, edge_id_dst, src_sorted, out, num_nodes, num_edges, stream, weight_rows, num_pairs);
}

int nqa_tp_scatter_bwd_edge(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x,
                            const void* y, const void* w, const void* grad_out, const int32_t* rowptr_dst,
                            const int32_t* edge_id_dst, const int32_t* src_sorted, void* grad_w, void* grad_y,
                            void* workspace, int64_t workspace_bytes, int64_t num_nodes, int64_t num_edges,
                            nqa_stream stream) {
  return nqa_tp_scatter_bwd_edge_impl(plan, plan_image, dtype, x, y, w, grad_out, rowptr_dst, edge_id_dst, src_sorted, grad_w, grad_y, workspace, workspace_bytes, num_nodes, num_edges, stream, nullptr, 0);
}

int nqa_tp_scatter_bwd_edge_paired(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x,
                            const void* y, const void* w, const void* grad_out, const int32_t* rowptr_dst,
                            const int32_t* edge_id_dst, const int32_t* src_sorted, void* grad_w, void* grad_y,
                            void* workspace, int64_t workspace_bytes, int64_t num_nodes, int64_t num_edges,
                            const int32_t* weight_rows, int64_t num_pairs, nqa_stream stream) {
  if (weight_rows == nullptr || num_pairs <= 0 || num_pairs > 1073741823) {
    set_error("nqa_tp_scatter_bwd_edge_paired: weight_rows / num_pairs missing or out of range");
    return NQA_ERR_INVALID;
  }
  return nqa_tp_scatter_bwd_edge_impl(plan, plan_image, dtype, x, y, w, grad_out, rowptr_dst, edge_id_dst, src_sorted, grad_w, grad_y, workspace, workspace_bytes, num_nodes, num_edges, stream, weight_rows, num_pairs);
}

int nqa_tp_scatter_bwd_fused(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x,
                             const void* y, const void* w, const void* grad_out, const int32_t* rowptr_dst,
                             const int32_t* edge_id_dst, const int32_t* src_sorted, const int32_t* rowptr_src,
                             const int32_t* edge_id_src, void* grad_w, void* grad_y, void* grad_x, void* workspace,
                             int64_t workspace_bytes, int64_t num_nodes, int64_t num_edges, nqa_stream stream) {
  return nqa_tp_scatter_bwd_fused_impl(plan, plan_image, dtype, x, y, w, grad_out, rowptr_dst, edge_id_dst, src_sorted, rowptr_src, edge_id_src, grad_w, grad_y, grad_x, workspace, workspace_bytes, num_nodes, num_edges, stream, nullptr, 0);
}

int nqa_tp_scatter_bwd_fused_paired(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x,
                             const void* y, const void* w, const void* grad_out, const int32_t* rowptr_dst,
                             const int32_t* edge_id_dst, const int32_t* src_sorted, const int32_t* rowptr_src,
                             const int32_t* edge_id_src, void* grad_w, void* grad_y, void* grad_x, void* workspace,
                             int64_t workspace_bytes, int64_t num_nodes, int64_t num_edges, const int32_t* weight_rows, int64_t num_pairs, nqa_stream stream) {
  if (weight_rows == nullptr || num_pairs <= 0 || num_pairs > 1073741823) {
    set_error("nqa_tp_scatter_bwd_fused_paired: weight_rows / num_pairs missing or out of range");
    return NQA_ERR_INVALID;
  }
  return nqa_tp_scatter_bwd_fused_impl(plan, plan_image, dtype, x, y, w, grad_out, rowptr_dst, edge_id_dst, src_sorted, rowptr_src, edge_id_src, grad_w, grad_y, grad_x, workspace, workspace_bytes, num_nodes, num_edges, stream, weight_rows, num_pairs);
}

int nqa_tp_scatter_bwd_x(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* y, const void* w,
                         const void* grad_out, const int32_t* rowptr_src, const int32_t* edge_id_src,
                         const int32_t* dst_sorted, void* grad_x, int64_t num_nodes, int64_t num_edges,
                         nqa_stream stream) {
  return nqa_tp_scatter_bwd_x_impl(plan, plan_image, dtype, y, w, grad_out, rowptr_src, edge_id_src, dst_sorted, grad_x, num_nodes, num_edges, stream, nullptr, 0);
}

int nqa_tp_scatter_bwd_x_paired(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* y, const void* w,
                         const void* grad_out, const int32_t* rowptr_src, const int32_t* edge_id_src,
                         const int32_t* dst_sorted, void* grad_x, int64_t num_nodes, int64_t num_edges,
                         const int32_t* weight_rows, int64_t num_pairs, nqa_stream stream) {
  if (weight_rows == nullptr || num_pairs <= 0 || num_pairs > 1073741823) {
    set_error("nqa_tp_scatter_bwd_x_paired: weight_rows / num_pairs missing or out of range");
    return NQA_ERR_INVALID;
  }
  return nqa_tp_scatter_bwd_x_impl(plan, plan_image, dtype, y, w, grad_out, rowptr_src, edge_id_src, dst_sorted, grad_x, num_nodes, num_edges, stream, weight_rows, num_pairs);
}

int64_t nqa_tp_bwd_pairs_workspace_bytes(const nqa_plan* plan, int32_t dtype, int64_t num_edges) {
  if (plan == nullptr || num_edges < 0 || (num_edges & 1) || !use_spec(plan, dtype) || !plan->spec->pair) return -1;
  const int nchunk = ((plan->uniform_mul + 63) / 64) * plan->spec->pair;  // grad_y partials per edge
  const int64_t ypart = nchunk > 1 ? num_edges * (int64_t)plan->dim_in2 * nchunk * 4 : 0;
  return ((ypart + 255) & ~(int64_t)255) + (num_edges / 2) * (int64_t)plan->dim_in1 * 4;
}

// The ring kernel's atomic grad_x form (round 6): one zeroed [N, dim_in1] accumulator instead of a row per pair.  On by
// default where the structure has the ring kernel; NQA_PAIR_GX_ATOMIC=0 keeps the rows (sums in a fixed order: results
// reproducible to the bit), NQA_PAIR_RING=0 the register kernel.
static bool pair_gx_atomic(const nqa_plan* plan, int64_t num_nodes, int64_t num_edges) {
  const char* ea = std::getenv("NQA_PAIR_GX_ATOMIC");  // (read at every call: the tests switch forms within one process)
  const char* er = std::getenv("NQA_PAIR_RING");
  // (the split kernel of the l_max = 3 structures has the accumulator form itself: spec->ring == 2)
  const bool on = (ea == nullptr || ea[0] != '0') && (plan->spec->ring == 2 || er == nullptr || er[0] != '0');
  // (the accumulator lives in the rows' workspace: [P, dim_in1] holds [N, dim_in1] whenever there are at least as many pairs
  // as nodes -- every list this is worth running on)
  return on && plan->spec->ring && (plan->uniform_mul & 63) == 0 && num_edges / 2 >= num_nodes;
}

int nqa_tp_scatter_bwd_pairs(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x, const void* y,
                             const void* w, const void* grad_out, const int32_t* owner_rowptr,
                             const int32_t* pair_other, const int32_t* pair_row, const int32_t* pair_edge_in,
                             const int32_t* pair_edge_out, const int32_t* other_rowptr, const int32_t* other_slot,
                             void* grad_w, void* grad_y, void* grad_x, void* workspace, int64_t workspace_bytes,
                             int64_t num_nodes, int64_t num_edges, nqa_stream stream) {
  int rc = check_common(plan, plan_image, dtype, "nqa_tp_scatter_bwd_pairs");
  if (rc != NQA_OK) return rc;
  const int64_t need = nqa_tp_bwd_pairs_workspace_bytes(plan, dtype, num_edges);
  if (need < 0) {
    set_error("nqa_tp_scatter_bwd_pairs: no pair-centric float32 kernel for this plan (or an odd edge count)");
    return NQA_ERR_UNSUPPORTED;
  }
  if ((num_nodes > 0 && (!owner_rowptr || (grad_x && !other_rowptr))) ||
      (num_edges > 0 && (!x || !y || !w || !grad_out || !pair_other || !pair_row || !pair_edge_in || !pair_edge_out ||
                         (grad_x && !other_slot) || !grad_w || !grad_y))) {
    set_error("nqa_tp_scatter_bwd_pairs: NULL operand");
    return NQA_ERR_INVALID;
  }
  if (num_edges > 0 && (workspace == nullptr || workspace_bytes < need)) {
    set_error("nqa_tp_scatter_bwd_pairs: workspace missing or too small");
    return NQA_ERR_WORKSPACE;
  }
  if (num_nodes == 0) return NQA_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  SpecArgs<float> a{};
  spec_fill(a, plan, num_nodes);
  const int nchunk = ((plan->uniform_mul + 63) / 64) * plan->spec->pair;  // grad_y partials per edge
  const int64_t ypart = nchunk > 1 ? num_edges * (int64_t)plan->dim_in2 * nchunk * 4 : 0;
  float* gxe = reinterpret_cast<float*>(static_cast<char*>(workspace) + ((ypart + 255) & ~(int64_t)255));
  a.x = static_cast<const float*>(x);
  a.y = static_cast<const float*>(y);
  a.w = static_cast<const float*>(w);
  a.g = static_cast<const float*>(grad_out);
  a.gw = static_cast<float*>(grad_w);
  a.gxe = grad_x ? gxe : nullptr;
  a.out = static_cast<float*>(grad_x);  // NULL: grad_w and grad_y only
  a.rowptr = owner_rowptr;
  a.nbr = pair_other;
  a.wid = pair_row;
  a.eid = pair_edge_in;
  a.eid2 = pair_edge_out;
  a.wP = 2147483647;
  const bool atomic = grad_x != nullptr && pair_gx_atomic(plan, num_nodes, num_edges);
  if (atomic) {
    a.gx_atomic = 1;
    if (hipMemsetAsync(gxe, 0, (size_t)num_nodes * plan->dim_in1 * 4, s) != hipSuccess) {
      set_error("nqa_tp_scatter_bwd_pairs: hipMemsetAsync of the grad_x accumulator failed");
      return NQA_ERR_LAUNCH;
    }
  }
  // round 6: with more than one (channel chunk, part) per edge the ring kernels add their grad_y sums straight into the
  // zeroed grad_y (same switch and same caveat as the grad_x accumulator: sums in arrival order) -- no [E, S x chunks] partial
  // rows, no reduce pass.  Only where a ring kernel is what runs: the unsplit one for either request, the split one with grad_x.
  const bool gy_atomic = nchunk > 1 && num_edges > 0 && pair_gx_atomic(plan, num_nodes, num_edges) &&
                         (plan->spec->ring == 1 || (plan->spec->ring == 2 && grad_x != nullptr)) && [] {
                           const char* er = std::getenv("NQA_PAIR_RING");
                           return er == nullptr || er[0] != '0';
                         }();
  if (nchunk == 1) {
    a.gy = static_cast<float*>(grad_y);
    a.gy_stride = plan->dim_in2;
  } else if (gy_atomic) {
    if (hipMemsetAsync(grad_y, 0, (size_t)num_edges * plan->dim_in2 * 4, s) != hipSuccess) {
      set_error("nqa_tp_scatter_bwd_pairs: hipMemsetAsync of grad_y failed");
      return NQA_ERR_LAUNCH;
    }
    a.gy = static_cast<float*>(grad_y);
    a.gy_stride = plan->dim_in2;
    a.gy_atomic = 1;
  } else {
    a.gy = static_cast<float*>(workspace);
    a.gy_stride = plan->dim_in2 * nchunk;
  }
  if (plan->spec->launch(4, spec_wpn(plan, num_nodes), a, s) != 0) {
    set_error("nqa_tp_scatter_bwd_pairs: kernel not available");
    return NQA_ERR_UNSUPPORTED;
  }
  rc = check_launch("nqa_tp_scatter_bwd_pairs(pairs)");
  if (rc != NQA_OK) return rc;
  if (nchunk > 1 && num_edges > 0 && !gy_atomic) {
    const int64_t total = num_edges * (int64_t)plan->dim_in2;
    hipLaunchKernelGGL(spec_gy_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                       static_cast<const float*>(workspace), static_cast<float*>(grad_y), plan->dim_in2, nchunk, total);
    rc = check_launch("nqa_tp_scatter_bwd_pairs(reduce)");
    if (rc != NQA_OK) return rc;
  }
  if (grad_x == nullptr) return NQA_OK;
  SpecArgs<float> b{};
  spec_fill(b, plan, num_nodes);
  b.gxe = gxe;
  b.out = static_cast<float*>(grad_x);
  if (atomic) {
    if (plan->spec->launch(9, 1, b, s) != 0) {
      set_error("nqa_tp_scatter_bwd_pairs: this structure has no accumulator kernel");
      return NQA_ERR_UNSUPPORTED;
    }
    return check_launch("nqa_tp_scatter_bwd_pairs(accumulator)");
  }
  b.rowptr = other_rowptr;
  b.eid = other_slot;
  if (plan->spec->launch(5, 1, b, s) != 0) {
    set_error("nqa_tp_scatter_bwd_pairs: this structure has no grad_x row-sum kernel");
    return NQA_ERR_UNSUPPORTED;
  }
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
  int rc = check_common(plan, plan_image, dtype, "nqa_tp_scatter_bwd_pairs_dual");
  if (rc != NQA_OK) return rc;
  if (!nqa_tp_bwd_pairs_dual_supported(plan, dtype) || (num_edges & 1)) {
    set_error("nqa_tp_scatter_bwd_pairs_dual: no dual pair-centric kernel for this plan (or an odd edge count)");
    return NQA_ERR_UNSUPPORTED;
  }
  const int64_t need = nqa_tp_bwd_pairs_workspace_bytes(plan, dtype, num_edges);
  if ((num_nodes > 0 && !owner_rowptr) ||
      (num_edges > 0 && (!x || !x_cot || !y || !y_cot || !w || !grad_out || !pair_other || !pair_row || !pair_edge_in ||
                         !pair_edge_out || !grad_w || !grad_y))) {
    set_error("nqa_tp_scatter_bwd_pairs_dual: NULL operand");
    return NQA_ERR_INVALID;
  }
  if (num_edges > 0 && (workspace == nullptr || workspace_bytes < need)) {
    set_error("nqa_tp_scatter_bwd_pairs_dual: workspace missing or too small");
    return NQA_ERR_WORKSPACE;
  }
  if (num_nodes == 0 || num_edges == 0) return NQA_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  SpecArgs<float> a{};
  spec_fill(a, plan, num_nodes);
  const int nchunk = (plan->uniform_mul + 63) / 64;
  a.x = static_cast<const float*>(x);
  a.x2 = static_cast<const float*>(x_cot);
  a.y = static_cast<const float*>(y);
  a.y2 = static_cast<const float*>(y_cot);
  a.w = static_cast<const float*>(w);
  a.w2 = static_cast<const float*>(w_cot);  // optional: grad_y += By(x, w_cot, grad_out)
  a.g = static_cast<const float*>(grad_out);
  a.gw = static_cast<float*>(grad_w);
  a.rowptr = owner_rowptr;
  a.nbr = pair_other;
  a.wid = pair_row;
  a.eid = pair_edge_in;
  a.eid2 = pair_edge_out;
  a.wP = 2147483647;
  if (nchunk == 1) {
    a.gy = static_cast<float*>(grad_y);
    a.gy_stride = plan->dim_in2;
  } else {
    a.gy = static_cast<float*>(workspace);
    a.gy_stride = plan->dim_in2 * nchunk;
  }
  if (plan->spec->launch(6, spec_wpn(plan, num_nodes), a, s) != 0) {
    set_error("nqa_tp_scatter_bwd_pairs_dual: kernel not available");
    return NQA_ERR_UNSUPPORTED;
  }
  rc = check_launch("nqa_tp_scatter_bwd_pairs_dual");
  if (rc != NQA_OK) return rc;
  if (nchunk > 1) {
    const int64_t total = num_edges * (int64_t)plan->dim_in2;
    hipLaunchKernelGGL(spec_gy_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                       static_cast<const float*>(workspace), static_cast<float*>(grad_y), plan->dim_in2, nchunk, total);
    rc = check_launch("nqa_tp_scatter_bwd_pairs_dual(reduce)");
  }
  return rc;
}

int32_t nqa_tp_fwd_jvp_supported(const nqa_plan* plan, int32_t dtype) {
  return (plan != nullptr && use_spec(plan, dtype)) ? 1 : 0;
}

int nqa_tp_scatter_fwd_jvp(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x, const void* y,
                           const void* w, const void* x_cot, const void* y_cot, const void* w_cot,
                           const int32_t* rowptr_dst, const int32_t* edge_id_dst, const int32_t* src_sorted, void* out,
                           int64_t num_nodes, int64_t num_edges, const int32_t* weight_rows, int64_t num_pairs,
                           nqa_stream stream) {
  int rc = check_common(plan, plan_image, dtype, "nqa_tp_scatter_fwd_jvp");
  if (rc != NQA_OK) return rc;
  if (!use_spec(plan, dtype)) {
    set_error("nqa_tp_scatter_fwd_jvp: no structure-specialised float32 kernel for this plan");
    return NQA_ERR_UNSUPPORTED;
  }
  if (num_nodes < 0 || num_edges < 0 || (num_nodes > 0 && (!out || !rowptr_dst)) ||
      (num_edges > 0 && (!x || !y || !w || !edge_id_dst || !src_sorted || (!x_cot && !y_cot && !w_cot))) ||
      (weight_rows != nullptr && (num_pairs <= 0 || num_pairs > 1073741823))) {
    set_error("nqa_tp_scatter_fwd_jvp: NULL operand (at least one cotangent is required)");
    return NQA_ERR_INVALID;
  }
  if (num_nodes == 0) return NQA_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (num_edges == 0) {  // no terms: the edge operands (cotangents included) are empty and may be NULL
    if (hipMemsetAsync(out, 0, (size_t)num_nodes * plan->dim_out * 4, s) != hipSuccess) {
      set_error("nqa_tp_scatter_fwd_jvp: hipMemsetAsync failed");
      return NQA_ERR_LAUNCH;
    }
    return NQA_OK;
  }
  SpecArgs<float> a{};
  spec_fill(a, plan, num_nodes);
  a.x = static_cast<const float*>(x);
  a.y = static_cast<const float*>(y);
  a.w = static_cast<const float*>(w);
  a.x2 = static_cast<const float*>(x_cot);
  a.y2 = static_cast<const float*>(y_cot);
  a.w2 = static_cast<const float*>(w_cot);
  a.out = static_cast<float*>(out);
  a.rowptr = rowptr_dst;
  a.eid = edge_id_dst;
  a.nbr = src_sorted;
  a.wid = weight_rows ? weight_rows : edge_id_dst;
  a.wP = weight_rows ? (int32_t)num_pairs : 2147483647;
  if (plan->spec->launch(7, spec_wpn(plan, num_nodes), a, s) != 0) {
    set_error("nqa_tp_scatter_fwd_jvp: this structure has no forward-JVP kernel");
    return NQA_ERR_UNSUPPORTED;
  }
  return check_launch("nqa_tp_scatter_fwd_jvp");
}

int nqa_tp_scatter_bwd_x_dual(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* y, const void* w,
                              const void* y_cot, const void* w_cot, const void* grad_out, const int32_t* rowptr_src,
                              const int32_t* edge_id_src, const int32_t* dst_sorted, void* grad_x, int64_t num_nodes,
                              int64_t num_edges, const int32_t* weight_rows, int64_t num_pairs, nqa_stream stream) {
  int rc = check_common(plan, plan_image, dtype, "nqa_tp_scatter_bwd_x_dual");
  if (rc != NQA_OK) return rc;
  if (!use_spec(plan, dtype)) {
    set_error("nqa_tp_scatter_bwd_x_dual: no structure-specialised float32 kernel for this plan");
    return NQA_ERR_UNSUPPORTED;
  }
  if ((num_nodes > 0 && (!grad_x || !rowptr_src)) ||
      (num_edges > 0 && (!y || !w || !y_cot || !w_cot || !grad_out || !edge_id_src || !dst_sorted)) ||
      (weight_rows != nullptr && (num_pairs <= 0 || num_pairs > 1073741823))) {
    set_error("nqa_tp_scatter_bwd_x_dual: NULL operand");
    return NQA_ERR_INVALID;
  }
  if (num_nodes == 0) return NQA_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (num_edges == 0) {  // no terms: the edge operands (cotangents included) are empty and may be NULL
    if (hipMemsetAsync(grad_x, 0, (size_t)num_nodes * plan->dim_in1 * 4, s) != hipSuccess) {
      set_error("nqa_tp_scatter_bwd_x_dual: hipMemsetAsync failed");
      return NQA_ERR_LAUNCH;
    }
    return NQA_OK;
  }
  SpecArgs<float> a{};
  spec_fill(a, plan, num_nodes);
  a.y = static_cast<const float*>(y);
  a.w = static_cast<const float*>(w);
  a.y2 = static_cast<const float*>(y_cot);
  a.w2 = static_cast<const float*>(w_cot);
  a.g = static_cast<const float*>(grad_out);
  a.out = static_cast<float*>(grad_x);
  a.rowptr = rowptr_src;
  a.eid = edge_id_src;
  a.nbr = dst_sorted;
  a.wid = weight_rows ? weight_rows : edge_id_src;
  a.wP = weight_rows ? (int32_t)num_pairs : 2147483647;
  if (plan->spec->launch(8, spec_wpn(plan, num_nodes), a, s) != 0) {
    set_error("nqa_tp_scatter_bwd_x_dual: kernel not available");
    return NQA_ERR_UNSUPPORTED;
  }
  return check_launch("nqa_tp_scatter_bwd_x_dual");
}

}  // extern "C"




