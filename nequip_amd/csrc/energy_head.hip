// Per-atom energy head in one launch per direction.
//
// After the last convolution the reference runs, on the N atom rows (nequip/model/nequip_models.py:371-399):
//   Gate (the last layer keeps scalars only: x = cst * act(h))                  nequip/nn/convnetlayer.py:162-164
//   ScalarMLP readout, depth 0: e = x @ (W * alpha), float32                    nequip/nn/mlp.py:262-268
//   PerTypeScaleShift: E_atom = shift[type] + scale[type] * double(e)           nequip/nn/atomwise.py:116-284
// and autograd runs the same chain backwards -- a dozen launches on [N, 64] / [N, 1] tensors that cost more in launch
// latency than in work.  Here: forward one launch (h -> E_atom, float64), backward one launch (dE_atom -> dh).
// Arithmetic as in the reference: the dot product in float32, scale / shift in float64.
//
// Training with trainable scale / shift tables (PerTypeScaleShift(scales_trainable / shifts_trainable), atomwise.py:190-234):
// the same forward launch, and a twice-differentiable backward that also returns the gradients of the readout weight and of
// the two tables (nqa_energy_head_train_bwd / _bwd_bwd below).  Those are sums over atoms: every workgroup leaves one row of
// partial sums, a second launch adds the rows in a fixed order -- no floating-point atomics, bit-reproducible results.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "plan.h"

namespace nqa {

template <typename T>
__device__ __forceinline__ T eh_act(int act, T x, T cst) {
  if (act == 1) return cst * x / (T(1) + expf(-x));
  if (act == 2) return cst * tanhf(x);
  return x;
}
template <typename T>
__device__ __forceinline__ T eh_act_grad(int act, T x, T cst) {
  if (act == 1) {
    const T s = T(1) / (T(1) + expf(-x));
    return cst * s * (T(1) + x * (T(1) - s));
  }
  if (act == 2) {
    const T t = tanhf(x);
    return cst * (T(1) - t * t);
  }
  return T(1);
}

// a''(x):  silu  cst s (1 - s) (2 + x (1 - 2 s)), s = sigmoid(x);  tanh  -2 cst t (1 - t^2);  identity  0
template <typename T>
__device__ __forceinline__ T eh_act_grad2(int act, T x, T cst) {
  if (act == 1) {
    const T s = T(1) / (T(1) + expf(-x));
    return cst * s * (T(1) - s) * (T(2) + x * (T(1) - T(2) * s));
  }
  if (act == 2) {
    const T t = tanhf(x);
    return T(-2) * cst * t * (T(1) - t * t);
  }
  return T(0);
}

struct EnergyHeadArgs {
  const float* __restrict__ h;        // [N, D] pre-activation scalars
  const float* __restrict__ w;        // [D] readout weights (alpha folded in)
  const double* __restrict__ scales;  // [n_scales] or NULL
  const double* __restrict__ shifts;  // [n_shifts] or NULL
  const int64_t* __restrict__ types;  // [N] (needed when n_scales > 1 or n_shifts > 1)
  const double* __restrict__ g_e;     // backward: [N] gradient w.r.t. the per-atom energies
  double* __restrict__ e_atom;        // forward: [N]
  float* __restrict__ g_h;            // backward: [N, D]
  int64_t N;
  int32_t D, act, n_scales, n_shifts;
  float cst;
};

// 16 lanes per atom, four atoms per wavefront; a lane walks the row in float4 steps of 16 lanes (D % 4 == 0)
__global__ __launch_bounds__(256) void energy_head_fwd_kernel(const EnergyHeadArgs a) {
  const int sub = threadIdx.x & 15;
  const int64_t z = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
  const bool ok = z < a.N;
  const float* __restrict__ row = a.h + (ok ? z : 0) * a.D;
  float s = 0.f;
  for (int c = 4 * sub; c < a.D; c += 64) {
    const float4 hv = *reinterpret_cast<const float4*>(row + c);
    const float4 wv = *reinterpret_cast<const float4*>(a.w + c);
    s += wv.x * eh_act(a.act, hv.x, a.cst) + wv.y * eh_act(a.act, hv.y, a.cst) + wv.z * eh_act(a.act, hv.z, a.cst) +
         wv.w * eh_act(a.act, hv.w, a.cst);
  }
  s += __shfl_xor(s, 8);
  s += __shfl_xor(s, 4);
  s += __shfl_xor(s, 2);
  s += __shfl_xor(s, 1);
  if (ok && sub == 0) {
    const int t = (a.n_scales > 1 || a.n_shifts > 1) ? (int)a.types[z] : 0;
    double e = (double)s;
    if (a.scales != nullptr) e *= a.scales[a.n_scales > 1 ? t : 0];
    if (a.shifts != nullptr) e += a.shifts[a.n_shifts > 1 ? t : 0];
    a.e_atom[z] = e;
  }
}

__global__ __launch_bounds__(256) void energy_head_bwd_kernel(const EnergyHeadArgs a) {
  const int q = a.D >> 2;  // float4 per row
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.N * q) return;
  const int64_t z = idx / q;
  const int c = (int)(idx - z * q) * 4;
  double g = a.g_e[z];
  if (a.scales != nullptr) g *= a.scales[a.n_scales > 1 ? (int)a.types[z] : 0];
  const float gf = (float)g;
  const float4 hv = *reinterpret_cast<const float4*>(a.h + z * a.D + c);
  const float4 wv = *reinterpret_cast<const float4*>(a.w + c);
  float4 r;
  r.x = gf * wv.x * eh_act_grad(a.act, hv.x, a.cst);
  r.y = gf * wv.y * eh_act_grad(a.act, hv.y, a.cst);
  r.z = gf * wv.z * eh_act_grad(a.act, hv.z, a.cst);
  r.w = gf * wv.w * eh_act_grad(a.act, hv.w, a.cst);
  *reinterpret_cast<float4*>(a.g_h + z * a.D + c) = r;
}

// ---- training head: first and second backward with the parameter gradients -------------------------------------------------
constexpr int EH_KMAX = 8;          // float4 steps of a lane along its row: dim <= 64 * EH_KMAX
constexpr int EH_TABLE_MAX = 128;   // entries of a scale / shift table whose gradient is accumulated in LDS
constexpr int EH_MAX_GROUPS = 256;  // workgroups (= rows of partial sums) of the first stage

struct EnergyHeadTrainArgs {
  const float* __restrict__ h;        // [N, D]
  const float* __restrict__ w;        // [D]
  const double* __restrict__ scales;  // [n_scales] or NULL
  const int64_t* __restrict__ types;  // [N]
  const double* __restrict__ g_e;     // [N]
  const float* __restrict__ v;        // second backward: [N, D] cotangent of g_h
  float* __restrict__ g_h;            // [N, D] or NULL (first: g_h, second: the gradient w.r.t. h)
  double* __restrict__ gg_e;          // second backward: [N] or NULL
  float* __restrict__ part_w;         // [groups, D] or NULL
  double* __restrict__ part_scale;    // [groups, n_scales] or NULL
  double* __restrict__ part_shift;    // [groups, n_shifts] or NULL (first backward only)
  int64_t N;
  int32_t D, act, n_scales, n_shifts;
  float cst;
};

// Row layout of the kernels above: 16 lanes per atom (a "slot"), 16 slots per workgroup, float4 steps of 64 columns.  A
// workgroup walks the atoms z = 16 (block + k gridDim) + slot.  Per lane: the weight-gradient terms of its own columns in
// registers.  Per slot: the per-type terms in a private float64 LDS row (one writing lane per row: plain read-modify-write).
// At the end the slots are added in a fixed order: 4 slots of a wavefront by shuffles, the 4 wavefronts and the 16 table rows
// through LDS; the workgroup stores ONE row of partial sums.
//   SECOND == false:  g_h = gf w a'(h),      row sum s = sum_c w a(h)        w: gf a(h)       scale: g_e double(s)   shift: g_e
//   SECOND == true:   g_h = gf w a''(h) v,   row sum u = sum_c v w a'(h)     w: gf a'(h) v    scale: g_e double(u)   gg_e = scale double(u)
//   with gf = float(g_e * scale[type])
template <bool SECOND>
__global__ __launch_bounds__(256) void energy_head_train_kernel(const EnergyHeadTrainArgs a) {
  extern __shared__ __attribute__((aligned(16))) char eh_smem[];
  const int ns = a.part_scale != nullptr ? a.n_scales : 0;
  const int nh = a.part_shift != nullptr ? a.n_shifts : 0;
  double* __restrict__ slot_scale = reinterpret_cast<double*>(eh_smem);  // [16, ns]
  double* __restrict__ slot_shift = slot_scale + 16 * ns;                // [16, nh]
  float* __restrict__ wave_w = reinterpret_cast<float*>(slot_shift + 16 * nh);  // [4, D] (byte offset: a multiple of 128)
  const int tid = threadIdx.x, sub = tid & 15, slot = tid >> 4;
  for (int i = tid; i < 16 * (ns + nh); i += 256) slot_scale[i] = 0.0;
  __syncthreads();

  float4 acc[EH_KMAX];
#pragma unroll
  for (int k = 0; k < EH_KMAX; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  const bool typed = a.n_scales > 1 || a.n_shifts > 1;
  for (int64_t z0 = (int64_t)blockIdx.x * 16; z0 < a.N; z0 += (int64_t)gridDim.x * 16) {  // (uniform trip count)
    const int64_t z = z0 + slot;
    const bool ok = z < a.N;
    const int64_t zr = ok ? z : 0;
    const int t = typed ? (int)a.types[zr] : 0;
    const int ts = a.n_scales > 1 ? min(max(t, 0), a.n_scales - 1) : 0;
    const double ge = ok ? a.g_e[zr] : 0.0;
    const double sc = a.scales != nullptr ? a.scales[ts] : 1.0;
    const float gf = (float)(ge * sc);
    const float* __restrict__ row = a.h + zr * a.D;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < EH_KMAX; ++k) {
      const int c = 4 * sub + 64 * k;
      if (c < a.D) {
        const float4 hv = *reinterpret_cast<const float4*>(row + c);
        const float4 wv = *reinterpret_cast<const float4*>(a.w + c);
        float4 r, p;  // r: the g_h entries, p: the weight-gradient terms
        if (SECOND) {
          const float4 vv = *reinterpret_cast<const float4*>(a.v + zr * a.D + c);
          const float dx = eh_act_grad(a.act, hv.x, a.cst), dy = eh_act_grad(a.act, hv.y, a.cst),
                      dz = eh_act_grad(a.act, hv.z, a.cst), dw = eh_act_grad(a.act, hv.w, a.cst);
          s += vv.x * wv.x * dx + vv.y * wv.y * dy + vv.z * wv.z * dz + vv.w * wv.w * dw;
          p = make_float4(gf * dx * vv.x, gf * dy * vv.y, gf * dz * vv.z, gf * dw * vv.w);
          r.x = gf * wv.x * eh_act_grad2(a.act, hv.x, a.cst) * vv.x;
          r.y = gf * wv.y * eh_act_grad2(a.act, hv.y, a.cst) * vv.y;
          r.z = gf * wv.z * eh_act_grad2(a.act, hv.z, a.cst) * vv.z;
          r.w = gf * wv.w * eh_act_grad2(a.act, hv.w, a.cst) * vv.w;
        } else {
          const float ax = eh_act(a.act, hv.x, a.cst), ay = eh_act(a.act, hv.y, a.cst), az = eh_act(a.act, hv.z, a.cst),
                      aw = eh_act(a.act, hv.w, a.cst);
          s += wv.x * ax + wv.y * ay + wv.z * az + wv.w * aw;  // (the forward kernel's expression: the same s)
          p = make_float4(gf * ax, gf * ay, gf * az, gf * aw);
          r.x = gf * wv.x * eh_act_grad(a.act, hv.x, a.cst);
          r.y = gf * wv.y * eh_act_grad(a.act, hv.y, a.cst);
          r.z = gf * wv.z * eh_act_grad(a.act, hv.z, a.cst);
          r.w = gf * wv.w * eh_act_grad(a.act, hv.w, a.cst);
        }
        if (ok) {
          if (a.g_h != nullptr) *reinterpret_cast<float4*>(a.g_h + z * a.D + c) = r;
          acc[k].x += p.x;
          acc[k].y += p.y;
          acc[k].z += p.z;
          acc[k].w += p.w;
        }
      }
    }
    s += __shfl_xor(s, 8);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    if (ok && sub == 0) {
      if (SECOND && a.gg_e != nullptr) a.gg_e[z] = sc * (double)s;
      if (ns > 0) slot_scale[slot * ns + ts] += ge * (double)s;
      if (nh > 0) slot_shift[slot * nh + (nh > 1 ? min(max(t, 0), nh - 1) : 0)] += ge;
    }
  }

  if (a.part_w != nullptr) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < EH_KMAX; ++k) {  // slots of this wavefront: lanes l, l + 16, l + 32, l + 48
      acc[k].x += __shfl_xor(acc[k].x, 16);
      acc[k].y += __shfl_xor(acc[k].y, 16);
      acc[k].z += __shfl_xor(acc[k].z, 16);
      acc[k].w += __shfl_xor(acc[k].w, 16);
      acc[k].x += __shfl_xor(acc[k].x, 32);
      acc[k].y += __shfl_xor(acc[k].y, 32);
      acc[k].z += __shfl_xor(acc[k].z, 32);
      acc[k].w += __shfl_xor(acc[k].w, 32);
      const int c = 4 * lane + 64 * k;
      if (lane < 16 && c < a.D) *reinterpret_cast<float4*>(wave_w + wave * a.D + c) = acc[k];
    }
  }
  __syncthreads();  // (also: the slot rows are complete)
  if (a.part_w != nullptr)
    for (int c = tid; c < a.D; c += 256)
      a.part_w[(int64_t)blockIdx.x * a.D + c] =
          ((wave_w[c] + wave_w[a.D + c]) + wave_w[2 * a.D + c]) + wave_w[3 * a.D + c];
  for (int i = tid; i < ns; i += 256) {
    double r = 0.0;
    for (int q = 0; q < 16; ++q) r += slot_scale[q * ns + i];
    a.part_scale[(int64_t)blockIdx.x * ns + i] = r;
  }
  for (int i = tid; i < nh; i += 256) {
    double r = 0.0;
    for (int q = 0; q < 16; ++q) r += slot_shift[q * nh + i];
    a.part_shift[(int64_t)blockIdx.x * nh + i] = r;
  }
}

// second stage: one thread per output entry adds the rows of partial sums in row order (groups <= EH_MAX_GROUPS; groups == 0,
// no atoms, writes zeros)
__global__ __launch_bounds__(256) void energy_head_train_sum_kernel(const float* __restrict__ part_w,
                                                                    const double* __restrict__ part_scale,
                                                                    const double* __restrict__ part_shift,
                                                                    float* __restrict__ g_w, double* __restrict__ g_scale,
                                                                    double* __restrict__ g_shift, int groups, int D, int ns,
                                                                    int nh) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i < D) {
    float r = 0.f;
    for (int b = 0; b < groups; ++b) r += part_w[(int64_t)b * D + i];
    g_w[i] = r;
    return;
  }
  i -= D;
  if (i < ns) {
    double r = 0.0;
    for (int b = 0; b < groups; ++b) r += part_scale[(int64_t)b * ns + i];
    g_scale[i] = r;
    return;
  }
  i -= ns;
  if (i < nh) {
    double r = 0.0;
    for (int b = 0; b < groups; ++b) r += part_shift[(int64_t)b * nh + i];
    g_shift[i] = r;
  }
}

inline int eh_groups(int64_t num_nodes) {
  const int64_t g = (num_nodes + 15) / 16;
  return (int)(g < EH_MAX_GROUPS ? g : EH_MAX_GROUPS);
}
// workspace: [groups, n_scales] + [groups, n_shifts] float64, then [groups, dim] float32
inline int64_t eh_workspace_bytes(int64_t num_nodes, int32_t dim, int32_t n_scales, int32_t n_shifts) {
  const int64_t g = eh_groups(num_nodes);
  return g * ((int64_t)(n_scales + n_shifts) * 8 + (int64_t)dim * 4);
}

static int eh_train_launch(bool second, const char* name, const void* h, const void* w, const void* scales, int32_t n_scales,
                           int32_t n_shifts, const int64_t* types, const void* grad_e, const void* v, void* g_h, void* gg_e,
                           void* g_w, void* g_scales, void* g_shifts, void* workspace, int64_t workspace_bytes, int32_t dim,
                           int32_t act, double cst, int64_t num_nodes, nqa_stream stream) {
  const int ns = g_scales != nullptr ? n_scales : 0, nh = g_shifts != nullptr ? n_shifts : 0;
  const int dw = g_w != nullptr ? dim : 0;
  if (num_nodes < 0 || dim <= 0 || (dim & 3) != 0 || dim > 64 * EH_KMAX || act < 0 || act > 2 || n_scales < 0 ||
      n_shifts < 0 || ns > EH_TABLE_MAX || nh > EH_TABLE_MAX || (g_scales != nullptr && n_scales == 0) ||
      (g_shifts != nullptr && n_shifts == 0) || (n_scales > 0 && !scales) ||
      (num_nodes > 0 && (!h || !w || !grad_e || (second && !v) || ((n_scales > 1 || nh > 1) && !types))) ||
      (eh_workspace_bytes(num_nodes, dw, ns, nh) > 0 &&
       (!workspace || workspace_bytes < eh_workspace_bytes(num_nodes, dw, ns, nh)))) {
    set_error(std::string(name) + ": invalid argument (dim a multiple of 4 up to 512, gradient tables of up to 128 entries, "
                                  "workspace of nqa_energy_head_train_workspace_bytes)");
    return NQA_ERR_INVALID;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int groups = eh_groups(num_nodes);
  double* part_scale = static_cast<double*>(workspace);
  double* part_shift = part_scale + (int64_t)groups * ns;
  float* part_w = reinterpret_cast<float*>(part_shift + (int64_t)groups * nh);
  if (num_nodes > 0) {
    EnergyHeadTrainArgs a{};
    a.h = static_cast<const float*>(h);
    a.w = static_cast<const float*>(w);
    a.scales = n_scales > 0 ? static_cast<const double*>(scales) : nullptr;
    a.types = types;
    a.g_e = static_cast<const double*>(grad_e);
    a.v = static_cast<const float*>(v);
    a.g_h = static_cast<float*>(g_h);
    a.gg_e = static_cast<double*>(gg_e);
    a.part_w = dw ? part_w : nullptr;
    a.part_scale = ns ? part_scale : nullptr;
    a.part_shift = nh ? part_shift : nullptr;
    a.N = num_nodes;
    a.D = dim;
    a.act = act;
    a.n_scales = n_scales;
    a.n_shifts = nh;
    a.cst = (float)cst;
    const size_t lds = (size_t)16 * (ns + nh) * sizeof(double) + (dw ? (size_t)4 * dim * sizeof(float) : 0);
    if (second)
      hipLaunchKernelGGL(energy_head_train_kernel<true>, dim3((unsigned)groups), dim3(256), lds, s, a);
    else
      hipLaunchKernelGGL(energy_head_train_kernel<false>, dim3((unsigned)groups), dim3(256), lds, s, a);
  }
  const int outs = dw + ns + nh;
  if (outs > 0)
    hipLaunchKernelGGL(energy_head_train_sum_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, s, part_w, part_scale,
                       part_shift, static_cast<float*>(g_w), static_cast<double*>(g_scales), static_cast<double*>(g_shifts),
                       groups, dw, ns, nh);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error(std::string(name) + ": " + hipGetErrorString(e));
    return NQA_ERR_LAUNCH;
  }
  return NQA_OK;
}

}  // namespace nqa

extern "C" {

int nqa_energy_head(int32_t backward, const void* h, const void* readout_weight, const void* scales, int32_t n_scales,
                    const void* shifts, int32_t n_shifts, const int64_t* atom_types, const void* grad_e, void* out,
                    int32_t dim, int32_t act, double cst, int64_t num_nodes, nqa_stream stream) {
  using namespace nqa;
  if (num_nodes < 0 || dim <= 0 || (dim & 3) != 0 || act < 0 || act > 2 || n_scales < 0 || n_shifts < 0 ||
      (num_nodes > 0 && (!h || !readout_weight || !out || (backward && !grad_e))) ||
      ((n_scales > 1 || n_shifts > 1) && atom_types == nullptr) || (n_scales > 0 && !scales) || (n_shifts > 0 && !shifts)) {
    set_error("nqa_energy_head: invalid argument (dim must be a positive multiple of 4)");
    return NQA_ERR_INVALID;
  }
  if (num_nodes == 0) return NQA_OK;
  EnergyHeadArgs a{};
  a.h = static_cast<const float*>(h);
  a.w = static_cast<const float*>(readout_weight);
  a.scales = n_scales > 0 ? static_cast<const double*>(scales) : nullptr;
  a.shifts = n_shifts > 0 ? static_cast<const double*>(shifts) : nullptr;
  a.types = atom_types;
  a.N = num_nodes;
  a.D = dim;
  a.act = act;
  a.n_scales = n_scales;
  a.n_shifts = n_shifts;
  a.cst = (float)cst;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (backward) {
    a.g_e = static_cast<const double*>(grad_e);
    a.g_h = static_cast<float*>(out);
    const int64_t items = num_nodes * (dim >> 2);
    hipLaunchKernelGGL(energy_head_bwd_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, a);
  } else {
    a.e_atom = static_cast<double*>(out);
    hipLaunchKernelGGL(energy_head_fwd_kernel, dim3((unsigned)((num_nodes * 16 + 255) / 256)), dim3(256), 0, s, a);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error(std::string("nqa_energy_head: ") + hipGetErrorString(e));
    return NQA_ERR_LAUNCH;
  }
  return NQA_OK;
}

int64_t nqa_energy_head_train_workspace_bytes(int64_t num_nodes, int32_t dim, int32_t n_scales, int32_t n_shifts) {
  if (num_nodes < 0 || dim < 0 || n_scales < 0 || n_shifts < 0) return -1;
  return nqa::eh_workspace_bytes(num_nodes, dim, n_scales, n_shifts);
}

int nqa_energy_head_train_bwd(const void* h, const void* readout_weight, const void* scales, int32_t n_scales,
                              int32_t n_shifts, const int64_t* atom_types, const void* grad_e, void* grad_h, void* grad_w,
                              void* grad_scales, void* grad_shifts, void* workspace, int64_t workspace_bytes, int32_t dim,
                              int32_t act, double cst, int64_t num_nodes, nqa_stream stream) {
  return nqa::eh_train_launch(false, "nqa_energy_head_train_bwd", h, readout_weight, scales, n_scales, n_shifts, atom_types,
                              grad_e, nullptr, grad_h, nullptr, grad_w, grad_scales, grad_shifts, workspace, workspace_bytes,
                              dim, act, cst, num_nodes, stream);
}

int nqa_energy_head_train_bwd_bwd(const void* h, const void* readout_weight, const void* scales, int32_t n_scales,
                                  const int64_t* atom_types, const void* grad_e, const void* cot_grad_h, void* grad_grad_e,
                                  void* grad_h, void* grad_w, void* grad_scales, void* workspace, int64_t workspace_bytes,
                                  int32_t dim, int32_t act, double cst, int64_t num_nodes, nqa_stream stream) {
  return nqa::eh_train_launch(true, "nqa_energy_head_train_bwd_bwd", h, readout_weight, scales, n_scales, 0, atom_types, grad_e,
                              cot_grad_h, grad_h, grad_grad_e, grad_w, grad_scales, nullptr, workspace, workspace_bytes, dim,
                              act, cst, num_nodes, stream);
}

}  // extern "C"
