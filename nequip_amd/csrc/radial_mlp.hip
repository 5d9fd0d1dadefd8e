// Radial network on the matrix cores: edge_weight = silu(edge_embedding @ (W0*a0)) @ (W1*a1), and its
// vector-Jacobian product w.r.t. the edge embedding (the radial leg of the force backward).
//
// Replaces ScalarMLPFunction.forward as InteractionBlock.edge_mlp (nequip/nn/interaction_block.py:119-127,196;
// nequip/nn/mlp.py:141-156,194-196,262-268: bias-free layers y = x @ (W * alpha), alpha = gain/sqrt(fan_in),
// SiLU in between) for the standard one-hidden-layer radial MLP, and the autograd of those mm/SiLU ops.
//
// This is the one true dense GEMM on the hot path ([E,H] x [H,W], K = H = 64/128).  Two interchangeable GEMM modes:
//   NQA_MLP_FP32   : exact-fp32 MFMA (v_mfma_f32_32x32x2_f32: bitwise an fp32 fma chain, 157 TFLOP/s peak);
//   NQA_MLP_BF16X6 : every fp32 operand split exactly into three bf16 terms, six partial products accumulated in fp32 on
//                    v_mfma_f32_32x32x16_bf16 (fp32-accurate, 2.7x the fp32-MFMA ceiling) -- second half of this file;
//   NQA_MLP_F16X3  : (forward) operands scaled by powers of two and split into two fp16 terms, three partial products on
//                    v_mfma_f32_32x32x16_f16 -- half the matrix instructions of BF16X6 at the same fp32-level accuracy
//                    (2^-22 per operand); the backward of this mode is the bf16 split.
// Kernel structure (both modes):
//   forward : a workgroup owns 128 edges; each wavefront keeps the SiLU-activated hidden rows of its 32 edges in
//             VGPRs as MFMA fragments for the whole kernel (the hidden layer never touches HBM) and streams
//             the second-layer weights through LDS in column chunks;
//   backward: g_h = g_w @ (W1*a1)^T with K = W streamed from HBM, then
//             g_emb = (g_h * silu'(pre)) @ (W0*a0)^T with the pre-activations recomputed from the embedding
//             (8 FMAs per element) instead of being stored.
// Roofline: 2*H*W FLOP per edge vs 4*W bytes written/read per edge: MFMA-bound in fp32 mode, between the bf16-MFMA
// and HBM roofs in split mode.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <string>
#include <type_traits>

#include "launch_status.h"
#include "mfma_split.h"

namespace nqa {

constexpr int kMlpRows = 128;  // edges per workgroup (4 wavefronts x 32 rows)
constexpr int kMaxNb = 8;    // radial basis size limit of the fused kernels (nequip default num_bessels = 8)

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains vmcnt (CDNA4 counts stores in
// vmcnt), which would make every chunk wait for its own HBM stores / prefetch loads at the barrier.
typedef float mlp_v4f __attribute__((ext_vector_type(4)));
// The weight rows are written once and read by the tensor-product kernels long after the caches have turned over:
// nontemporal stores keep them from displacing the node rows those kernels gather (cu20k: tp_fwd 2.96 -> 2.83 ms,
// radial_mlp_fwd -1 %).  Nontemporal LOADS of the gradient rows in the backward were measured too: 3.15 -> 4.1 ms, not used.
__device__ __forceinline__ void mlp_store4(float* p, const float4& v) {
  __builtin_nontemporal_store((mlp_v4f){v.x, v.y, v.z, v.w}, reinterpret_cast<mlp_v4f*>(p));
}

__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ float silu_f(float x) { return x / (1.0f + __expf(-x)); }
// silu(x), silu'(x), silu''(x) from one sigmoid (training epilogues)
__device__ __forceinline__ void silu_all_f(float x, float& h, float& d1, float& d2) {
  const float sig = 1.0f / (1.0f + __expf(-x));
  const float om = 1.0f - sig;
  h = x * sig;
  d1 = sig * (1.0f + x * om);
  d2 = sig * om * (2.0f + x * (1.0f - 2.0f * sig));
}
__device__ __forceinline__ float silu_grad_f(float x) {
  const float s = 1.0f / (1.0f + __expf(-x));
  return s * (1.0f + x * (1.0f - s));
}
// The last-layer entry points (XIN) get their pre-activations as DATA, exact as given.  __expf rounds x log2(e) to fp32
// before the hardware exponential: an error of |x| 2^-24 relative to the result, 1.8e-6 of silu'(-30), which an fp32
// evaluation of the same formula does not have (tests/test_radial_mlp_launches.py, the rows of -30).  Here the rounding
// error of that product -- recovered with one fma -- and the low part of log2(e) enter as a first-order correction.  The
// two-layer kernels keep __expf: their x = emb W0 is a rounded sum whose own error is of the same size.
__device__ __forceinline__ float exp_neg_given_f(float x) {
  constexpr float c_hi = -1.44269502162933349609375f, c_lo = -1.92596299112661746e-8f;  // -log2(e) = c_hi + c_lo
  const float t = x * c_hi;
  const float r = __builtin_fmaf(x, c_hi, -t) + x * c_lo;  // -x log2(e) = t + r
  return __builtin_amdgcn_exp2f(t) * (1.0f + r * 0.693147182f);
}
__device__ __forceinline__ float silu_given_f(float x) { return x / (1.0f + exp_neg_given_f(x)); }
__device__ __forceinline__ float silu_grad_given_f(float x) {
  const float s = 1.0f / (1.0f + exp_neg_given_f(x));
  return s * (1.0f + x * (1.0f - s));
}

// ------------------------------------------------------------------------------------------------------------
// forward: out[E, W] = silu(emb[E, NB] @ W0s[NB, H]) @ W1s[H, W]
// ------------------------------------------------------------------------------------------------------------
// MFMA 32x32x2 f32 register maps (cdna guide): A: lane l holds A[i = l&31][k = l>>5]; B: B[k = l>>5][j = l&31];
// D: 16 regs, D[i = (r&3) + 8*(r>>2) + 4*(l>>5)][j = l&31].
//
// Everything is computed transposed, with j = edge:  step 1  hT[k][e] = sum_c W0s[c][k] emb[e][c]  (4 MFMAs per
// 32 hidden rows) leaves lane (e, half) holding the hidden values k = 32*kb + (r&3) + 8*(r>>2) + 4*half -- exactly
// one value per MFMA k-pair of step 2 if step s = 16*kb + r pairs the hidden indices {kmap(s), kmap(s) + 4}.  So the
// SiLU-activated accumulators of step 1 ARE the B operands of step 2 (no shuffles, the hidden layer never leaves
// the VGPRs), and  step 2  outT[n][e] = sum_k W1s[k][n] h[e][k]  leaves lane (e, half) holding 4 consecutive output
// columns per register quad -> float4 stores.
__device__ __forceinline__ constexpr int mlp_kmap(int s) { return 32 * (s >> 4) + (s & 3) + 8 * ((s & 15) >> 2); }

// `dbg` is always 0: the host passes the constant.  Its bits selected timing ablations (removed from every other kernel
// and from the host); the never-taken tests stay in this kernel's text because without them the compiler allocates 2-8
// more VGPRs for six instantiations, the default backward among them (profiles/mlp_refactor_kernel_resources_*.txt).
template <int H>
__global__ __launch_bounds__(256) void radial_mlp_fwd_kernel(const float* __restrict__ emb,
                                                             const float* __restrict__ W0,
                                                             const float* __restrict__ W1, float a0, float a1,
                                                             int nb, int W, int64_t E, float* __restrict__ out,
                                                             int dbg) {
  constexpr int BN = 64;            // output columns per chunk
  constexpr int KP = H / 2;         // MFMA k-pairs
  __shared__ float w0s[H * kMaxNb];  // [k][c] (c contiguous)
  __shared__ float bs[2][H * BN];    // double-buffered W1 chunk [k][n]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int half = lane >> 5;
  const int l31 = lane & 31;
  const int64_t row0 = (int64_t)blockIdx.x * kMlpRows + wv * 32;
  const int64_t myrow = row0 + l31;
  const bool row_ok = myrow < E;

  for (int i = tid; i < H * kMaxNb; i += 256) {
    const int k = i / kMaxNb, c = i - k * kMaxNb;
    w0s[i] = c < nb ? W0[c * H + k] * a0 : 0.f;  // zero padding: the k-pair loop runs over kMaxNb
  }
  const int nchunks = (W + BN - 1) / BN;
  // global -> registers (issued early) and registers -> LDS (written late): the L2 latency of the next W1 chunk
  // hides under the MFMAs of the current one
  constexpr int NV = H * (BN / 4) / 256;  // float4 per thread per chunk
  float4 pre4[NV];
  auto stage_load = [&](int n0) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int i = tid + v * 256;
      const int k = i / (BN / 4), q = i - k * (BN / 4);
      const int n = n0 + q * 4;
      float4 t4 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (n + 3 < W) t4 = *reinterpret_cast<const float4*>(W1 + (int64_t)k * W + n);  // W % 4 == 0
      pre4[v] = t4;
    }
  };
  auto stage_store = [&](int buf) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int i = tid + v * 256;
      const int k = i / (BN / 4), q = i - k * (BN / 4);
      float4 t4 = pre4[v];
      t4.x *= a1; t4.y *= a1; t4.z *= a1; t4.w *= a1;
      *reinterpret_cast<float4*>(&bs[buf][k * BN + q * 4]) = t4;
    }
  };
  stage_load(0);
  stage_store(0);
  __syncthreads();

  // ---- step 1: hidden layer on MFMA, SiLU in registers -----------------------------------------------------
  float hreg[KP];  // hreg[s] = h[myrow][mlp_kmap(s) + 4*half]
  {
    float ev[kMaxNb];
#pragma unroll
    for (int c = 0; c < kMaxNb; ++c) ev[c] = (c < nb && row_ok) ? emb[myrow * nb + c] : 0.f;
#pragma unroll
    for (int kb = 0; kb < H / 32; ++kb) {
      f32x16 hacc = {0};
#pragma unroll
      for (int s2 = 0; s2 < kMaxNb / 2; ++s2) {
        const float av = w0s[(kb * 32 + l31) * kMaxNb + 2 * s2 + half];  // A[i = hidden][c]
        const float bv = half ? ev[2 * s2 + 1] : ev[2 * s2];               // B[c][j = edge]
        hacc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, hacc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) hreg[kb * 16 + r] = row_ok ? silu_f(hacc[r]) : 0.f;
    }
  }

  // ---- step 2: out^T chunks -----------------------------------------------------------------------------------
  for (int ch = 0; ch < nchunks; ++ch) {
    const int buf = ch & 1;
    if (ch + 1 < nchunks && !(dbg & 2)) stage_load((ch + 1) * BN);
    const float* __restrict__ b = bs[buf] + (4 * half) * BN + l31;
    f32x16 acc0 = {0}, acc1 = {0};
    // W1 fragments are fetched from LDS one register batch (TB k-pairs) ahead of the MFMAs that consume them
    constexpr int TB = 8;
    float bq[2][TB][2];
#pragma unroll
    for (int i = 0; i < TB; ++i) {
      bq[0][i][0] = b[mlp_kmap(i) * BN];
      bq[0][i][1] = b[mlp_kmap(i) * BN + 32];
    }
#pragma unroll
    for (int tb = 0; tb < KP / TB; ++tb) {
      if (tb + 1 < KP / TB) {
#pragma unroll
        for (int i = 0; i < TB; ++i) {
          bq[(tb + 1) & 1][i][0] = b[mlp_kmap((tb + 1) * TB + i) * BN];
          bq[(tb + 1) & 1][i][1] = b[mlp_kmap((tb + 1) * TB + i) * BN + 32];
        }
      }
      // pin the order: the compiler otherwise sinks each LDS read next to its MFMA and waits lgkmcnt(0) per pair
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < TB; ++i) {
        // A[i = n][k] = W1s[k][n] (LDS), B[k][j = edge] = h (registers)
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[tb & 1][i][0], hreg[tb * TB + i], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[tb & 1][i][1], hreg[tb * TB + i], acc1, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // next chunk registers -> LDS first (its loads were issued before the MFMAs and have landed), then the output
    // stores of this chunk, which nothing below waits for (lds_barrier does not drain vmcnt)
    if (ch + 1 < nchunks && !(dbg & 2)) stage_store(buf ^ 1);
    const int n0 = ch * BN;
    if (dbg & 1) {
      if (acc0[0] == 12345.f && acc1[3] == 777.f) out[0] = 1.f;  // ablation: keep the MFMAs live, skip the stores
    } else if (row_ok) {
      // lane (edge, half) holds columns n0 + 32*tile + 8*g + 4*half + (0..3) in registers 4g..4g+3
      float* __restrict__ o = out + myrow * W + n0 + 4 * half;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c0 = n0 + 4 * half + 8 * g;
        if (c0 + 3 < W)
          *reinterpret_cast<float4*>(o + 8 * g) = make_float4(acc0[4 * g], acc0[4 * g + 1], acc0[4 * g + 2], acc0[4 * g + 3]);
        if (c0 + 32 + 3 < W)
          *reinterpret_cast<float4*>(o + 32 + 8 * g) =
              make_float4(acc1[4 * g], acc1[4 * g + 1], acc1[4 * g + 2], acc1[4 * g + 3]);
      }
    }
    lds_barrier();
  }
}

// ------------------------------------------------------------------------------------------------------------
// backward: g_emb[E, NB] = ((g_w[E, W] @ W1s^T[W, H]) * silu'(pre)) @ W0s^T[H, NB]
// ------------------------------------------------------------------------------------------------------------
// W1s^T, scaled by a1, in k-major order ([W][H]) so that the B tiles of the main loop are contiguous.
__global__ __launch_bounds__(256) void radial_mlp_transpose_w1_kernel(const float* __restrict__ W1, float a1, int H,
                                                                      int W, float* __restrict__ W1T) {
  const int i = blockIdx.x * 256 + threadIdx.x;  // over W * H, n fastest
  if (i >= W * H) return;
  const int k = i / H, n = i - k * H;
  W1T[i] = W1[(int64_t)n * W + k] * a1;
}

template <int H>
__global__ __launch_bounds__(256) void radial_mlp_bwd_kernel(const float* __restrict__ emb,
                                                             const float* __restrict__ W0,
                                                             const float* __restrict__ W1T,
                                                             const float* __restrict__ gw, float a0, int nb, int W,
                                                             int64_t E, float* __restrict__ g_emb) {
  // K (= W, the forward's output columns) is consumed in chunks of BK = 64.  MFMA k-pairing: at step kp the lanes
  // of half h contribute k = k0 + 32 h + kp, so every lane needs 32 *contiguous* floats of its own g_w row per
  // chunk: the A operand goes HBM -> registers directly (one full 128 B line per lane and chunk, no LDS), only the
  // shared B tile (W1s^T chunk [64][H]) is staged through LDS.
  constexpr int BK = 64;
  constexpr int NT = H / 32;        // 32-wide column tiles of the hidden layer per wavefront
  constexpr int GS = H + 1;         // padded row stride of the g_pre tile
  constexpr int kMain = 2 * BK * H;  // double-buffered B tile
  constexpr int kEpi = kMlpRows * GS;
  constexpr int kBuf = kMain > kEpi ? kMain : kEpi;
  __shared__ float smem[kBuf];
  __shared__ float w0s[H * kMaxNb];        // [k][c]
  __shared__ float w0t[kMaxNb * H];        // [c][k]
  __shared__ float es[kMlpRows * kMaxNb];  // embedding tile [row][c]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int half = lane >> 5;
  const int l31 = lane & 31;
  const int64_t blk0 = (int64_t)blockIdx.x * kMlpRows;
  const int64_t myrow = blk0 + wv * 32 + l31;
  const bool row_ok = myrow < E;

  for (int i = tid; i < H * kMaxNb; i += 256) {
    const int k = i / kMaxNb, c = i - k * kMaxNb;
    const float v = c < nb ? W0[c * H + k] * a0 : 0.f;
    w0s[i] = v;
    w0t[c * H + k] = v;
  }
  for (int i = tid; i < kMlpRows * kMaxNb; i += 256) {
    const int r = i / kMaxNb, c = i - r * kMaxNb;
    es[i] = (c < nb && blk0 + r < E) ? emb[(blk0 + r) * nb + c] : 0.f;
  }

  const int nchunks = (W + BK - 1) / BK;
  constexpr int NB4 = BK * H / 4 / 256;  // float4 per thread per B tile
  float4 pb[NB4];
  float4 pa[BK / 2 / 4];                 // this lane's 32 floats of the next chunk
  const float* __restrict__ grow = gw + (row_ok ? myrow : 0) * W + 32 * half;
  auto load_a = [&](int k0) {
#pragma unroll
    for (int v = 0; v < BK / 2 / 4; ++v) {
      const int k = k0 + 32 * half + 4 * v;
      pa[v] = (row_ok && k + 3 < W) ? *reinterpret_cast<const float4*>(grow + k0 + 4 * v)
                                    : make_float4(0.f, 0.f, 0.f, 0.f);  // W % 4 == 0
    }
  };
  auto load_b = [&](int k0) {
#pragma unroll
    for (int v = 0; v < NB4; ++v) {
      const int i = (tid + v * 256) * 4;  // element index inside the [BK][H] tile
      const int k = k0 + i / H;
      pb[v] = k < W ? *reinterpret_cast<const float4*>(W1T + (int64_t)k0 * H + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto store_b = [&](int buf) {
    float* __restrict__ bs = smem + buf * BK * H;
#pragma unroll
    for (int v = 0; v < NB4; ++v) *reinterpret_cast<float4*>(bs + (tid + v * 256) * 4) = pb[v];
  };
  load_b(0);
  load_a(0);
  store_b(0);
  __syncthreads();

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (f32x16){0};

  for (int ch = 0; ch < nchunks; ++ch) {
    const int buf = ch & 1;
    // A fragments of this chunk (registers), then prefetch the next chunk's A (HBM) and B (L2) behind the MFMAs
    float av[BK / 2];
#pragma unroll
    for (int v = 0; v < BK / 2 / 4; ++v) {
      av[4 * v + 0] = pa[v].x;
      av[4 * v + 1] = pa[v].y;
      av[4 * v + 2] = pa[v].z;
      av[4 * v + 3] = pa[v].w;
    }
    if (ch + 1 < nchunks) {
      load_a((ch + 1) * BK);
      load_b((ch + 1) * BK);
    }
    const float* __restrict__ bs = smem + buf * BK * H + (32 * half) * H + l31;
    constexpr int TB = 8;  // k-steps per register batch of B fragments
    float bq[2][TB][NT];
#pragma unroll
    for (int i = 0; i < TB; ++i)
#pragma unroll
      for (int t = 0; t < NT; ++t) bq[0][i][t] = bs[i * H + t * 32];
#pragma unroll
    for (int tb = 0; tb < BK / 2 / TB; ++tb) {
      if (tb + 1 < BK / 2 / TB) {
#pragma unroll
        for (int i = 0; i < TB; ++i)
#pragma unroll
          for (int t = 0; t < NT; ++t) bq[(tb + 1) & 1][i][t] = bs[((tb + 1) * TB + i) * H + t * 32];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < TB; ++i)
#pragma unroll
        for (int t = 0; t < NT; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tb * TB + i], bq[tb & 1][i][t], acc[t], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (ch + 1 < nchunks) store_b(buf ^ 1);
    lds_barrier();
  }

  // epilogue: pre-activations recomputed on MFMA in the accumulator layout (pre[row][k] = sum_c emb[row][c] W0s[c][k]:
  // 4 MFMAs per 32x32 tile), g_pre = g_h * silu'(pre) in registers, one pass through LDS for the NB-wide GEMV
  float* __restrict__ gp = smem;  // re-uses the staging buffers (all waves passed the last lds_barrier)
  {
    const float* __restrict__ erow = es + (wv * 32 + l31) * kMaxNb;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x16 pacc = {0};
#pragma unroll
      for (int s2 = 0; s2 < kMaxNb / 2; ++s2) {
        const float av = erow[2 * s2 + half];                          // A[i = row][c]
        const float bv = w0t[(2 * s2 + half) * H + t * 32 + l31];      // B[c][j = hidden]
        pacc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, pacc, 0, 0, 0);
      }
      const int col = t * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int lr = wv * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;  // row within the block
        gp[lr * GS + col] = acc[t][r] * silu_grad_f(pacc[r]);
      }
    }
  }
  __syncthreads();
  {
    // g_emb[r][c] = sum_k g_pre[r][k] W0s[c][k]: two threads per row, each over half of k, all NB columns at once
    const int r = tid >> 1, kh = tid & 1;
    float sacc[kMaxNb];
#pragma unroll
    for (int c = 0; c < kMaxNb; ++c) sacc[c] = 0.f;
    const float* __restrict__ gr = gp + r * GS + kh * (H / 2);
    const float* __restrict__ wr = w0s + kh * (H / 2) * kMaxNb;
#pragma unroll 4
    for (int k = 0; k < H / 2; ++k) {
      const float gv = gr[k];
      const float4 w0 = *reinterpret_cast<const float4*>(wr + k * kMaxNb);
      const float4 w1 = *reinterpret_cast<const float4*>(wr + k * kMaxNb + 4);
      sacc[0] += gv * w0.x; sacc[1] += gv * w0.y; sacc[2] += gv * w0.z; sacc[3] += gv * w0.w;
      sacc[4] += gv * w1.x; sacc[5] += gv * w1.y; sacc[6] += gv * w1.z; sacc[7] += gv * w1.w;
    }
#pragma unroll
    for (int c = 0; c < kMaxNb; ++c) sacc[c] += __shfl_xor(sacc[c], 1, 64);
    if (kh == 0 && blk0 + r < E) {
      for (int c = 0; c < nb; ++c) g_emb[(blk0 + r) * nb + c] = sacc[c];
    }
  }
}

// ============================================================================================================
// Split-operand variants: fp32-accurate GEMMs on the bf16 ("bf16x6") and fp16 ("f16x3") matrix cores; the splits and
// their error analysis are in mfma_split.h.
// ============================================================================================================
// The split moves both kernels from MFMA-bound to HBM-bound (the forward writes, the backward reads, 4*W bytes per
// edge).  Weights are split once per call by a small prepass kernel that also lays them out in fragment order (one
// contiguous 1 KiB wave read per fragment, conflict-free ds_read_b128), so staging a tile into LDS is a plain copy.
// The power-of-two scales of the fp16 split: weights per 32-column tile (prepass), hidden activations per row (in
// registers, the row's values sit in one lane pair).  That applies where the scale of a row is known before its first
// k-step, i.e. to the forward GEMM; the backward streams the gradient rows and scales them per chunk.

// hidden index held by lane-half `half`, element t of bf16 k-step s, when the hidden layer is produced by the
// transposed fp32 MFMA of step 1 (accumulator register r = 8*(s&1) + t of 32-row block s>>1)
__device__ __forceinline__ constexpr int mlp_hmap(int s, int half, int t) {
  return 32 * (s >> 1) + (t & 3) + 8 * (2 * (s & 1) + (t >> 2)) + 4 * half;
}

// Forward weight fragments: Wf[tile][s][split][lane] (uint4) = A[i = column 32*tile + (lane&31)][k-step s, half, t]
// of W1s^T with the hidden order of mlp_hmap; split 0/1/2 = hi/mid/lo.
__global__ __launch_bounds__(256) void radial_mlp_split_w1_fwd_kernel(const float* __restrict__ W1, float a1, int H,
                                                                      int W, u32x4* __restrict__ Wf) {
  const int KS = H / 16;
  const int ntiles = (W + 31) / 32;
  const int idx = blockIdx.x * 256 + threadIdx.x;  // (tile, s, lane)
  if (idx >= ntiles * KS * 64) return;
  const int lane = idx & 63, s = (idx >> 6) % KS, tile = idx / (64 * KS);
  const int n = 32 * tile + (lane & 31), half = lane >> 5;
  u32x4 h, m, l;
#pragma unroll
  for (int tp = 0; tp < 4; ++tp) {
    const float v0 = n < W ? W1[(int64_t)mlp_hmap(s, half, 2 * tp) * W + n] * a1 : 0.f;
    const float v1 = n < W ? W1[(int64_t)mlp_hmap(s, half, 2 * tp + 1) * W + n] * a1 : 0.f;
    uint32_t a, b, c;
    split_pair(v0, v1, a, b, c);
    h[tp] = a; m[tp] = b; l[tp] = c;
  }
  u32x4* __restrict__ o = Wf + ((int64_t)(tile * KS + s) * 3) * 64 + lane;
  o[0] = h; o[64] = m; o[128] = l;
}

// f16x3 forward weight fragments: Wf[tile][s][plane][lane] (plane 0 / 1 = h / l) of the tile scaled by a power of two,
// tile_scale[tile] = the inverse power (multiplied back on the accumulators).  One workgroup per tile: the maximum over
// the tile's H x 32 values comes first.
__global__ __launch_bounds__(256) void radial_mlp_split_w1_fwd_f16_kernel(const float* __restrict__ W1, float a1, int H,
                                                                          int W, u32x4* __restrict__ Wf,
                                                                          float* __restrict__ tile_scale) {
  __shared__ float red[4];
  const int KS = H / 16;
  const int tile = blockIdx.x;
  const int tid = threadIdx.x;
  float m = 0.f;
  for (int i = tid; i < H * 32; i += 256) {
    const int k = i >> 5, n = 32 * tile + (i & 31);
    if (n < W) m = fmaxf(m, fabsf(W1[(int64_t)k * W + n] * a1));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float su = f16_scale_up(m);
  if (tid == 0) tile_scale[tile] = 1.f / su;
  for (int idx = tid; idx < KS * 64; idx += 256) {
    const int lane = idx & 63, s = idx >> 6;
    const int n = 32 * tile + (lane & 31), half = lane >> 5;
    u32x4 h, l;
#pragma unroll
    for (int tp = 0; tp < 4; ++tp) {
      const float v0 = n < W ? W1[(int64_t)mlp_hmap(s, half, 2 * tp) * W + n] * a1 * su : 0.f;
      const float v1 = n < W ? W1[(int64_t)mlp_hmap(s, half, 2 * tp + 1) * W + n] * a1 * su : 0.f;
      uint32_t a, b;
      split_pair_f16(v0, v1, a, b);
      h[tp] = a; l[tp] = b;
    }
    u32x4* __restrict__ o = Wf + ((int64_t)(tile * KS + s) * 2) * 64 + lane;
    o[0] = h; o[64] = l;
  }
}

// Backward weight fragments: Wb[chunk][s][split][nt][lane] = B[k = 32*chunk + 16*half + 8*s + t][j = 32*nt + (lane&31)]
// of W1s^T, i.e. 8 consecutive floats of row j of W1s.
__global__ __launch_bounds__(256) void radial_mlp_split_w1_bwd_kernel(const float* __restrict__ W1, float a1, int H,
                                                                      int W, u32x4* __restrict__ Wb) {
  const int NT = H / 32;
  const int nchunks = (W + 31) / 32;
  const int idx = blockIdx.x * 256 + threadIdx.x;  // (chunk, s, nt, lane)
  if (idx >= nchunks * 2 * NT * 64) return;
  const int lane = idx & 63, nt = (idx >> 6) % NT, s = (idx / (64 * NT)) & 1, chunk = idx / (128 * NT);
  const int j = 32 * nt + (lane & 31), half = lane >> 5;
  const int k0 = 32 * chunk + 16 * half + 8 * s;
  u32x4 h, m, l;
#pragma unroll
  for (int tp = 0; tp < 4; ++tp) {
    const int k = k0 + 2 * tp;
    const float v0 = k < W ? W1[(int64_t)j * W + k] * a1 : 0.f;
    const float v1 = k + 1 < W ? W1[(int64_t)j * W + k + 1] * a1 : 0.f;
    uint32_t a, b, c;
    split_pair(v0, v1, a, b, c);
    h[tp] = a; m[tp] = b; l[tp] = c;
  }
  u32x4* __restrict__ o = Wb + ((int64_t)((chunk * 2 + s) * 3) * NT + nt) * 64 + lane;
  o[0] = h; o[(int64_t)NT * 64] = m; o[(int64_t)2 * NT * 64] = l;
}

// f16x3 backward weight fragments: Wb[chunk][s][plane][nt][lane] (plane 0 / 1 = h / l) of the 32-row K chunk scaled by
// 2^chunk_exp[chunk] (largest magnitude into [2^14, 2^15); exponent clamped to +-100).  One workgroup per chunk.
__global__ __launch_bounds__(256) void radial_mlp_split_w1_bwd_f16_kernel(const float* __restrict__ W1, float a1, int H,
                                                                          int W, u32x4* __restrict__ Wb,
                                                                          int* __restrict__ chunk_exp) {
  __shared__ float red[4];
  const int NT = H / 32;
  const int chunk = blockIdx.x;
  const int tid = threadIdx.x;
  float m = 0.f;
  for (int i = tid; i < H * 32; i += 256) {
    const int j = i >> 5, k = 32 * chunk + (i & 31);
    if (k < W) m = fmaxf(m, fabsf(W1[(int64_t)j * W + k] * a1));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  int ex = 0;
  if (m > 0.f && m < 3.0e38f) {
    int e;
    (void)frexpf(m, &e);
    ex = 15 - e;
    ex = ex > 100 ? 100 : (ex < -100 ? -100 : ex);
  }
  const float su = ldexpf(1.f, ex);
  if (tid == 0) chunk_exp[chunk] = ex;
  for (int idx = tid; idx < 2 * NT * 64; idx += 256) {  // (s, nt, lane)
    const int lane = idx & 63, nt = (idx >> 6) % NT, sk = idx / (64 * NT);
    const int j = 32 * nt + (lane & 31), half = lane >> 5;
    const int k0 = 32 * chunk + 16 * half + 8 * sk;
    u32x4 h, l;
#pragma unroll
    for (int tp = 0; tp < 4; ++tp) {
      const int k = k0 + 2 * tp;
      const float v0 = k < W ? W1[(int64_t)j * W + k] * a1 * su : 0.f;
      const float v1 = k + 1 < W ? W1[(int64_t)j * W + k + 1] * a1 * su : 0.f;
      uint32_t a, b;
      split_pair_f16(v0, v1, a, b);
      h[tp] = a; l[tp] = b;
    }
    u32x4* __restrict__ o = Wb + ((int64_t)((chunk * 2 + sk) * 2) * NT + nt) * 64 + lane;
    o[0] = h; o[(int64_t)NT * 64] = l;
  }
}

// The four wavefronts (32 edges each) share every staged weight tile (1.7 GB of L2 -> LDS weight traffic per
// middle-layer launch, i.e. the whole L2 bandwidth for ~100 us).
// TAN (nqa_radial_mlp_fwd_tangent): the hidden layer fed to the second GEMM is (cemb W0) silu'(emb W0) instead of
// silu(emb W0) -- the directional derivative of the MLP along cemb; only step 1 differs.
template <int H, bool TAN = false>
__global__ __launch_bounds__(256, 2) void radial_mlp_fwd_bf16x6_kernel(const float* __restrict__ emb,
                                                                    const float* __restrict__ W0,
                                                                    const u32x4* __restrict__ Wf, float a0, int nb,
                                                                    int W, int64_t E, float* __restrict__ out,
                                                                    const float* __restrict__ cemb = nullptr) {
  constexpr int NW = 4;                 // wavefronts per workgroup
  constexpr int KS = H / 16;            // bf16 k-steps
  constexpr int TILE = KS * 3 * 64;     // uint4 per 32-column weight tile (24 KiB for H = 128)
  constexpr int NTH = NW * 64;          // threads per workgroup
  constexpr int NV = TILE / NTH;        // uint4 per thread per tile
  static_assert(TILE % NTH == 0, "tile must divide evenly over the workgroup");
  constexpr int kTS = 36;               // padded row stride (floats) of the per-wave output transpose tile
  __shared__ float w0s[H * kMaxNb];     // [k][c]
  __shared__ u32x4 as[2][TILE];
  __shared__ __align__(16) float tbuf[NW * 32 * kTS];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int half = lane >> 5;
  const int l31 = lane & 31;
  const int64_t myrow = (int64_t)blockIdx.x * (NW * 32) + wv * 32 + l31;
  const bool row_ok = myrow < E;

  // this lane's embedding row first: its HBM latency overlaps the weight staging below
  // (unpredicated loads from a clamped row, masked afterwards: per-element predicates would turn into eight
  // branch + load + wait sequences, i.e. eight serial HBM round trips before the first MFMA)
  float ev[kMaxNb];
  {
    const float* __restrict__ er = emb + (row_ok ? myrow : (E - 1)) * nb;
    if (nb == kMaxNb) {
      const float4 e0 = *reinterpret_cast<const float4*>(er);
      const float4 e1 = *reinterpret_cast<const float4*>(er + 4);
      ev[0] = e0.x; ev[1] = e0.y; ev[2] = e0.z; ev[3] = e0.w;
      ev[4] = e1.x; ev[5] = e1.y; ev[6] = e1.z; ev[7] = e1.w;
    } else {
#pragma unroll
      for (int c = 0; c < kMaxNb; ++c) ev[c] = er[c < nb ? c : nb - 1];
#pragma unroll
      for (int c = 0; c < kMaxNb; ++c) ev[c] = c < nb ? ev[c] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < kMaxNb; ++c) ev[c] = row_ok ? ev[c] : 0.f;
  }
  float cv[kMaxNb];
  if (TAN) {
    const float* __restrict__ cr = cemb + (row_ok ? myrow : (E - 1)) * nb;
#pragma unroll
    for (int c = 0; c < kMaxNb; ++c) cv[c] = cr[c < nb ? c : nb - 1];
#pragma unroll
    for (int c = 0; c < kMaxNb; ++c) cv[c] = (row_ok && c < nb) ? cv[c] : 0.f;
  }
  for (int i = tid; i < H * kMaxNb; i += NTH) {
    const int k = i / kMaxNb, c = i - k * kMaxNb;
    w0s[i] = c < nb ? W0[c * H + k] * a0 : 0.f;
  }
  const int ntiles = (W + 31) / 32;
  u32x4 pre[NV];
  auto stage_load = [&](int tile) {
#pragma unroll
    for (int v = 0; v < NV; ++v) pre[v] = Wf[(int64_t)tile * TILE + tid + v * NTH];
  };
  auto stage_store = [&](int buf) {
#pragma unroll
    for (int v = 0; v < NV; ++v) as[buf][tid + v * NTH] = pre[v];
  };
  // Weight tiles are fetched two tiles ahead (global -> registers during tile t-1, registers -> LDS at the start of
  // tile t, consumed in tile t+1): vmcnt retires in order and also counts the output stores, so waiting for a
  // prefetch issued only one tile ago would wait for the previous tile's HBM stores as well.
  stage_load(0);
  stage_store(0);
  if (ntiles > 1) stage_load(1);
  __syncthreads();

  // ---- step 1: hidden layer (K = nb <= 8) in exact fp32 on MFMA, SiLU, split into bf16 B fragments ---------------
  u32x4 bh[KS], bm[KS], bl[KS];
  {
#pragma unroll
    for (int kb = 0; kb < H / 32; ++kb) {
      f32x16 hacc = {0};
#pragma unroll
      for (int s2 = 0; s2 < kMaxNb / 2; ++s2) {
        const float av = w0s[(kb * 32 + l31) * kMaxNb + 2 * s2 + half];
        const float bv = half ? ev[2 * s2 + 1] : ev[2 * s2];
        hacc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, hacc, 0, 0, 0);
      }
      f32x16 qacc = {0};
      if (TAN) {
#pragma unroll
        for (int s2 = 0; s2 < kMaxNb / 2; ++s2) {
          const float av = w0s[(kb * 32 + l31) * kMaxNb + 2 * s2 + half];
          const float bv = half ? cv[2 * s2 + 1] : cv[2 * s2];
          qacc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, qacc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const float h0 = row_ok ? (TAN ? qacc[r] * silu_grad_f(hacc[r]) : silu_f(hacc[r])) : 0.f;
        const float h1 = row_ok ? (TAN ? qacc[r + 1] * silu_grad_f(hacc[r + 1]) : silu_f(hacc[r + 1])) : 0.f;
        uint32_t a, b, c;
        split_pair(h0, h1, a, b, c);
        const int s = 2 * kb + (r >> 3), tp = (r & 7) >> 1;
        bh[s][tp] = a; bm[s][tp] = b; bl[s][tp] = c;
      }
    }
  }

  // ---- step 2: out^T tiles of 32 columns -----------------------------------------------------------------------
  // Two accumulator sets alternate between tiles: the epilogue of tile t-1 (accumulator read-out, 4 float4 stores)
  // is emitted after the first k-steps of tile t have been queued on the matrix pipe, so it overlaps with them
  // instead of draining the pipe at every tile boundary.
  // The accumulator layout gives every lane 16 B pieces of 32 different rows; stored directly, each store
  // instruction would touch 32 lines with 32 B each.  A wave-private LDS transpose (4 KiB) turns the tile into
  // row-major order so that each store instruction writes 8 complete 128 B row segments.
  float* __restrict__ tb = tbuf + wv * (32 * kTS);
  const int64_t wrow0 = (int64_t)blockIdx.x * (NW * 32) + wv * 32;
  auto emit = [&](const f32x16& pa, const f32x16& pb, int tile) {
    // lane (edge, half) holds columns 8*g + 4*half + (0..3) of its row in registers 4g..4g+3
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4*>(tb + l31 * kTS + 8 * g + 4 * half) =
          make_float4(pa[4 * g] + pb[4 * g], pa[4 * g + 1] + pb[4 * g + 1], pa[4 * g + 2] + pb[4 * g + 2],
                      pa[4 * g + 3] + pb[4 * g + 3]);
    const int n0 = tile * 32;
    const int c4 = lane & 7, rsub = lane >> 3;
    if (wrow0 + 32 <= E && n0 + 32 <= W) {  // wave-uniform common case: full tile, unpredicated stores
      float* __restrict__ ob = out + (wrow0 + rsub) * W + n0 + 4 * c4;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        mlp_store4(ob + (int64_t)(8 * i) * W, *reinterpret_cast<const float4*>(tb + (8 * i + rsub) * kTS + 4 * c4));
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 8 * i + rsub;
        const float4 v = *reinterpret_cast<const float4*>(tb + r * kTS + 4 * c4);
        if (wrow0 + r < E && n0 + 4 * c4 + 3 < W) *reinterpret_cast<float4*>(out + (wrow0 + r) * W + n0 + 4 * c4) = v;
      }
    }
  };
  auto tile_body = [&](int tile, f32x16& accA, f32x16& accB, const f32x16& prevA, const f32x16& prevB) {
    const int buf = tile & 1;
    if (tile + 1 < ntiles) stage_store(buf ^ 1);
    if (tile + 2 < ntiles) stage_load(tile + 2);
    const u32x4* __restrict__ a = as[buf] + lane;
    accA = (f32x16){0};  // large partial products
    accB = (f32x16){0};  // small partial products, summed with accA at the end
    u32x4 fa[2][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) fa[0][q] = a[q * 64];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      if (s + 1 < KS) {
#pragma unroll
        for (int q = 0; q < 3; ++q) fa[(s + 1) & 1][q] = a[((s + 1) * 3 + q) * 64];
      }
      __builtin_amdgcn_sched_barrier(0);
      const int sb = s & 1;
      const u32x4 &ah = fa[sb][0], &am = fa[sb][1], &al = fa[sb][2];
      accA = mfma_bf16(ah, bh[s], accA);
      accB = mfma_bf16(am, bm[s], accB);
      accA = mfma_bf16(ah, bm[s], accA);
      accB = mfma_bf16(ah, bl[s], accB);
      accA = mfma_bf16(am, bh[s], accA);
      accB = mfma_bf16(al, bh[s], accB);
      __builtin_amdgcn_sched_barrier(0);
      if (s == 1 && tile > 0) {
        emit(prevA, prevB, tile - 1);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    lds_barrier();
  };
  f32x16 a0A, a0B, a1A, a1B;
  for (int tile = 0; tile < ntiles; tile += 2) {
    tile_body(tile, a0A, a0B, a1A, a1B);
    if (tile + 1 < ntiles) tile_body(tile + 1, a1A, a1B, a0A, a0B);
  }
  if (ntiles & 1)
    emit(a0A, a0B, ntiles - 1);
  else
    emit(a1A, a1B, ntiles - 1);
}

// Balanced forward (inference): the launch is a fixed grid of 2 workgroups per CU, and workgroup g owns the contiguous
// range [g U / G, (g + 1) U / G) of the U = (128-row blocks) x (32-column tiles) work units in block-major order.
// With one workgroup per block the 1565 blocks of the cfg-3 pair list run in 3.06 rounds over the 512 slots -- the
// fourth, almost empty round costs a quarter of the kernel; here every slot gets 67.2 +- 1 tiles.  K is never split
// (a unit is a complete 128 x 32 output tile), so no fix-up pass is needed; a workgroup that enters a block in the
// middle recomputes that block's hidden layer (about 0.7 tile-times, at most two extra blocks per workgroup).
// The tile pipeline (weight tiles two ahead, alternating accumulator sets, epilogue of unit i-1 behind the first
// k-steps of unit i) runs straight across block boundaries; the next block's embedding row is requested one tile early.
// F16: the second GEMM on the two-plane fp16 split (three products per k-step, weight tiles of 16 KiB, tile_scale from
// the prepass) instead of the three-plane bf16 split (six products, 24 KiB tiles).
// XIN: the last layer of a deeper MLP (nqa_radial_mlp_last_fwd): `emb` holds the PRE-activations [E, H] of the layer's
// input (written by the previous fused launch); the hidden rows are silu(pre), loaded in the accumulator layout of the
// K = num_basis MFMA they replace (four float4 per 32-channel block and lane).  W0 / a0 / nb are unused.
template <int H, bool F16, bool XIN = false>
__global__ __launch_bounds__(256, 2) void radial_mlp_fwd_split_bal_kernel(const float* __restrict__ emb,
                                                                       const float* __restrict__ W0,
                                                                       const u32x4* __restrict__ Wf, float a0, int nb,
                                                                       int W, int64_t E, float* __restrict__ out,
                                                                       const float* __restrict__ tile_scale) {
  constexpr int KS = H / 16;
  constexpr int NPL = F16 ? 2 : 3;      // operand planes
  constexpr int TILE = KS * NPL * 64;
  constexpr int NTH = 256;
  constexpr int NV = TILE / NTH;
  static_assert(TILE % NTH == 0, "tile must divide evenly over the workgroup");
  constexpr int kTS = 36;
  // (the first-layer weights come straight from global memory -- L2 -- once per block, in the A-fragment order of the
  // hidden-layer MFMA: 2 KiB per wavefront, and 4 KiB of LDS less: three workgroups per CU fit in F16 mode)
  __shared__ u32x4 as[2][TILE];
  __shared__ __align__(16) float tbuf[4 * 32 * kTS];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int half = lane >> 5;
  const int l31 = lane & 31;
  const int ntiles = (W + 31) / 32;
  const int64_t nblk = (E + kMlpRows - 1) / kMlpRows;
  const int64_t U = nblk * ntiles;
  const int64_t u0 = U * (int64_t)blockIdx.x / gridDim.x;
  const int64_t u1 = U * ((int64_t)blockIdx.x + 1) / gridDim.x;
  if (u0 >= u1) return;  // (workgroup-uniform)

  auto load_ev = [&](int64_t blk, float (&ev)[kMaxNb]) __attribute__((always_inline)) {
    if constexpr (XIN) return;  // (the pre-activation rows are loaded where they are consumed)
    const int64_t row = blk * kMlpRows + wv * 32 + l31;
    const float* __restrict__ er = emb + (row < E ? row : (E - 1)) * nb;
    if (nb == kMaxNb) {
      const float4 e0 = *reinterpret_cast<const float4*>(er);
      const float4 e1 = *reinterpret_cast<const float4*>(er + 4);
      ev[0] = e0.x; ev[1] = e0.y; ev[2] = e0.z; ev[3] = e0.w;
      ev[4] = e1.x; ev[5] = e1.y; ev[6] = e1.z; ev[7] = e1.w;
    } else {
#pragma unroll
      for (int c = 0; c < kMaxNb; ++c) ev[c] = er[c < nb ? c : nb - 1];
#pragma unroll
      for (int c = 0; c < kMaxNb; ++c) ev[c] = c < nb ? ev[c] : 0.f;
    }
  };
  int64_t blk = u0 / ntiles;
  int t = (int)(u0 - blk * ntiles);
  float ev[kMaxNb], evn[kMaxNb];
  load_ev(blk, ev);
#pragma unroll
  for (int c = 0; c < kMaxNb; ++c) evn[c] = 0.f;
  u32x4 pre[NV];
  auto stage_load = [&](int tile) __attribute__((always_inline)) {
#pragma unroll
    for (int v = 0; v < NV; ++v) pre[v] = Wf[(int64_t)tile * TILE + tid + v * NTH];
  };
  auto stage_store = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int v = 0; v < NV; ++v) as[buf][tid + v * NTH] = pre[v];
  };
  auto tile_after = [&](int tt, int k) { return (tt + k) % ntiles; };
  stage_load(t);
  stage_store(0);
  if (u0 + 1 < u1) stage_load(tile_after(t, 1));
  __syncthreads();

  u32x4 bh[KS], bm[F16 ? 1 : KS], bl[KS];
  float row_scale = 1.f;  // F16: inverse of the power of two this lane's row was multiplied by
  auto hidden = [&](const float (&e)[kMaxNb], bool row_ok, int64_t hblk) __attribute__((always_inline)) {
    float hv[F16 ? (H / 32) * 16 : 1];
    float w0v[XIN ? 1 : H / 32][kMaxNb / 2];  // all requests first: one L2 latency per block, not sixteen
    float4 pin[XIN ? H / 32 : 1][4];
    if constexpr (XIN) {
      // register r of the 32 x 32 accumulator layout <-> hidden channel 32 kb + (r & 3) + 8 (r >> 2) + 4 half of edge row l31
      const int64_t row = hblk * kMlpRows + wv * 32 + l31;
      const float* __restrict__ pr = emb + (row < E ? row : (E - 1)) * H + 4 * half;
#pragma unroll
      for (int kb = 0; kb < H / 32; ++kb)
#pragma unroll
        for (int g = 0; g < 4; ++g) pin[kb][g] = *reinterpret_cast<const float4*>(pr + kb * 32 + 8 * g);
    } else {
#pragma unroll
      for (int kb = 0; kb < H / 32; ++kb)
#pragma unroll
        for (int s2 = 0; s2 < kMaxNb / 2; ++s2) {
          const int c = 2 * s2 + half;
          w0v[kb][s2] = W0[(c < nb ? c : 0) * H + kb * 32 + l31];
        }
    }
#pragma unroll
    for (int kb = 0; kb < H / 32; ++kb) {
      f32x16 hacc = {0};
      if constexpr (XIN) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          hacc[4 * g] = pin[kb][g].x; hacc[4 * g + 1] = pin[kb][g].y; hacc[4 * g + 2] = pin[kb][g].z; hacc[4 * g + 3] = pin[kb][g].w;
        }
      } else {
#pragma unroll
        for (int s2 = 0; s2 < kMaxNb / 2; ++s2) {
          const float av = (2 * s2 + half) < nb ? w0v[kb][s2] * a0 : 0.f;
          const float bv = half ? e[2 * s2 + 1] : e[2 * s2];
          hacc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, hacc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const float h0 = row_ok ? (XIN ? silu_given_f(hacc[r]) : silu_f(hacc[r])) : 0.f;
        const float h1 = row_ok ? (XIN ? silu_given_f(hacc[r + 1]) : silu_f(hacc[r + 1])) : 0.f;
        if constexpr (F16) {
          hv[kb * 16 + r] = h0;
          hv[kb * 16 + r + 1] = h1;
        } else {
          uint32_t a, b, c;
          split_pair(h0, h1, a, b, c);
          const int s = 2 * kb + (r >> 3), tp = (r & 7) >> 1;
          bh[s][tp] = a; bm[s][tp] = b; bl[s][tp] = c;
        }
      }
    }
    if constexpr (F16) {
      // the row's H values sit in this lane and in lane ^ 32
      float m = 0.f;
#pragma unroll
      for (int i = 0; i < (H / 32) * 16; ++i) m = fmaxf(m, fabsf(hv[i]));
      m = fmaxf(m, __shfl_xor(m, 32));
      const float su = f16_scale_up(m);
      row_scale = 1.f / su;
#pragma unroll
      for (int kb = 0; kb < H / 32; ++kb) {
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          uint32_t a, b;
          split_pair_f16(hv[kb * 16 + r] * su, hv[kb * 16 + r + 1] * su, a, b);
          const int s = 2 * kb + (r >> 3), tp = (r & 7) >> 1;
          bh[s][tp] = a; bl[s][tp] = b;
        }
      }
    }
  };
  hidden(ev, blk * kMlpRows + wv * 32 + l31 < E, blk);

  float* __restrict__ tb = tbuf + wv * (32 * kTS);
  // bf16: pa + pb (large + small partial products).  F16: (pa + pb) * rs * tile_scale with rs the row scale of the unit
  // the accumulators belong to.
  auto emit = [&](const f32x16& pa, const f32x16& pb, int tile, int64_t wrow0, float rs) __attribute__((always_inline)) {
    if constexpr (F16) {
      const float f = rs * tile_scale[tile];
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(tb + l31 * kTS + 8 * g + 4 * half) =
            make_float4((pa[4 * g] + pb[4 * g]) * f, (pa[4 * g + 1] + pb[4 * g + 1]) * f,
                        (pa[4 * g + 2] + pb[4 * g + 2]) * f, (pa[4 * g + 3] + pb[4 * g + 3]) * f);
    } else {
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(tb + l31 * kTS + 8 * g + 4 * half) =
            make_float4(pa[4 * g] + pb[4 * g], pa[4 * g + 1] + pb[4 * g + 1], pa[4 * g + 2] + pb[4 * g + 2],
                        pa[4 * g + 3] + pb[4 * g + 3]);
    }
    const int n0 = tile * 32;
    const int c4 = lane & 7, rsub = lane >> 3;
    if (wrow0 + 32 <= E && n0 + 32 <= W) {
      float* __restrict__ ob = out + (wrow0 + rsub) * W + n0 + 4 * c4;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        mlp_store4(ob + (int64_t)(8 * i) * W, *reinterpret_cast<const float4*>(tb + (8 * i + rsub) * kTS + 4 * c4));
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 8 * i + rsub;
        const float4 v = *reinterpret_cast<const float4*>(tb + r * kTS + 4 * c4);
        if (wrow0 + r < E && n0 + 4 * c4 + 3 < W) *reinterpret_cast<float4*>(out + (wrow0 + r) * W + n0 + 4 * c4) = v;
      }
    }
  };
  // one work unit; `i` = index of the unit in this workgroup's range (selects the LDS weight buffer)
  int prev_tile = 0;
  int64_t prev_row0 = 0;
  float prev_rs = 1.f;
  auto unit = [&](int64_t i, f32x16& accA, f32x16& accB, const f32x16& prevA, const f32x16& prevB)
      __attribute__((always_inline)) {
    const int64_t left = (u1 - u0) - i;  // units left including this one
    if (t == 0 && i > 0) {  // entering the next block: its embedding row was requested during the previous tile
      ++blk;
#pragma unroll
      for (int c = 0; c < kMaxNb; ++c) ev[c] = evn[c];
      hidden(ev, blk * kMlpRows + wv * 32 + l31 < E, blk);
    }
    const int buf = (int)(i & 1);
    if (left > 1) stage_store(buf ^ 1);
    if (left > 2) stage_load(tile_after(t, 2));
    if (t == ntiles - 1 && left > 1) load_ev(blk + 1, evn);
    const u32x4* __restrict__ a = as[buf] + lane;
    accA = (f32x16){0};
    accB = (f32x16){0};
    u32x4 fa[2][NPL];
#pragma unroll
    for (int q = 0; q < NPL; ++q) fa[0][q] = a[q * 64];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      if (s + 1 < KS) {
#pragma unroll
        for (int q = 0; q < NPL; ++q) fa[(s + 1) & 1][q] = a[((s + 1) * NPL + q) * 64];
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (F16) {
        const u32x4 &ah = fa[s & 1][0], &al = fa[s & 1][1];
        // the three products rotate over the two accumulators so that no instruction waits for its predecessor
        // (one accumulator = one dependent chain was measured: 168 registers, three workgroups per CU, 4 % slower)
        if (s & 1) {
          accB = mfma_f16(ah, bl[s], accB);
          accA = mfma_f16(al, bh[s], accA);
          accB = mfma_f16(ah, bh[s], accB);
        } else {
          accA = mfma_f16(ah, bl[s], accA);
          accB = mfma_f16(al, bh[s], accB);
          accA = mfma_f16(ah, bh[s], accA);
        }
      } else {
        const u32x4 &ah = fa[s & 1][0], &am = fa[s & 1][1], &al = fa[s & 1][2];
        accA = mfma_bf16(ah, bh[s], accA);
        accB = mfma_bf16(am, bm[s], accB);
        accA = mfma_bf16(ah, bm[s], accA);
        accB = mfma_bf16(ah, bl[s], accB);
        accA = mfma_bf16(am, bh[s], accA);
        accB = mfma_bf16(al, bh[s], accB);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (s == 1 && i > 0) {
        emit(prevA, prevB, prev_tile, prev_row0, prev_rs);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    lds_barrier();
    prev_tile = t;
    prev_row0 = blk * kMlpRows + wv * 32;
    prev_rs = row_scale;
    if (++t == ntiles) t = 0;
  };
  f32x16 a0A, a0B, a1A, a1B;
  const int64_t n = u1 - u0;
  for (int64_t i = 0; i < n; i += 2) {
    unit(i, a0A, a0B, a1A, a1B);
    if (i + 1 < n) unit(i + 1, a1A, a1B, a0A, a0B);
  }
  if (n & 1)
    emit(a0A, a0B, prev_tile, prev_row0, prev_rs);
  else
    emit(a1A, a1B, prev_tile, prev_row0, prev_rs);
}

}  // namespace nqa
#include "radial_mlp_pipe.h"
namespace nqa {

// TM (training mode, see nqa_radial_mlp_bwd_train): 0 = inference (g_emb only); 1 = additionally hid_out = silu(P)
// and the per-workgroup partial of dW0 = emb^T (G_h silu'(P)); 2 = second order with a cotangent row block cemb:
// Q = cemb W0, hid_out = Q silu'(P), g_emb = (Q G_h silu''(P)) W0^T, dW0 partial = emb^T (Q G_h silu'') + cemb^T (G_h silu').
// Everything happens in the epilogue on the tile that is already on chip; the main loop is the same code.
// PAIR (nqa_radial_mlp_bwd_paired): the incoming gradient is the sum of two row streams gw[row] + gw2[row] (the two
// directed edges of a pair wrote their halves separately), added in registers when a chunk is consumed.
// F16: the two-plane fp16 split with a RUNNING per-row scale (main loop only: the training epilogues work on the
// accumulators after they have been brought back to the true scale).  The gradient rows stream in
// with no scale known in advance, so every row carries an exponent S: its accumulators hold 2^S x the true sums, a chunk
// is multiplied by 2^(S - chunk_exp[chunk]) (the weights of the chunk were multiplied by 2^chunk_exp[chunk]) before it
// is split, and S is lowered -- the row's accumulators are multiplied by the power of two that bridges the old and the
// new scale -- whenever a chunk's largest magnitude would leave fp16's range.  S is set three bits below the limit, so
// later chunks up to 8x larger pass without a rescale.  Both factors are powers of two: exact.  The error of a product
// is 2^-22 of the row's (running) maximum x the chunk's weight maximum, the rounding level of the fp32 sum itself.
// XIN (nqa_radial_mlp_last_bwd, TM = 0): the last layer of a deeper MLP -- `emb` holds the pre-activations P [E, H] of the
// layer's input, the result is grad_P = (g W^T) silu'(P) written to `g_emb` as [E, H]; no first-layer GEMV.
// (`dbg`: always 0, as for radial_mlp_fwd_kernel)
template <int H, int TM, bool PAIR = false, bool F16 = false, bool XIN = false>
__global__ __launch_bounds__(256, 2) void radial_mlp_bwd_split_kernel(const float* __restrict__ emb,
                                                                    const float* __restrict__ W0,
                                                                    const u32x4* __restrict__ Wb,
                                                                    const float* __restrict__ gw, float a0, int nb,
                                                                    int W, int64_t E, float* __restrict__ g_emb,
                                                                    int dbg, const float* __restrict__ cemb,
                                                                    float* __restrict__ hid_out,
                                                                    float* __restrict__ w0_part,
                                                                    const float* __restrict__ gw2 = nullptr,
                                                                    const int* __restrict__ chunk_exp = nullptr) {
  // K (= W) is consumed in chunks of 32 columns = two bf16 k-steps; lane (row, half) owns the 16 contiguous floats
  // 32*chunk + 16*half + [0, 16) of its g_w row per chunk: HBM -> registers directly, split in registers.
  constexpr int NT = H / 32;
  constexpr int NPL = F16 ? 2 : 3;        // operand planes
  constexpr int CH = 2 * NPL * NT * 64;   // uint4 per chunk of B fragments (24 KiB for H = 128; 16 KiB in F16 mode)
  constexpr int NV = CH / 256;
  constexpr int GS = H + 1;
  constexpr int kMainBytes = 2 * CH * 16;
  constexpr int kEpiBytes = kMlpRows * GS * 4;
  constexpr int kBufBytes = kMainBytes > kEpiBytes ? kMainBytes : kEpiBytes;
  __shared__ __align__(16) unsigned char smem_raw[kBufBytes];
  __shared__ float w0s[H * kMaxNb];        // [k][c]
  __shared__ float w0t[kMaxNb * H];        // [c][k]
  __shared__ float es[kMlpRows * kMaxNb];  // embedding tile [row][c]
  __shared__ int rowexp[F16 ? kMlpRows : 1];  // F16: per-row exponents on their way from the row's lane to its registers
  // cotangent tile [row][c] of the second-order mode: only needed after the GEMV pass, so for H = 128 (where LDS caps
  // the occupancy) it reuses w0s' storage; each lane keeps its own cotangent row in registers until then
  __shared__ float cs_own[(TM == 2 && H * kMaxNb < kMlpRows * kMaxNb) ? kMlpRows * kMaxNb : 1];
  float* __restrict__ cs = (H * kMaxNb >= kMlpRows * kMaxNb) ? w0s : cs_own;
  u32x4* __restrict__ bsm = reinterpret_cast<u32x4*>(smem_raw);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int half = lane >> 5;
  const int l31 = lane & 31;
  const int64_t blk0 = (int64_t)blockIdx.x * kMlpRows;
  const int64_t myrow = blk0 + wv * 32 + l31;
  const bool row_ok = myrow < E;

  if constexpr (!XIN) {
    for (int i = tid; i < H * kMaxNb; i += 256) {
      const int k = i / kMaxNb, c = i - k * kMaxNb;
      const float v = c < nb ? W0[c * H + k] * a0 : 0.f;
      w0s[i] = v;
      w0t[c * H + k] = v;
    }
    for (int i = tid; i < kMlpRows * kMaxNb; i += 256) {
      const int r = i / kMaxNb, c = i - r * kMaxNb;
      const int64_t rr = blk0 + r < E ? blk0 + r : E - 1;  // clamped, unpredicated load; masked below
      const float v = emb[rr * nb + (c < nb ? c : nb - 1)];
      es[i] = (c < nb && blk0 + r < E) ? v : 0.f;
    }
  }
  float cvr[kMaxNb];
  if (TM == 2) {
    const float* __restrict__ cr = cemb + (row_ok ? myrow : (E - 1)) * nb;
#pragma unroll
    for (int c = 0; c < kMaxNb; ++c) cvr[c] = cr[c < nb ? c : nb - 1];
#pragma unroll
    for (int c = 0; c < kMaxNb; ++c) cvr[c] = (row_ok && c < nb) ? cvr[c] : 0.f;
  }

  const int nchunks = (W + 31) / 32;
  u32x4 pb[NV];
  const float* __restrict__ grow = gw + (row_ok ? myrow : 0) * W + 16 * half;
  const float* __restrict__ grow2 = PAIR ? gw2 + (row_ok ? myrow : 0) * W + 16 * half : nullptr;
  const bool rows_full = blk0 + kMlpRows <= E;  // workgroup-uniform
  auto load_rows = [&](const float* __restrict__ gr, int ch, float4 (&pa)[4]) {
    if (rows_full && 32 * ch + 32 <= W) {  // uniform common case: unpredicated loads
#pragma unroll
      for (int v = 0; v < 4; ++v) pa[v] = *reinterpret_cast<const float4*>(gr + 32 * ch + 4 * v);
    } else {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int k = 32 * ch + 16 * half + 4 * v;
        pa[v] = (row_ok && k + 3 < W) ? *reinterpret_cast<const float4*>(gr + 32 * ch + 4 * v)
                                      : make_float4(0.f, 0.f, 0.f, 0.f);  // W % 4 == 0
      }
    }
  };
  auto load_a = [&](int ch, float4 (&pa)[4], float4 (&pc)[4]) {
    if (dbg & 1) return;  // ablation: no g_w traffic
    load_rows(grow, ch, pa);
    if (PAIR) load_rows(grow2, ch, pc);
  };
  auto load_b = [&](int ch) {
#pragma unroll
    for (int v = 0; v < NV; ++v) pb[v] = Wb[(int64_t)ch * CH + tid + v * 256];
  };
  auto store_b = [&](int buf) {
#pragma unroll
    for (int v = 0; v < NV; ++v) bsm[buf * CH + tid + v * 256] = pb[v];
  };
  // g_w (HBM) is fetched two chunks ahead into alternating register sets, the weight fragments (L2) one chunk ahead
  // and *before* the g_w request of the same iteration: vmcnt retires in order, so the wait for the fragments then
  // leaves the younger HBM loads in flight.
  float4 paA[4], paB[4];
  float4 pcA[PAIR ? 4 : 1], pcB[PAIR ? 4 : 1];  // second row stream (PAIR)
  load_b(0);
  load_a(0, paA, reinterpret_cast<float4(&)[4]>(pcA));
  store_b(0);
  if (nchunks > 1) load_a(1, paB, reinterpret_cast<float4(&)[4]>(pcB));
  __syncthreads();

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (f32x16){0};
  constexpr int kUnset = 1 << 20;
  int S = kUnset;                              // F16: exponent of this lane's row (unset while the row is all zero)
  int we_next = F16 ? chunk_exp[0] : 0;        // F16: weight exponent of the chunk about to be consumed
  // rows (r, half) of the accumulator registers <- values held by the rows' own lanes (same wavefront: LDS in order)
  auto rows_from_lanes = [&](int value, int (&out)[16]) __attribute__((always_inline)) {
    int* __restrict__ rb = rowexp + wv * 32;
    if (half == 0) rb[l31] = value;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int r = 0; r < 16; ++r) out[r] = rb[(r & 3) + 8 * (r >> 2) + 4 * half];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };

  auto body = [&](int ch, float4 (&pa)[4], float4 (&pc)[4]) {
    const int buf = ch & 1;
    if (PAIR) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        pa[v].x += pc[v].x; pa[v].y += pc[v].y; pa[v].z += pc[v].z; pa[v].w += pc[v].w;
      }
    }
    // split this chunk's 16 floats into the A fragments of its two k-steps
    u32x4 ah[2], am[F16 ? 1 : 2], al[2];
    if constexpr (F16) {
      const int we = we_next;
      if (ch + 1 < nchunks) we_next = chunk_exp[ch + 1];
      float m = 0.f;  // the row's largest magnitude in this chunk (its other 16 values sit in lane ^ 32)
#pragma unroll
      for (int v = 0; v < 4; ++v)
        m = fmaxf(m, fmaxf(fmaxf(fabsf(pa[v].x), fabsf(pa[v].y)), fmaxf(fabsf(pa[v].z), fabsf(pa[v].w))));
      m = fmaxf(m, __shfl_xor(m, 32));
      int shift = 0;
      if (m > 0.f && m < 3.0e38f) {
        int em;
        (void)frexpf(m, &em);          // m < 2^em
        const int cap = 15 - em + we;  // largest S that keeps m 2^(S - we) below 2^15
        if (cap < S) {
          int ns = cap - 3;
          ns = ns > we + 100 ? we + 100 : (ns < we - 100 ? we - 100 : ns);
          shift = S == kUnset ? 0 : S - ns;
          S = ns;
        }
      }
      if (ch > 0 && __any(shift > 0)) {  // (rare after the first chunks: a new maximum 8x above every earlier one)
        int kr[16];
        rows_from_lanes(shift, kr);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[t][r] = ldexpf(acc[t][r], -kr[r]);
      }
      int q = S == kUnset ? 0 : S - we;
      q = q > 120 ? 120 : (q < -120 ? -120 : q);
      const float qs = ldexpf(1.f, q);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        uint32_t a, b;
        split_pair_f16(pa[2 * s].x * qs, pa[2 * s].y * qs, a, b);
        ah[s][0] = a; al[s][0] = b;
        split_pair_f16(pa[2 * s].z * qs, pa[2 * s].w * qs, a, b);
        ah[s][1] = a; al[s][1] = b;
        split_pair_f16(pa[2 * s + 1].x * qs, pa[2 * s + 1].y * qs, a, b);
        ah[s][2] = a; al[s][2] = b;
        split_pair_f16(pa[2 * s + 1].z * qs, pa[2 * s + 1].w * qs, a, b);
        ah[s][3] = a; al[s][3] = b;
      }
    } else
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      uint32_t a, b, c;
      split_pair(pa[2 * s].x, pa[2 * s].y, a, b, c);
      ah[s][0] = a; am[s][0] = b; al[s][0] = c;
      split_pair(pa[2 * s].z, pa[2 * s].w, a, b, c);
      ah[s][1] = a; am[s][1] = b; al[s][1] = c;
      split_pair(pa[2 * s + 1].x, pa[2 * s + 1].y, a, b, c);
      ah[s][2] = a; am[s][2] = b; al[s][2] = c;
      split_pair(pa[2 * s + 1].z, pa[2 * s + 1].w, a, b, c);
      ah[s][3] = a; am[s][3] = b; al[s][3] = c;
    }
    if (ch + 1 < nchunks && !(dbg & 2) && !((dbg & 8) && (ch & 1))) load_b(ch + 1);
    if (ch + 2 < nchunks) load_a(ch + 2, pa, pc);
    const u32x4* __restrict__ bs = bsm + buf * CH + lane;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      u32x4 fb[NPL][NT];
      if constexpr (F16) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int t = 0; t < NT; ++t) fb[q][t] = bs[((s * 2 + q) * NT + t) * 64];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = mfma_f16(al[s], fb[0][t], acc[t]);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = mfma_f16(ah[s], fb[1][t], acc[t]);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = mfma_f16(ah[s], fb[0][t], acc[t]);
        __builtin_amdgcn_sched_barrier(0);
        continue;
      }
      if (!(dbg & 16) || ch == 0) {  // (ablation bit 16: weight fragments read from LDS for the first chunk only)
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
          for (int t = 0; t < NT; ++t) fb[q][t] = bs[((s * 3 + q) * NT + t) * 64];
      } else {
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
          for (int t = 0; t < NT; ++t) fb[q][t] = (u32x4){0x3f803f80u + (unsigned)lane, 0x3c003c00u, 0x38003800u + (unsigned)t, 0x3f803f80u + (unsigned)q};
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = mfma_bf16(am[s], fb[1][t], acc[t]);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = mfma_bf16(ah[s], fb[2][t], acc[t]);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = mfma_bf16(al[s], fb[0][t], acc[t]);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = mfma_bf16(ah[s], fb[1][t], acc[t]);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = mfma_bf16(am[s], fb[0][t], acc[t]);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = mfma_bf16(ah[s], fb[0][t], acc[t]);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (ch + 1 < nchunks && !(dbg & 2) && !((dbg & 8) && (ch & 1))) store_b(buf ^ 1);
    if (!(dbg & 4)) lds_barrier();
  };
  for (int ch = 0; ch < nchunks; ch += 2) {
    body(ch, paA, reinterpret_cast<float4(&)[4]>(pcA));
    if (ch + 1 < nchunks) body(ch + 1, paB, reinterpret_cast<float4(&)[4]>(pcB));
  }

  if constexpr (F16) {  // accumulators back to the true scale: 2^-S of their row
    int sr[16];
    rows_from_lanes(S == kUnset ? 0 : S, sr);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = ldexpf(acc[t][r], -sr[r]);
  }
  if constexpr (XIN) {
    // grad_P[row][col] = G_h[row][col] silu'(P[row][col]) straight from the accumulator layout: register r of tile t is
    // (row = 32 wv + (r & 3) + 8 (r >> 2) + 4 half, col = 32 t + l31) -- 128-byte runs per (row, half)
    static_assert(!XIN || TM == 0, "XIN is an inference backward");
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = t * 32 + l31;
      float pv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t row = blk0 + wv * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        pv[r] = emb[(row < E ? row : (E - 1)) * H + col];
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t row = blk0 + wv * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (row < E) g_emb[row * H + col] = acc[t][r] * silu_grad_given_f(pv[r]);
      }
    }
    return;
  }
  // epilogue (exact fp32): pre-activations recomputed on MFMA in the accumulator layout, g_pre = g_h * silu'(pre),
  // one pass through LDS for the NB-wide GEMV -- identical to the fp32 kernel
  float* __restrict__ gp = reinterpret_cast<float*>(smem_raw);
  {
    const float* __restrict__ erow = es + (wv * 32 + l31) * kMaxNb;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x16 pacc = {0};
#pragma unroll
      for (int s2 = 0; s2 < kMaxNb / 2; ++s2) {
        const float av = erow[2 * s2 + half];
        const float bv = w0t[(2 * s2 + half) * H + t * 32 + l31];
        pacc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, pacc, 0, 0, 0);
      }
      f32x16 qacc = {0};
      if (TM == 2) {
#pragma unroll
        for (int s2 = 0; s2 < kMaxNb / 2; ++s2) {
          const float av = half ? cvr[2 * s2 + 1] : cvr[2 * s2];
          const float bv = w0t[(2 * s2 + half) * H + t * 32 + l31];
          qacc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, qacc, 0, 0, 0);
        }
      }
      const int col = t * 32 + l31;
      if (TM == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int lr = wv * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          gp[lr * GS + col] = acc[t][r] * silu_grad_f(pacc[r]);
        }
      } else {
        float hv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int lr = wv * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          float h, d1, d2;
          silu_all_f(pacc[r], h, d1, d2);
          if (TM == 1) {
            gp[lr * GS + col] = acc[t][r] * d1;
            hv[r] = h;
          } else {
            gp[lr * GS + col] = qacc[r] * acc[t][r] * d2;
            hv[r] = qacc[r] * d1;
            acc[t][r] *= d1;  // G_h silu'(P): second partial pass below
          }
        }
        // hidden-side output rows (silu(P) / Q silu'(P)), 128-byte runs per (row, half)
        float* __restrict__ hrow = hid_out + (blk0 + wv * 32 + 4 * half) * (int64_t)H + col;
        if (rows_full) {
#pragma unroll
          for (int r = 0; r < 16; ++r) hrow[(int64_t)((r & 3) + 8 * (r >> 2)) * H] = hv[r];
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int lr = wv * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (blk0 + lr < E) hrow[(int64_t)((r & 3) + 8 * (r >> 2)) * H] = hv[r];
          }
        }
      }
    }
  }
  __syncthreads();
  {
    const int r = tid >> 1, kh = tid & 1;
    float sacc[kMaxNb];
#pragma unroll
    for (int c = 0; c < kMaxNb; ++c) sacc[c] = 0.f;
    const float* __restrict__ gr = gp + r * GS + kh * (H / 2);
    const float* __restrict__ wr = w0s + kh * (H / 2) * kMaxNb;
#pragma unroll 4
    for (int k = 0; k < H / 2; ++k) {
      const float gv = gr[k];
      const float4 w0 = *reinterpret_cast<const float4*>(wr + k * kMaxNb);
      const float4 w1 = *reinterpret_cast<const float4*>(wr + k * kMaxNb + 4);
      sacc[0] += gv * w0.x; sacc[1] += gv * w0.y; sacc[2] += gv * w0.z; sacc[3] += gv * w0.w;
      sacc[4] += gv * w1.x; sacc[5] += gv * w1.y; sacc[6] += gv * w1.z; sacc[7] += gv * w1.w;
    }
#pragma unroll
    for (int c = 0; c < kMaxNb; ++c) sacc[c] += __shfl_xor(sacc[c], 1, 64);
    if (kh == 0 && blk0 + r < E) {
      for (int c = 0; c < nb; ++c) g_emb[(blk0 + r) * nb + c] = sacc[c];
    }
  }
  if (TM != 0) {
    // this workgroup's partial of dW0[c][k] = sum_rows emb[row][c] * tile[row][k]  (rows past E have emb = 0);
    // thread = (k, group of CPT basis functions)
    constexpr int NCG = 256 / H, CPT = kMaxNb / NCG;
    const int k = tid % H, cg = tid / H;
    float part[CPT];
#pragma unroll
    for (int i = 0; i < CPT; ++i) part[i] = 0.f;
    for (int r = 0; r < kMlpRows; ++r) {
      const float gv = gp[r * GS + k];
#pragma unroll
      for (int i = 0; i < CPT; ++i) part[i] += es[r * kMaxNb + cg * CPT + i] * gv;
    }
    if (TM == 2) {
      __syncthreads();  // every reader of the cotangent-side tile (and of w0s, reused for the cotangent rows) is done
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          gp[(wv * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * GS + t * 32 + l31] = acc[t][r];
      if (half == 0) {
#pragma unroll
        for (int c = 0; c < kMaxNb; ++c) cs[(wv * 32 + l31) * kMaxNb + c] = cvr[c];
      }
      __syncthreads();
      for (int r = 0; r < kMlpRows; ++r) {
        const float gv = gp[r * GS + k];
#pragma unroll
        for (int i = 0; i < CPT; ++i) part[i] += cs[r * kMaxNb + cg * CPT + i] * gv;
      }
    }
    float* __restrict__ wp = w0_part + (int64_t)blockIdx.x * nb * H;
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int c = cg * CPT + i;
      if (c < nb) wp[c * H + k] = part[i];
    }
  }
}

}  // namespace nqa

using namespace nqa;

// ---- host side ---------------------------------------------------------------------------------------------------------
namespace {

// Switches (env_flag / env_int of plan.h).  Every one is read at every call, because the tests select kernel forms
// within one process; only the CU count is looked up once.
int mlp_num_cus() {
  static const int num_cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    return n;
  }();
  return num_cus;
}

// Workspace of one (mode, direction, H, W): the weight fragments (fp32 backward: the transposed weights) and, for the
// fp16 split, a second field behind them -- forward: one float per 32-column tile (the inverse of the tile's
// power-of-two scale), backward: one int per 32-column chunk (the exponent the chunk was scaled by).
//   F16X3 forward : ceil(W/32) tiles x (H/16) k-steps x 2 planes x 1 KiB     F16X3 backward: ceil(W/32) chunks x 2 k-steps
//   BF16X6        : ceil(W/32) tiles x (H/16) k-steps x 3 planes x 1 KiB                     x 2 planes x (H/32) x 1 KiB
//   FP32 backward : [W (+ 4 x 64 padding rows read by the last chunk)][H] floats; the FP32 forward needs none.
struct MlpLayout {
  int64_t total;   // bytes; -1: no such form
  int64_t second;  // byte offset of the second field; -1: none
};
MlpLayout mlp_layout(int32_t mode, int32_t backward, int32_t H, int32_t W) {
  if (H <= 0 || W <= 0) return {-1, -1};
  const int64_t n32 = (W + 31) / 32;
  if (mode == NQA_MLP_F16X3) {
    const int64_t frag = backward ? n32 * 2 * 2 * (H / 32) * 1024 : n32 * (H / 16) * 2 * 1024;
    return {frag + ((n32 * 4 + 255) & ~(int64_t)255), frag};
  }
  if (mode == NQA_MLP_BF16X6) return {n32 * (H / 16) * 3 * 1024, -1};
  if (mode != NQA_MLP_FP32) return {-1, -1};
  if (!backward) return {0, -1};
  return {(int64_t)H * W * (int64_t)sizeof(float) + 4 * 64 * H * (int64_t)sizeof(float), -1};
}
struct MlpWorkspace {
  u32x4* fragments;
  void* second;
  template <class T>
  T* second_as() const { return static_cast<T*>(second); }
};
MlpWorkspace mlp_view(void* workspace, const MlpLayout& lay) {
  return {static_cast<u32x4*>(workspace),
          lay.second < 0 ? nullptr : reinterpret_cast<void*>(static_cast<char*>(workspace) + lay.second)};
}

int fail(int rc, const std::string& text) {
  set_error(text);
  return rc;
}

// Operands of the two drivers.  `fn` names the entry point in the error texts.  `xin`: `in` holds the pre-activations
// [E, H] of the last layer of a deeper MLP (no first layer: w0 null, alpha0 = 1, nb = 0; fp16 split only).
struct MlpCall {
  const char* fn;
  int32_t dtype, mode;
  bool xin;
  const void *in, *w0;
  double alpha0;
  const void* w1;
  double alpha1;
  int32_t nb, H, W;
  int64_t E;
  void* workspace;
  int64_t workspace_bytes;
  int32_t workspace_ready;
  nqa_stream stream;
};

// Checks shared by both directions; `io_ok`: the direction's own pointers are there.  NQA_OK with E == 0 is the
// caller's early return.
int mlp_check(const MlpCall& c, bool io_ok) {
  const std::string fn(c.fn);
  const bool h_ok = c.H == 64 || c.H == 128;
  if (c.xin) {
    if (c.dtype != NQA_F32 || c.mode != NQA_MLP_F16X3)
      return fail(NQA_ERR_UNSUPPORTED, fn + ": float32 on the two-plane fp16 split (NQA_MLP_F16X3) only");
    if (c.E < 0 || !h_ok || c.W <= 0 || c.W % 4 != 0 || (c.E > 0 && (!c.in || !c.w1 || !io_ok)))
      return fail(h_ok ? NQA_ERR_INVALID : NQA_ERR_UNSUPPORTED,
                  fn + ": invalid argument (hidden 64 / 128, out_features % 4 == 0)");
    return NQA_OK;
  }
  if (c.dtype != NQA_F32) return fail(NQA_ERR_UNSUPPORTED, fn + ": only float32 is implemented on MFMA");
  if (c.mode != NQA_MLP_FP32 && c.mode != NQA_MLP_BF16X6 && c.mode != NQA_MLP_F16X3)
    return fail(NQA_ERR_INVALID, fn + ": unknown mode");
  if (c.E < 0 || c.nb <= 0 || c.nb > kMaxNb || c.W <= 0 || (c.E > 0 && (!c.in || !c.w0 || !c.w1)))
    return fail(NQA_ERR_INVALID, fn + ": invalid argument");
  if (!h_ok) return fail(NQA_ERR_UNSUPPORTED, fn + ": hidden width must be 64 or 128 for the fused MFMA kernel");
  return NQA_OK;
}

// The template dispatch, once per kernel family: f(H) and f(H, TM, PAIR) with the values as integral constants.
template <int V>
using ic = std::integral_constant<int, V>;
template <class F>
void by_h(int H, F&& f) {
  if (H == 128) f(ic<128>{});
  else f(ic<64>{});
}
template <class F>
void by_h_tm_pair(int H, int tm, bool pair, F&& f) {  // (a second gradient stream goes with tm == 0 only)
  by_h(H, [&](auto h) {
    if (pair) f(h, ic<0>{}, std::true_type{});
    else if (tm == 0) f(h, ic<0>{}, std::false_type{});
    else if (tm == 1) f(h, ic<1>{}, std::false_type{});
    else f(h, ic<2>{}, std::false_type{});
  });
}

// forward; `cotangent`: the tangent of the output along it instead (NQA_MLP_BF16X6)
int mlp_fwd(const MlpCall& c, const void* cotangent, void* out) {
  const std::string fn(c.fn);
  int rc = mlp_check(c, out != nullptr);
  if (rc != NQA_OK || c.E == 0) return rc;
  if (out == nullptr || c.W % 4 != 0) return fail(NQA_ERR_INVALID, fn + ": invalid output (needs out_features % 4 == 0)");
  const MlpLayout lay = mlp_layout(c.mode, 0, c.H, c.W);
  if (lay.total > 0 && (c.workspace == nullptr || c.workspace_bytes < lay.total))
    return fail(NQA_ERR_WORKSPACE, fn + ": workspace missing or too small");
  if (cotangent != nullptr && c.mode != NQA_MLP_BF16X6)
    return fail(NQA_ERR_UNSUPPORTED,
                c.mode == NQA_MLP_F16X3
                    ? "nqa_radial_mlp_fwd_tangent: NQA_MLP_F16X3 is a mode of the plain forward (use NQA_MLP_BF16X6)"
                    : "nqa_radial_mlp_fwd_tangent: only NQA_MLP_BF16X6 is implemented");
  const MlpWorkspace ws = mlp_view(c.workspace, lay);
  hipStream_t s = static_cast<hipStream_t>(c.stream);
  const int nb = c.nb, H = c.H, W = c.W;
  const int64_t E = c.E;
  const float a0 = (float)c.alpha0, a1 = (float)c.alpha1;
  const float* e = static_cast<const float*>(c.in);
  const float* a = static_cast<const float*>(c.w0);
  const float* b = static_cast<const float*>(c.w1);
  float* o = static_cast<float*>(out);
  u32x4* wf = ws.fragments;
  const int ntiles = (W + 31) / 32;
  const unsigned grid = (unsigned)((E + kMlpRows - 1) / kMlpRows);
  // balanced work-unit ranges (128-row block x 32-column tile) over a fixed grid of two workgroups per CU
  const auto balanced_grid = [&] {
    const int64_t units = (int64_t)grid * ntiles, slots = 2 * (int64_t)mlp_num_cus();
    return (unsigned)(units < slots ? units : slots);
  };
  if (c.mode == NQA_MLP_F16X3) {
    float* ts = ws.second_as<float>();
    if (!c.workspace_ready)
      hipLaunchKernelGGL(radial_mlp_split_w1_fwd_f16_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, b, a1, H, W, wf, ts);
    const unsigned gb = balanced_grid();
    // round 5: outputs of complete 32-column tiles run on the issue-scheduled kernel (radial_mlp_pipe.h; NQA_MLP_PIPE=0:
    // the general kernel)
    // (H = 64 stays on the general kernel: its 166 registers keep three wavefronts per SIMD, the scheduled form needs 170)
    if (!c.xin && env_flag("NQA_MLP_PIPE", true) && H == 128 && W % 32 == 0 && ntiles <= 128) {
      // tile epilogue: through the wave-private LDS transpose (default: 128-133 us for the cfg-3 middle layer, 48 us for the
      // first / last one) or straight from the accumulators with the MFMA operands swapped (NQA_MLP_PIPE_DIRECT=1: 134-161
      // / 50 us at 244 registers) -- profiles/r5_mlp_fwd_kernel_trace.txt; the round-4 kernel: 149-161 / 60 us
      if (env_flag("NQA_MLP_PIPE_DIRECT", false))
        hipLaunchKernelGGL((radial_mlp_fwd_pipe_kernel<128, true>), dim3(gb), dim3(256), 0, s, e, a, wf, a0, nb, W, E, o, ts);
      else
        hipLaunchKernelGGL((radial_mlp_fwd_pipe_kernel<128, false>), dim3(gb), dim3(256), 0, s, e, a, wf, a0, nb, W, E, o, ts);
      return launch_status(c.fn);
    }
    by_h(H, [&](auto h) {
      constexpr int HH = decltype(h)::value;
      if (c.xin)
        hipLaunchKernelGGL((radial_mlp_fwd_split_bal_kernel<HH, true, true>), dim3(gb), dim3(256), 0, s, e, a, wf, a0, nb,
                           W, E, o, ts);
      else
        hipLaunchKernelGGL((radial_mlp_fwd_split_bal_kernel<HH, true>), dim3(gb), dim3(256), 0, s, e, a, wf, a0, nb, W, E,
                           o, ts);
    });
    return launch_status(c.fn);
  }
  if (c.mode == NQA_MLP_BF16X6) {
    const int nfrag = ntiles * (H / 16) * 64;
    if (!c.workspace_ready)
      hipLaunchKernelGGL(radial_mlp_split_w1_fwd_kernel, dim3((unsigned)((nfrag + 255) / 256)), dim3(256), 0, s, b, a1, H,
                         W, wf);
    if (cotangent != nullptr) {
      const float* ct = static_cast<const float*>(cotangent);
      by_h(H, [&](auto h) {
        hipLaunchKernelGGL((radial_mlp_fwd_bf16x6_kernel<decltype(h)::value, true>), dim3(grid), dim3(256), 0, s, e, a, wf,
                           a0, nb, W, E, o, ct);
      });
      return launch_status("nqa_radial_mlp_fwd_tangent");
    }
    // default: the balanced form (NQA_MLP_FWD_BALANCED=0: one workgroup per 128-row block)
    if (env_flag("NQA_MLP_FWD_BALANCED", true)) {
      const unsigned gb = balanced_grid();
      by_h(H, [&](auto h) {
        hipLaunchKernelGGL((radial_mlp_fwd_split_bal_kernel<decltype(h)::value, false>), dim3(gb), dim3(256), 0, s, e, a,
                           wf, a0, nb, W, E, o, nullptr);
      });
      return launch_status(c.fn);
    }
    by_h(H, [&](auto h) {
      hipLaunchKernelGGL((radial_mlp_fwd_bf16x6_kernel<decltype(h)::value>), dim3(grid), dim3(256), 0, s, e, a, wf, a0, nb,
                         W, E, o, nullptr);
    });
    return launch_status(c.fn);
  }
  by_h(H, [&](auto h) {
    hipLaunchKernelGGL(radial_mlp_fwd_kernel<decltype(h)::value>, dim3(grid), dim3(256), 0, s, e, a, b, a0, a1, nb, W, E,
                       o, 0);
  });
  return launch_status(c.fn);
}

// backward to the input.  tm = 1 / 2: the training forms (hidden_out, w0_partials; 2: second order along `cotangent`);
// `gw2`: a second gradient stream for the paired rows; the idle hint rides in c.mode.
int mlp_bwd(MlpCall c, int tm, const void* cotangent, void* hidden_out, void* w0_partials, const void* gw, const void* gw2,
            void* grad_in) {
  const std::string fn(c.fn);
  const bool device_idle = !c.xin && (c.mode & NQA_MLP_HINT_DEVICE_IS_IDLE) != 0;
  if (!c.xin) c.mode &= ~NQA_MLP_HINT_DEVICE_IS_IDLE;
  int rc = mlp_check(c, gw != nullptr && grad_in != nullptr);
  if (rc != NQA_OK || c.E == 0) return rc;
  if (gw == nullptr || grad_in == nullptr || c.W % 4 != 0)
    return fail(NQA_ERR_INVALID, fn + ": invalid argument (needs out_features % 4 == 0)");
  const MlpLayout lay = mlp_layout(c.mode, 1, c.H, c.W);
  if (c.workspace == nullptr || c.workspace_bytes < lay.total)
    return fail(NQA_ERR_WORKSPACE, fn + ": workspace missing or too small");
  if (c.mode == NQA_MLP_FP32 && (tm != 0 || gw2 != nullptr))
    return fail(NQA_ERR_UNSUPPORTED,
                "nqa_radial_mlp_bwd_train / _paired: NQA_MLP_BF16X6 or NQA_MLP_F16X3 (no exact-fp32 form)");
  if (gw2 != nullptr && tm != 0) return fail(NQA_ERR_UNSUPPORTED, "nqa_radial_mlp_bwd_paired: inference backward only");
  const MlpWorkspace ws = mlp_view(c.workspace, lay);
  hipStream_t s = static_cast<hipStream_t>(c.stream);
  const int nb = c.nb, H = c.H, W = c.W;
  const int64_t E = c.E;
  const float a0 = (float)c.alpha0, a1 = (float)c.alpha1;
  const float* e = static_cast<const float*>(c.in);
  const float* a = static_cast<const float*>(c.w0);
  const float* b = static_cast<const float*>(c.w1);
  const float* g = static_cast<const float*>(gw);
  const float* g2 = static_cast<const float*>(gw2);
  const float* ct = static_cast<const float*>(cotangent);
  float* ho = static_cast<float*>(hidden_out);
  float* wp = static_cast<float*>(w0_partials);
  float* o = static_cast<float*>(grad_in);
  u32x4* wb = ws.fragments;
  const int nchunks = (W + 31) / 32;
  const unsigned grid = (unsigned)((E + kMlpRows - 1) / kMlpRows);
  const char* launch_fn = g2 != nullptr && !c.xin ? "nqa_radial_mlp_bwd_paired" : c.fn;
  if (c.mode == NQA_MLP_F16X3) {
    int* ce = ws.second_as<int>();
    if (!c.workspace_ready)
      hipLaunchKernelGGL(radial_mlp_split_w1_bwd_f16_kernel, dim3((unsigned)nchunks), dim3(256), 0, s, b, a1, H, W, wb, ce);
    // round 5 (radial_mlp_pipe.h): three more forms of the inference backward, all OPT-IN:
    //   NQA_MLP_BWD_COAL=1     radial_mlp_bwd_coal_kernel (widths that are multiples of 64): g_w in coalesced 256-byte row pieces
    //                          through an LDS transpose -- alone 226-230 us for the cfg-3 middle layer against 240-244 us of the
    //                          general kernel (94 / 96 us first / last layer; profiles/r5_mlp_bwd_kernel_trace.txt);
    //   NQA_MLP_BWD_BALANCED=1 radial_mlp_bwd_pipe_kernel: lane-=-row loads like the general kernel, 235-243 us.
    // Neither is the default: in the step the radial backward runs on a side stream NEXT TO the node / tensor-product kernels,
    // and a persistent launch that holds two workgroups on every CU for its whole duration costs those more than it saves
    // (same-box A/B of the whole step, profiles/r5_step_ab_mlp.txt: 2.37-2.39 ms with the general backward kernel, 2.48-2.49 ms
    // with the coalesced persistent one, both with the new forward).
    //   NQA_MLP_BWD_SMALL      0 never (default), 1 with NQA_MLP_HINT_DEVICE_IS_IDLE, 2 whenever the shape fits: narrow
    //                          outputs (W <= 256: the first / last layer of the BASELINE models), all fragments resident in
    //                          LDS, independent wavefronts, epilogue in registers (radial_mlp_bwd_small_kernel: alone 96 -> 76 us
    //                          at cfg-3's W = 192, inside the step 87 -> 72 us for the first layer's launch -- and yet the step
    //                          as a whole comes out 2 % SLOWER in four of four same-box repetitions, with the hint and without;
    //                          profiles/r5_mlp_bwd_small.txt).
    if (!c.xin && tm == 0 && g2 == nullptr && env_flag("NQA_MLP_PIPE", true)) {
      const int small_mode = env_int("NQA_MLP_BWD_SMALL", 0);
      if ((small_mode == 2 || (small_mode == 1 && device_idle)) && H == 128 && W % 32 == 0 && W <= 256) {
        const size_t lds = (size_t)nchunks * (2 * 2 * (H / 32) * 64) * 16 + (size_t)(H / 32) * 16 * 2 * kMaxNb * 4 +
                           (size_t)kMaxNb * H * 4 + (((size_t)nchunks * 4 + 15) & ~(size_t)15);
        static bool attr_set = false;
        if (!attr_set) {
          if (hipFuncSetAttribute(reinterpret_cast<const void*>(&radial_mlp_bwd_small_kernel<128>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512) != hipSuccess) {
            (void)hipGetLastError();
          }
          attr_set = true;
        }
        const int64_t want = ((E + 31) / 32 + 7) / 8;  // one 32-row block per wavefront at least
        const unsigned gb = (unsigned)(want < (int64_t)mlp_num_cus() ? want : (int64_t)mlp_num_cus());
        hipLaunchKernelGGL((radial_mlp_bwd_small_kernel<128>), dim3(gb), dim3(512), lds, s, e, a, wb, g, a0, nb, W, E, o, ce);
        return launch_status(c.fn);
      }
      const bool balanced = env_flag("NQA_MLP_BWD_BALANCED", false);
      const bool use_coal = env_flag("NQA_MLP_BWD_COAL", false) && H == 128 && W % 64 == 0;
      if (use_coal || (balanced && W % 32 == 0)) {
        // NQA_MLP_BWD_WGS_PER_CU=1: half the chip for the (side-stream) persistent launch
        const int per_cu = env_int("NQA_MLP_BWD_WGS_PER_CU", 2);
        const int64_t slots = (int64_t)(per_cu >= 1 && per_cu <= 2 ? per_cu : 2) * mlp_num_cus();
        const unsigned gb = (unsigned)((int64_t)grid < slots ? (int64_t)grid : slots);
        if (hipMemsetAsync(o, 0, (size_t)E * nb * sizeof(float), s) != hipSuccess)
          return fail(NQA_ERR_LAUNCH, fn + ": hipMemsetAsync failed");
        const auto launch = [&](auto h, auto pf) {
          hipLaunchKernelGGL((radial_mlp_bwd_pipe_kernel<decltype(h)::value, decltype(pf)::value>), dim3(gb), dim3(256), 0,
                             s, e, a, wb, g, a0, nb, W, E, o, ce);
        };
        if (use_coal && !balanced)
          hipLaunchKernelGGL((radial_mlp_bwd_coal_kernel<128>), dim3(gb), dim3(256), 0, s, e, a, wb, g, a0, nb, W, E, o, ce);
        else if (H == 64) launch(ic<64>{}, ic<2>{});
        else if (env_int("NQA_MLP_BWD_PF", 2) == 4) launch(ic<128>{}, ic<4>{});
        else launch(ic<128>{}, ic<2>{});
        return launch_status(c.fn);
      }
    }
    by_h_tm_pair(H, tm, g2 != nullptr, [&](auto h, auto t, auto p) {
      constexpr int HH = decltype(h)::value, TT = decltype(t)::value;
      constexpr bool PP = decltype(p)::value;
      if constexpr (TT == 0) {
        if (c.xin) {
          hipLaunchKernelGGL((radial_mlp_bwd_split_kernel<HH, 0, PP, true, true>), dim3(grid), dim3(256), 0, s, e, a, wb, g,
                             a0, nb, W, E, o, 0, ct, ho, wp, g2, ce);
          return;
        }
      }
      hipLaunchKernelGGL((radial_mlp_bwd_split_kernel<HH, TT, PP, true>), dim3(grid), dim3(256), 0, s, e, a, wb, g, a0, nb,
                         W, E, o, 0, ct, ho, wp, g2, ce);
    });
    return launch_status(launch_fn);
  }
  if (c.mode == NQA_MLP_BF16X6) {
    const int nfrag = nchunks * 2 * (H / 32) * 64;
    if (!c.workspace_ready)
      hipLaunchKernelGGL(radial_mlp_split_w1_bwd_kernel, dim3((unsigned)((nfrag + 255) / 256)), dim3(256), 0, s, b, a1, H,
                         W, wb);
    by_h_tm_pair(H, tm, g2 != nullptr, [&](auto h, auto t, auto p) {
      constexpr int HH = decltype(h)::value, TT = decltype(t)::value;
      constexpr bool PP = decltype(p)::value;
      hipLaunchKernelGGL((radial_mlp_bwd_split_kernel<HH, TT, PP>), dim3(grid), dim3(256), 0, s, e, a, wb, g, a0, nb, W, E,
                         o, 0, ct, ho, wp, g2, nullptr);
    });
    return launch_status(launch_fn);
  }
  float* w1t = static_cast<float*>(c.workspace);  // [W (+ padding rows read by the last chunk)][H]
  if (!c.workspace_ready)
    hipLaunchKernelGGL(radial_mlp_transpose_w1_kernel, dim3((unsigned)((H * W + 255) / 256)), dim3(256), 0, s, b, a1, H, W,
                       w1t);
  by_h(H, [&](auto h) {
    hipLaunchKernelGGL(radial_mlp_bwd_kernel<decltype(h)::value>, dim3(grid), dim3(256), 0, s, e, a, w1t, g, a0, nb, W, E,
                       o);
  });
  return launch_status(c.fn);
}

}  // namespace

extern "C" {

int nqa_radial_mlp_supported(int32_t dtype, int32_t num_basis, int32_t hidden, int32_t out_features) {
  return (dtype == NQA_F32 && num_basis > 0 && num_basis <= kMaxNb && (hidden == 64 || hidden == 128) &&
          out_features > 0 && out_features % 4 == 0)
             ? 1
             : 0;
}

int64_t nqa_radial_mlp_workspace_bytes(int32_t mode, int32_t backward, int32_t hidden, int32_t out_features) {
  return mlp_layout(mode, backward, hidden, out_features).total;
}

int64_t nqa_radial_mlp_train_tiles(int64_t num_edges) {
  return num_edges <= 0 ? 0 : (num_edges + kMlpRows - 1) / kMlpRows;
}

int nqa_radial_mlp_fwd(int32_t dtype, int32_t mode, const void* edge_embedding, const void* w0, double alpha0,
                       const void* w1, double alpha1, int32_t num_basis, int32_t hidden, int32_t out_features,
                       int64_t num_edges, void* edge_weight, void* workspace, int64_t workspace_bytes,
                       int32_t workspace_ready, nqa_stream stream) {
  return mlp_fwd({"nqa_radial_mlp_fwd", dtype, mode, false, edge_embedding, w0, alpha0, w1, alpha1, num_basis, hidden,
                  out_features, num_edges, workspace, workspace_bytes, workspace_ready, stream},
                 nullptr, edge_weight);
}

int nqa_radial_mlp_fwd_tangent(int32_t dtype, int32_t mode, const void* edge_embedding, const void* cotangent,
                               const void* w0, double alpha0, const void* w1, double alpha1, int32_t num_basis,
                               int32_t hidden, int32_t out_features, int64_t num_edges, void* out, void* workspace,
                               int64_t workspace_bytes, int32_t workspace_ready, nqa_stream stream) {
  if (num_edges > 0 && cotangent == nullptr)
    return fail(NQA_ERR_INVALID, "nqa_radial_mlp_fwd_tangent: cotangent is required");
  return mlp_fwd({"nqa_radial_mlp_fwd", dtype, mode, false, edge_embedding, w0, alpha0, w1, alpha1, num_basis, hidden,
                  out_features, num_edges, workspace, workspace_bytes, workspace_ready, stream},
                 cotangent, out);
}

int nqa_radial_mlp_bwd(int32_t dtype, int32_t mode, const void* edge_embedding, const void* w0, double alpha0,
                       const void* w1, double alpha1, const void* grad_edge_weight, int32_t num_basis,
                       int32_t hidden, int32_t out_features, int64_t num_edges, void* grad_edge_embedding,
                       void* workspace, int64_t workspace_bytes, int32_t workspace_ready, nqa_stream stream) {
  return mlp_bwd({"nqa_radial_mlp_bwd", dtype, mode, false, edge_embedding, w0, alpha0, w1, alpha1, num_basis, hidden,
                  out_features, num_edges, workspace, workspace_bytes, workspace_ready, stream},
                 0, nullptr, nullptr, nullptr, grad_edge_weight, nullptr, grad_edge_embedding);
}

int nqa_radial_mlp_bwd_paired(int32_t dtype, int32_t mode, const void* edge_embedding, const void* w0, double alpha0,
                              const void* w1, double alpha1, const void* grad_edge_weight,
                              const void* grad_edge_weight2, int32_t num_basis, int32_t hidden, int32_t out_features,
                              int64_t num_edges, void* grad_edge_embedding, void* workspace, int64_t workspace_bytes,
                              int32_t workspace_ready, nqa_stream stream) {
  if (num_edges > 0 && grad_edge_weight2 == nullptr)
    return fail(NQA_ERR_INVALID, "nqa_radial_mlp_bwd_paired: second gradient stream is required");
  return mlp_bwd({"nqa_radial_mlp_bwd", dtype, mode, false, edge_embedding, w0, alpha0, w1, alpha1, num_basis, hidden,
                  out_features, num_edges, workspace, workspace_bytes, workspace_ready, stream},
                 0, nullptr, nullptr, nullptr, grad_edge_weight, grad_edge_weight2, grad_edge_embedding);
}

int nqa_radial_mlp_bwd_train(int32_t dtype, int32_t mode, const void* edge_embedding, const void* cotangent,
                             const void* w0, double alpha0, const void* w1, double alpha1,
                             const void* grad_edge_weight, int32_t num_basis, int32_t hidden, int32_t out_features,
                             int64_t num_edges, void* grad_edge_embedding, void* hidden_out, void* w0_partials,
                             void* workspace, int64_t workspace_bytes, int32_t workspace_ready, nqa_stream stream) {
  if (num_edges > 0 && (hidden_out == nullptr || w0_partials == nullptr))
    return fail(NQA_ERR_INVALID, "nqa_radial_mlp_bwd_train: hidden_out and w0_partials are required");
  return mlp_bwd({"nqa_radial_mlp_bwd", dtype, mode, false, edge_embedding, w0, alpha0, w1, alpha1, num_basis, hidden,
                  out_features, num_edges, workspace, workspace_bytes, workspace_ready, stream},
                 cotangent ? 2 : 1, cotangent, hidden_out, w0_partials, grad_edge_weight, nullptr, grad_edge_embedding);
}

// ---- the last layer of a deeper MLP on the same GEMM cores (depth >= 2: nequip/nn/mlp.py:81-196 with
// hidden_layers_depth >= 2, e.g. configs/tutorial.yaml:222-223) -------------------------------------------------------
int nqa_radial_mlp_last_fwd(int32_t dtype, int32_t mode, const void* pre, const void* w, double alpha, int32_t hidden,
                            int32_t out_features, int64_t num_edges, void* out, void* workspace, int64_t workspace_bytes,
                            int32_t workspace_ready, nqa_stream stream) {
  return mlp_fwd({"nqa_radial_mlp_last_fwd", dtype, mode, true, pre, nullptr, 1.0, w, alpha, 0, hidden, out_features,
                  num_edges, workspace, workspace_bytes, workspace_ready, stream},
                 nullptr, out);
}

int nqa_radial_mlp_last_bwd(int32_t dtype, int32_t mode, const void* pre, const void* w, double alpha,
                            const void* grad_out, const void* grad_out2, int32_t hidden, int32_t out_features,
                            int64_t num_edges, void* grad_pre, void* workspace, int64_t workspace_bytes,
                            int32_t workspace_ready, nqa_stream stream) {
  return mlp_bwd({"nqa_radial_mlp_last_bwd", dtype, mode, true, pre, nullptr, 1.0, w, alpha, 0, hidden, out_features,
                  num_edges, workspace, workspace_bytes, workspace_ready, stream},
                 0, nullptr, nullptr, nullptr, grad_out, grad_out2, grad_pre);
}

}  // extern "C"
