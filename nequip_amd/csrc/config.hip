// Conflict-free inverse gradients, ConFIG (nequip/train/config.py::ConFIGLightningModule._ConFIG_backwards, arXiv 2408.11104)
// as multi-tensor launches.
//
// The reference stacks the K per-term gradients into a [K, P] matrix, normalises its rows, solves the underdetermined system
// with torch.linalg.lstsq (or pinv) on the tall matrix and reads the result back on the host.  Every number of that method is a
// function of the K x K Gram matrix G_kl = g_k . g_l, and the new gradient is a linear combination of the g_k:
//   n_k = max(sqrt(G_kk), eps)      Gh_kl = G_kl / (n_k n_l)      bh = b / max(|b|, eps)
//   c   = pinv(Gh) bh   (cyclic Jacobi; eigenvalues <= CONFIG_TAU * lambda_max are dropped)
//   xi  = sqrt(max(c' Gh c, 0))     d = max(xi, eps)     s = (sum_k sum_l G_kl c_l / n_l) / d
//   w_l = s c_l / (n_l d)           new_grad = sum_l w_l g_l          |new_grad| = |s| xi / d
// Layout: the tensor table and chunk map of multi_tensor.h, with the records of ema.hip (nqa_ema_tensor).  In a table entry
// `ema` is the .grad of a parameter and `param` its slice of ROW 0 of the [K, row_stride] buffer of collected gradients; row k
// lies k * row_stride elements further.  row_stride is a multiple of 4 elements, so every row is 16-byte aligned when row 0 is.
//   config_collect_kernel   row k of the buffer = .grad (widened exactly where the buffer is float64), .grad = 0, one pass; with
//                           row < 0 only the zeros.
//   config_gram_kernel      one workgroup per CONFIG_GRAM_CHUNK elements of the rows: the K (K + 1) / 2 products in double, lanes
//                           by shuffles, waves through LDS, all in a fixed order; written to partials[chunk][pair].
//   config_solve_kernel     one workgroup: the partials added in a fixed order, then one thread runs the solve above on
//                           matrices in LDS and writes out = [w_0 .. w_7, |new_grad|, clip factor].  With clip_mode "norm" the
//                           factor min(1, clip / (|new_grad| + 1e-6)) (torch's clip_grad_norm_) is folded into w.
//   config_apply_kernel     .grad[i] = (dtype of the parameter) clamp( sum_l w_l row_l[i] ), the sum in double; the clamp to
//                           +-clip only with clip_mode "value" (NaN passes, as in torch's clamp).
// No floating-point atomics, nothing read by the host: the same gradients give the same bits, and all four capture.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "multi_tensor.h"

namespace nqa {

constexpr int CONFIG_CHUNK = NQA_EMA_CHUNK;
constexpr int CONFIG_THREADS = 256;
constexpr int CONFIG_WAVES = CONFIG_THREADS / 64;
constexpr int CONFIG_GRAM_CHUNK = NQA_CONFIG_GRAM_CHUNK;
constexpr int CONFIG_MAX_K = NQA_CONFIG_MAX_TERMS;
constexpr int CONFIG_MAX_PAIRS = CONFIG_MAX_K * (CONFIG_MAX_K + 1) / 2;
constexpr double CONFIG_TAU = 1e-12;
constexpr int CONFIG_SWEEPS = 30;
static_assert(CONFIG_MAX_K == 8 && NQA_CONFIG_OUT == CONFIG_MAX_K + 2, "out = [w_0 .. w_7, |new_grad|, clip factor]");

// ---- collect --------------------------------------------------------------------------------------------------------------------
// S: dtype of the .grad, D: dtype of the buffer (float -> float, float -> double, double -> double)
template <typename S, typename D>
__device__ __forceinline__ void config_collect_chunk(void* grad, void* row, int64_t offset, int len) {
  NQA_GLOBAL S* g = (NQA_GLOBAL S*)grad + offset;
  NQA_GLOBAL D* r = row ? (NQA_GLOBAL D*)row + offset : nullptr;
  chunk_walk<S, CONFIG_THREADS>(len, aligned16(g, r), [&](int i, auto width) {
    constexpr int N = decltype(width)::value;
    S x[N];
    if (r) {
      D y[N];
      pack_load<S, N>(g + i, x);
#pragma unroll
      for (int j = 0; j < N; ++j) y[j] = (D)x[j];
      pack_store<D, N>(r + i, y);
    }
#pragma unroll
    for (int j = 0; j < N; ++j) x[j] = S(0);
    pack_store<S, N>(g + i, x);
  });
}

__global__ __launch_bounds__(CONFIG_THREADS) void config_collect_kernel(const nqa_ema_tensor* __restrict__ tensors,
                                                                         const nqa_mt_chunk* __restrict__ chunks,
                                                                         const int64_t* __restrict__ n_chunks, int row,
                                                                         int64_t row_stride, int buf_dtype) {
  nqa_ema_tensor t;
  int64_t offset;
  int len;
  if (!chunk_of<CONFIG_CHUNK>(tensors, chunks, n_chunks, t, offset, len)) return;
  const int64_t esz = buf_dtype == NQA_F64 ? 8 : 4;
  void* dst = row < 0 ? nullptr : (void*)((char*)t.param + (int64_t)row * row_stride * esz);
  // (a float64 .grad under a float32 buffer is outside the contract of nequip_amd.h: the chunk is skipped)
  if (t.dtype == NQA_F64) {
    if (buf_dtype == NQA_F64) config_collect_chunk<double, double>(t.ema, dst, offset, len);
  } else if (buf_dtype == NQA_F64) {
    config_collect_chunk<float, double>(t.ema, dst, offset, len);
  } else {
    config_collect_chunk<float, float>(t.ema, dst, offset, len);
  }
}

// ---- Gram matrix ----------------------------------------------------------------------------------------------------------------
template <int K, typename D>
__device__ __forceinline__ void config_gram_chunk(const D* __restrict__ buf, int64_t row_stride, int64_t start, int len,
                                                  double* __restrict__ out, double (*lds)[CONFIG_MAX_PAIRS]) {
  constexpr int NP = K * (K + 1) / 2;
  double acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) acc[p] = 0.0;
  const D* base = buf + start;
  for (int i = threadIdx.x; i < len; i += CONFIG_THREADS) {
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (double)base[(int64_t)k * row_stride + i];
    int p = 0;
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int l = k; l < K; ++l) acc[p++] += v[k] * v[l];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    double a = acc[p];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
    if (lane == 0) lds[wave][p] = a;
  }
  __syncthreads();
  if (threadIdx.x < NP) {
    double a = lds[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < CONFIG_WAVES; ++w) a += lds[w][threadIdx.x];
    out[threadIdx.x] = a;
  }
}

template <typename D>
__global__ __launch_bounds__(CONFIG_THREADS) void config_gram_kernel(const D* __restrict__ buf, int K, int64_t row_stride,
                                                                      const int64_t* __restrict__ numel,
                                                                      double* __restrict__ partials) {
  __shared__ double lds[CONFIG_WAVES][CONFIG_MAX_PAIRS];
  const int64_t start = (int64_t)blockIdx.x * CONFIG_GRAM_CHUNK;
  const int64_t left = *numel - start;
  if (left <= 0) return;
  const int len = left < CONFIG_GRAM_CHUNK ? (int)left : CONFIG_GRAM_CHUNK;
  double* out = partials + (int64_t)blockIdx.x * (K * (K + 1) / 2);
  switch (K) {
    case 2: config_gram_chunk<2, D>(buf, row_stride, start, len, out, lds); break;
    case 3: config_gram_chunk<3, D>(buf, row_stride, start, len, out, lds); break;
    case 4: config_gram_chunk<4, D>(buf, row_stride, start, len, out, lds); break;
    case 5: config_gram_chunk<5, D>(buf, row_stride, start, len, out, lds); break;
    case 6: config_gram_chunk<6, D>(buf, row_stride, start, len, out, lds); break;
    case 7: config_gram_chunk<7, D>(buf, row_stride, start, len, out, lds); break;
    case 8: config_gram_chunk<8, D>(buf, row_stride, start, len, out, lds); break;
    default: break;
  }
}

// ---- the K x K solve ------------------------------------------------------------------------------------------------------------
// Matrices are [8][8] whatever K (in LDS on the device: one thread, run-time indices, no scratch).
struct ConfigSolveSpace {
  double G[CONFIG_MAX_K * CONFIG_MAX_K];   // Gram matrix of the raw gradients
  double Gh[CONFIG_MAX_K * CONFIG_MAX_K];  // ... of the normalised ones
  double A[CONFIG_MAX_K * CONFIG_MAX_K];   // Gh, diagonalised in place
  double V[CONFIG_MAX_K * CONFIG_MAX_K];   // eigenvectors in columns
  double n[CONFIG_MAX_K], bh[CONFIG_MAX_K], c[CONFIG_MAX_K];
};

// `gram`: the K (K + 1) / 2 entries of the upper triangle, row by row.  `out`: NQA_CONFIG_OUT doubles.
__host__ __device__ inline void config_solve(ConfigSolveSpace& s, const double* gram, int K, const double* b, double eps,
                                             int clip_mode, double clip, double* out) {
  constexpr int M = CONFIG_MAX_K;
  int p = 0;
  for (int k = 0; k < K; ++k)
    for (int l = k; l < K; ++l) s.G[k * M + l] = s.G[l * M + k] = gram[p++];
  double bn = 0.0;
  for (int k = 0; k < K; ++k) {
    const double r = sqrt(s.G[k * M + k]);
    s.n[k] = r > eps ? r : eps;
    bn += b[k] * b[k];
  }
  bn = sqrt(bn);
  bn = bn > eps ? bn : eps;
  for (int k = 0; k < K; ++k) {
    s.bh[k] = b[k] / bn;
    for (int l = 0; l < K; ++l) {
      s.Gh[k * M + l] = s.A[k * M + l] = s.G[k * M + l] / (s.n[k] * s.n[l]);
      s.V[k * M + l] = k == l ? 1.0 : 0.0;
    }
  }
  // cyclic Jacobi: until the off-diagonal part is below 2^-53 of the diagonal one (relative, in norm)
  for (int sweep = 0; sweep < CONFIG_SWEEPS; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < K; ++i) {
      diag += s.A[i * M + i] * s.A[i * M + i];
      for (int j = i + 1; j < K; ++j) off += s.A[i * M + j] * s.A[i * M + j];
    }
    if (!(off > 1.2e-32 * diag)) break;  // (also leaves on NaN)
    for (int i = 0; i < K - 1; ++i)
      for (int j = i + 1; j < K; ++j) {
        const double aij = s.A[i * M + j];
        if (aij == 0.0) continue;
        const double theta = (s.A[j * M + j] - s.A[i * M + i]) / (2.0 * aij);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
        for (int r = 0; r < K; ++r) {
          const double x = s.A[r * M + i], y = s.A[r * M + j];
          s.A[r * M + i] = cs * x - sn * y;
          s.A[r * M + j] = sn * x + cs * y;
        }
        for (int r = 0; r < K; ++r) {
          const double x = s.A[i * M + r], y = s.A[j * M + r];
          s.A[i * M + r] = cs * x - sn * y;
          s.A[j * M + r] = sn * x + cs * y;
        }
        for (int r = 0; r < K; ++r) {
          const double x = s.V[r * M + i], y = s.V[r * M + j];
          s.V[r * M + i] = cs * x - sn * y;
          s.V[r * M + j] = sn * x + cs * y;
        }
      }
  }
  double lmax = 0.0;
  for (int i = 0; i < K; ++i) lmax = s.A[i * M + i] > lmax ? s.A[i * M + i] : lmax;
  for (int k = 0; k < K; ++k) s.c[k] = 0.0;
  for (int i = 0; i < K; ++i) {
    const double lam = s.A[i * M + i];
    if (!(lam > CONFIG_TAU * lmax)) continue;  // (lmax == 0: every one is dropped, c = 0)
    double proj = 0.0;
    for (int k = 0; k < K; ++k) proj += s.V[k * M + i] * s.bh[k];
    proj /= lam;
    for (int k = 0; k < K; ++k) s.c[k] += s.V[k * M + i] * proj;
  }
  double xi2 = 0.0, dot = 0.0;
  for (int k = 0; k < K; ++k)
    for (int l = 0; l < K; ++l) {
      xi2 += s.c[k] * s.Gh[k * M + l] * s.c[l];
      dot += s.G[k * M + l] * s.c[l] / s.n[l];
    }
  const double xi = sqrt(xi2 > 0.0 ? xi2 : 0.0);
  const double d = xi > eps ? xi : eps;
  const double scale = dot / d;
  const double norm = fabs(scale) * xi / d;
  double factor = 1.0;
  if (clip_mode == NQA_CONFIG_CLIP_NORM) {
    const double f = clip / (norm + 1e-6);
    factor = f < 1.0 ? f : 1.0;
  }
  for (int l = 0; l < M; ++l) out[l] = l < K ? factor * (scale * s.c[l] / (s.n[l] * d)) : 0.0;
  out[M] = norm;
  out[M + 1] = factor;
}

__global__ __launch_bounds__(CONFIG_THREADS) void config_solve_kernel(const double* __restrict__ partials, int K,
                                                                       const int64_t* __restrict__ numel, int64_t gram_capacity,
                                                                       const double* __restrict__ b, double eps, int clip_mode,
                                                                       double clip, double* __restrict__ out) {
  __shared__ double red[CONFIG_WAVES];
  __shared__ double gram[CONFIG_MAX_PAIRS];
  __shared__ ConfigSolveSpace space;
  const int n_pairs = K * (K + 1) / 2;
  int64_t n = (*numel + CONFIG_GRAM_CHUNK - 1) / CONFIG_GRAM_CHUNK;
  n = n < 0 ? 0 : (n > gram_capacity ? gram_capacity : n);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int p = 0; p < n_pairs; ++p) {
    double a = 0.0;
    for (int64_t c = threadIdx.x; c < n; c += CONFIG_THREADS) a += partials[c * n_pairs + p];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
    if (lane == 0) red[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = red[0];
#pragma unroll
      for (int w = 1; w < CONFIG_WAVES; ++w) t += red[w];
      gram[p] = t;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) config_solve(space, gram, K, b, eps, clip_mode, clip, out);
}

// ---- apply ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double config_clamp(double v, bool clamp, double clip) {
  return clamp ? (v > clip ? clip : (v < -clip ? -clip : v)) : v;  // (NaN fails both comparisons and passes)
}

template <typename S, typename D>
__device__ __forceinline__ void config_apply_chunk(void* grad, const void* row0, int64_t offset, int len, int K, int64_t row_stride,
                                                   const double* __restrict__ w, bool clamp, double clip) {
  NQA_GLOBAL S* g = (NQA_GLOBAL S*)grad + offset;
  NQA_GLOBAL const D* r = (NQA_GLOBAL const D*)row0 + offset;
  // (rows are row_stride apart, a multiple of 16 bytes)
  chunk_walk<S, CONFIG_THREADS>(len, aligned16(g, r), [&](int i, auto width) {
    constexpr int N = decltype(width)::value;
    double acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.0;
    for (int l = 0; l < K; ++l) {
      D x[N];
      pack_load<D, N>(r + (int64_t)l * row_stride + i, x);
      const double wl = w[l];
#pragma unroll
      for (int j = 0; j < N; ++j) acc[j] += wl * (double)x[j];
    }
    S y[N];
#pragma unroll
    for (int j = 0; j < N; ++j) y[j] = (S)config_clamp(acc[j], clamp, clip);
    pack_store<S, N>(g + i, y);
  });
}

__global__ __launch_bounds__(CONFIG_THREADS) void config_apply_kernel(const nqa_ema_tensor* __restrict__ tensors,
                                                                       const nqa_mt_chunk* __restrict__ chunks,
                                                                       const int64_t* __restrict__ n_chunks, int K, int64_t row_stride,
                                                                       int buf_dtype, const double* __restrict__ w, int clip_mode,
                                                                       double clip) {
  nqa_ema_tensor t;
  int64_t offset;
  int len;
  if (!chunk_of<CONFIG_CHUNK>(tensors, chunks, n_chunks, t, offset, len)) return;
  const bool clamp = clip_mode == NQA_CONFIG_CLIP_VALUE;
  if (t.dtype == NQA_F64) {
    if (buf_dtype == NQA_F64) config_apply_chunk<double, double>(t.ema, t.param, offset, len, K, row_stride, w, clamp, clip);
  } else if (buf_dtype == NQA_F64) {
    config_apply_chunk<float, double>(t.ema, t.param, offset, len, K, row_stride, w, clamp, clip);
  } else {
    config_apply_chunk<float, float>(t.ema, t.param, offset, len, K, row_stride, w, clamp, clip);
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
static int config_invalid(const char* name, const char* what) {
  set_error(std::string(name) + ": " + what);
  return NQA_ERR_INVALID;
}

static int config_check_tables(const char* name, const void* tensors, const void* chunks, int64_t chunk_capacity,
                               const void* n_chunks, int64_t row_stride, int buf_dtype) {
  const int rc = check_tables(name, tensors, chunks, chunk_capacity, n_chunks);
  if (rc != NQA_OK) return rc;
  if (row_stride < 0 || row_stride % 4 != 0) return config_invalid(name, "row_stride must be a multiple of 4 elements");
  if (buf_dtype != NQA_F32 && buf_dtype != NQA_F64) return config_invalid(name, "the buffer is float32 or float64");
  return NQA_OK;
}

static bool config_clip_ok(int clip_mode, double clip) {
  if (clip_mode == NQA_CONFIG_CLIP_NONE) return true;
  return (clip_mode == NQA_CONFIG_CLIP_NORM || clip_mode == NQA_CONFIG_CLIP_VALUE) && clip >= 0.0;
}

}  // namespace nqa

extern "C" {

int32_t nqa_config_gram_chunk_elems(void) { return nqa::CONFIG_GRAM_CHUNK; }

int nqa_config_collect(const nqa_ema_tensor* tensors, const nqa_mt_chunk* chunks, int64_t chunk_capacity, const int64_t* n_chunks,
                       int32_t row, int64_t row_stride, int32_t buf_dtype, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_config_collect";
  const int rc = config_check_tables(name, tensors, chunks, chunk_capacity, n_chunks, row_stride, buf_dtype);
  if (rc != NQA_OK) return rc;
  if (row >= CONFIG_MAX_K) return config_invalid(name, "row must be below 8 (negative: only zero the gradients)");
  if (chunk_capacity == 0) return NQA_OK;
  hipLaunchKernelGGL(config_collect_kernel, dim3((unsigned)chunk_capacity), dim3(CONFIG_THREADS), 0,
                     static_cast<hipStream_t>(stream), tensors, chunks, n_chunks, (int)row, row_stride, (int)buf_dtype);
  return launch_status(name);
}

int nqa_config_gram(const void* buf, int32_t buf_dtype, int32_t n_terms, int64_t row_stride, const int64_t* numel,
                    int64_t gram_capacity, double* partials, const double* b, double norm_eps, int32_t clip_mode, double clip,
                    double* out, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_config_gram";
  if (n_terms < 2 || n_terms > CONFIG_MAX_K) return config_invalid(name, "2 <= n_terms <= 8");
  if (buf_dtype != NQA_F32 && buf_dtype != NQA_F64) return config_invalid(name, "the buffer is float32 or float64");
  if (gram_capacity < 0 || gram_capacity > INT32_MAX || row_stride < 0 || !numel || !b || !out ||
      (gram_capacity > 0 && (!buf || !partials)))
    return config_invalid(name, "buf, numel, partials, b and out are required, 0 <= gram_capacity < 2^31");
  if (!(norm_eps >= 0.0) || !config_clip_ok(clip_mode, clip))
    return config_invalid(name, "norm_eps >= 0, clip_mode none / norm / value with clip >= 0");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (gram_capacity > 0) {
    if (buf_dtype == NQA_F64)
      hipLaunchKernelGGL(config_gram_kernel<double>, dim3((unsigned)gram_capacity), dim3(CONFIG_THREADS), 0, s,
                         (const double*)buf, (int)n_terms, row_stride, numel, partials);
    else
      hipLaunchKernelGGL(config_gram_kernel<float>, dim3((unsigned)gram_capacity), dim3(CONFIG_THREADS), 0, s, (const float*)buf,
                         (int)n_terms, row_stride, numel, partials);
  }
  hipLaunchKernelGGL(config_solve_kernel, dim3(1), dim3(CONFIG_THREADS), 0, s, (const double*)partials, (int)n_terms, numel,
                     gram_capacity, b, norm_eps, (int)clip_mode, clip, out);
  return launch_status(name);
}

int nqa_config_apply(const nqa_ema_tensor* tensors, const nqa_mt_chunk* chunks, int64_t chunk_capacity, const int64_t* n_chunks,
                     int32_t n_terms, int64_t row_stride, int32_t buf_dtype, const double* weights, int32_t clip_mode, double clip,
                     nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_config_apply";
  const int rc = config_check_tables(name, tensors, chunks, chunk_capacity, n_chunks, row_stride, buf_dtype);
  if (rc != NQA_OK) return rc;
  if (n_terms < 1 || n_terms > CONFIG_MAX_K || !weights || !config_clip_ok(clip_mode, clip))
    return config_invalid(name, "1 <= n_terms <= 8, weights required, clip_mode none / norm / value with clip >= 0");
  if (chunk_capacity == 0) return NQA_OK;
  hipLaunchKernelGGL(config_apply_kernel, dim3((unsigned)chunk_capacity), dim3(CONFIG_THREADS), 0, static_cast<hipStream_t>(stream),
                     tensors, chunks, n_chunks, (int)n_terms, row_stride, (int)buf_dtype, weights, (int)clip_mode, clip);
  return launch_status(name);
}

int nqa_config_solve_host(const double* gram, int32_t n_terms, const double* b, double norm_eps, int32_t clip_mode, double clip,
                          double* out) {
  using namespace nqa;
  const char* name = "nqa_config_solve_host";
  if (n_terms < 1 || n_terms > CONFIG_MAX_K || !gram || !b || !out || !(norm_eps >= 0.0) || !config_clip_ok(clip_mode, clip))
    return config_invalid(name, "1 <= n_terms <= 8, host pointers gram / b / out, norm_eps >= 0, a valid clip");
  ConfigSolveSpace space;
  config_solve(space, gram, n_terms, b, norm_eps, clip_mode, clip, out);
  return NQA_OK;
}

}  // extern "C"
