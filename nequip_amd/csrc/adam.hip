// Adam / AdamW (torch.optim.Adam, torch.optim.AdamW: the optimizer of the reference's default training recipe) with gradient
// clipping, and ReduceLROnPlateau (torch.optim.lr_scheduler.ReduceLROnPlateau, the recipe's scheduler), as multi-tensor launches.
//
// torch's capturable Adam is some 47 launches per step at the train256 parameter set, and its scheduler writes a Python float
// that a captured step never sees.  Here the hyper-parameters of every parameter group are a record in device memory, which the
// scheduler's one-thread kernel rewrites and every step reads; the step count is the 0-d float32 `step` tensor of every
// parameter, as torch's capturable and fused forms keep it.
//
// Layout: the tensor table and chunk map of multi_tensor.h; a table entry is (parameter, .grad, exp_avg, exp_avg_sq,
// max_exp_avg_sq, step, element count, dtype, group), and there is one nqa_adam_group RECORD per parameter group.
//   adam_step_kernel      every workgroup reads its tensor's record, its group's record, *step and the clip record, and forms
//                         step + 1, bc1, bc2, lr / bc1 and sqrt(bc2) from the OLD values (pure functions of them: no workgroup
//                         depends on another), in double, each rounded once to the tensor's arithmetic type as ATen rounds a
//                         Python scalar; then per element torch's _single_tensor_adam:
//                           g = clip(grad);  maximize: g = -g;  coupled: g += wd p;  decoupled: p *= 1 - lr wd
//                           m = lerp(m, g, 1 - b1);  v = b2 v + (1 - b2) g g;  amsgrad: vmax = max(vmax, v), v := vmax below
//                           p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)                              (ATen's lerp)
//                         A tensor whose .grad is null is skipped, its state untouched.  .grad is only read.
//   adam_advance_kernel   one thread per table entry commits *step += 1 for the entries with a .grad.  A SECOND launch on the same
//                         stream, the rule of ema.hip's advance: every workgroup of the step has read the old count before its
//                         single writer starts.  No ticket, no atomics, no fence.
//   adam_sumsq_kernel     one wavefront per chunk: the squares of the chunk's gradient elements summed in double, every lane its
//                         elements in ascending order, the lanes by a fixed shuffle tree: one partial per chunk.
//   adam_norm_kernel      one wavefront: lane l adds a contiguous run of the partials in index order, lane 0 adds the 64 lane
//                         sums in lane order (through LDS, the only LDS of this file) and writes norm and
//                         factor = min(1, max_norm / (norm + 1e-6)), clip_grad_norm_'s.  No floating-point atomics: the same
//                         inputs give the same bits.
//   adam_plateau_kernel   one thread: torch's ReduceLROnPlateau.step on the metric behind a device pointer; when the patience is
//                         exhausted lr = max(lr factor, min_lr) is written into every group record whose lr - new_lr > eps.
//                         Compiled without contraction: every comparison is the IEEE operation torch's Python performs.
// Plain vector loads and stores.  Nothing is read by the host.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "multi_tensor.h"

namespace nqa {

constexpr int ADAM_CHUNK = NQA_EMA_CHUNK;
constexpr int ADAM_THREADS = 256;
constexpr int ADAM_WAVE = 64;
static_assert(sizeof(nqa_adam_tensor) == 64 && sizeof(nqa_adam_group) == 64 && sizeof(nqa_adam_clip) == 32 &&
                  sizeof(nqa_adam_plateau_state) == 80 && sizeof(nqa_mt_chunk) == 16,
              "the host writes these tables as 8-byte words");
static_assert((ADAM_CHUNK * sizeof(float)) % 16 == 0, "a chunk must keep the 16-byte alignment of its tensor");

// torch.clamp(g, -c, c): NaN passes; c = +inf is the identity
template <typename T>
__device__ __forceinline__ T adam_clamp(T g, T c) {
  return g < -c ? -c : (g > c ? c : g);
}

template <typename T>
struct AdamStepOp {
  T factor, clip_value, wd, decay, w1, b2, one_minus_b2, bc2_sqrt, eps, neg_step_size;
  bool by_norm, maximize, coupled, decoupled, amsgrad;
  __device__ AdamStepOp(const nqa_adam_group& g, const nqa_adam_clip& c, double step_old)
      : factor((T)c.factor), clip_value((T)c.clip_value), wd((T)g.weight_decay), decay((T)(1.0 - g.lr * g.weight_decay)),
        w1((T)(1.0 - g.beta1)), b2((T)g.beta2), one_minus_b2((T)(1.0 - g.beta2)), eps((T)g.eps), by_norm(c.factor != 1.0),
        maximize(g.maximize != 0), coupled(g.weight_decay != 0.0 && g.decoupled == 0),
        decoupled(g.weight_decay != 0.0 && g.decoupled != 0), amsgrad(g.amsgrad != 0) {
    const double step = step_old + 1.0;
    const double bc1 = 1.0 - pow(g.beta1, step), bc2 = 1.0 - pow(g.beta2, step);
    bc2_sqrt = (T)sqrt(bc2);
    neg_step_size = (T)(-(g.lr / bc1));
  }
  __device__ __forceinline__ void operator()(T& p, T g, T& m, T& v, T& vmax) const {
    if (by_norm) g = g * factor;  // (a factor of exactly 1 leaves every bit, a NaN's payload included)
    g = adam_clamp<T>(g, clip_value);
    if (maximize) g = -g;
    if (decoupled) p = p * decay;
    if (coupled) g = g + wd * p;
    m = lerp<T>(m, g, w1);
    v = b2 * v + one_minus_b2 * g * g;
    T root = v;
    if (amsgrad) root = vmax = (vmax != vmax || vmax > v) ? vmax : v;  // torch.maximum: a NaN of either side stays
    p = p + neg_step_size * (m / (sqrt(root) / bc2_sqrt + eps));
  }
};

// `len` elements at `offset` of the tensors of one table entry
template <typename T, bool AMSGRAD>
__device__ __forceinline__ void adam_step_chunk(const nqa_adam_tensor& t, int64_t offset, int len, const AdamStepOp<T> op) {
  NQA_GLOBAL T* p = (NQA_GLOBAL T*)t.param + offset;
  const NQA_GLOBAL T* g = (const NQA_GLOBAL T*)t.grad + offset;
  NQA_GLOBAL T* m = (NQA_GLOBAL T*)t.exp_avg + offset;
  NQA_GLOBAL T* v = (NQA_GLOBAL T*)t.exp_avg_sq + offset;
  NQA_GLOBAL T* x = AMSGRAD ? (NQA_GLOBAL T*)t.max_exp_avg_sq + offset : nullptr;
  chunk_walk<T, ADAM_THREADS>(len, aligned16(p, g, m, v, x), [&](int i, auto width) {
    constexpr int N = decltype(width)::value;
    T pe[N], ge[N], me[N], ve[N], xe[N] = {};
    pack_load<T, N>(p + i, pe);
    pack_load<T, N>(g + i, ge);
    pack_load<T, N>(m + i, me);
    pack_load<T, N>(v + i, ve);
    if constexpr (AMSGRAD) pack_load<T, N>(x + i, xe);
#pragma unroll
    for (int j = 0; j < N; ++j) op(pe[j], ge[j], me[j], ve[j], xe[j]);
    pack_store<T, N>(p + i, pe);
    pack_store<T, N>(m + i, me);
    pack_store<T, N>(v + i, ve);
    if constexpr (AMSGRAD) pack_store<T, N>(x + i, xe);
  });
}

template <typename T>
__device__ __forceinline__ void adam_step_typed(const nqa_adam_tensor& t, int64_t offset, int len, const nqa_adam_group& g,
                                                const nqa_adam_clip& c, double step_old) {
  const AdamStepOp<T> op(g, c, step_old);
  if (op.amsgrad)
    adam_step_chunk<T, true>(t, offset, len, op);
  else
    adam_step_chunk<T, false>(t, offset, len, op);
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_step_kernel(const nqa_adam_tensor* __restrict__ tensors,
                                                                  const nqa_mt_chunk* __restrict__ chunks,
                                                                  const int64_t* __restrict__ counts,
                                                                  const nqa_adam_group* __restrict__ groups, int32_t n_groups,
                                                                  const nqa_adam_clip* __restrict__ clip) {
  nqa_adam_tensor t;
  int64_t offset;
  int len;
  if (!chunk_of<ADAM_CHUNK>(tensors, chunks, counts, t, offset, len)) return;
  if (t.group < 0 || t.group >= n_groups) return;
  if (!t.grad || !t.param || !t.exp_avg || !t.exp_avg_sq || !t.step) return;  // (.grad is None: the parameter is skipped)
  const nqa_adam_group g = groups[t.group];
  if (g.amsgrad != 0 && !t.max_exp_avg_sq) return;
  const nqa_adam_clip c = *clip;
  const double step_old = (double)*t.step;
  if (t.dtype == NQA_F64)
    adam_step_typed<double>(t, offset, len, g, c, step_old);
  else
    adam_step_typed<float>(t, offset, len, g, c, step_old);
}

__global__ void adam_advance_kernel(const nqa_adam_tensor* __restrict__ tensors, int64_t tensor_capacity,
                                    const int64_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= tensor_capacity || i >= counts[1]) return;
  const nqa_adam_tensor t = tensors[i];
  if (t.grad && t.step) *t.step += 1.0f;
}

// lane 0 ends with the 64 values added by a fixed tree
__device__ __forceinline__ double adam_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
  return v;
}

template <typename T>
__device__ __forceinline__ double adam_sumsq_chunk(const nqa_adam_tensor& t, int64_t offset, int len) {
  const NQA_GLOBAL T* g = (const NQA_GLOBAL T*)t.grad + offset;
  double sum = 0.0;
  chunk_walk<T, ADAM_WAVE>(len, aligned16(g), [&](int i, auto width) {
    constexpr int N = decltype(width)::value;
    T ge[N];
    pack_load<T, N>(g + i, ge);
#pragma unroll
    for (int j = 0; j < N; ++j) sum += (double)ge[j] * (double)ge[j];
  });
  return sum;
}

__global__ __launch_bounds__(ADAM_WAVE) void adam_sumsq_kernel(const nqa_adam_tensor* __restrict__ tensors,
                                                                const nqa_mt_chunk* __restrict__ chunks,
                                                                const int64_t* __restrict__ counts,
                                                                double* __restrict__ partials) {
  if ((int64_t)blockIdx.x >= counts[0]) return;
  nqa_adam_tensor t;
  int64_t offset;
  int len;
  double sum = 0.0;  // (uniform branches: the whole wavefront reaches the shuffles)
  if (chunk_of<ADAM_CHUNK>(tensors, chunks, counts, t, offset, len) && t.grad)
    sum = t.dtype == NQA_F64 ? adam_sumsq_chunk<double>(t, offset, len) : adam_sumsq_chunk<float>(t, offset, len);
  sum = adam_wave_sum(sum);
  if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

__global__ __launch_bounds__(ADAM_WAVE) void adam_norm_kernel(const double* __restrict__ partials, int64_t chunk_capacity,
                                                               const int64_t* __restrict__ counts,
                                                               nqa_adam_clip* __restrict__ clip) {
  __shared__ double lanes[ADAM_WAVE];
  int64_t n = counts[0];
  if (n > chunk_capacity) n = chunk_capacity;
  if (n < 0) n = 0;
  const int64_t per = (n + ADAM_WAVE - 1) / ADAM_WAVE;
  const int64_t begin = (int64_t)threadIdx.x * per;
  const int64_t end = begin + per < n ? begin + per : n;
  double sum = 0.0;
  for (int64_t i = begin; i < end; ++i) sum += partials[i];
  lanes[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double total = 0.0;
  for (int l = 0; l < ADAM_WAVE; ++l) total += lanes[l];
  const double norm = sqrt(total);
  const double coef = clip->max_norm / (norm + 1e-6);
  clip->norm = norm;
  clip->factor = coef > 1.0 ? 1.0 : coef;  // torch.clamp(coef, max=1.0): a NaN stays
}

static int adam_check(const char* name, const void* tensors, const void* chunks, int64_t chunk_capacity, const void* counts) {
  const int rc = check_tables(name, tensors, chunks, chunk_capacity, counts);
  if (rc != NQA_OK) return rc;
  if (!tensors || !counts) {
    set_error(std::string(name) + ": the tensor table and the counts [chunks in use, tensors in use] are required");
    return NQA_ERR_INVALID;
  }
  return NQA_OK;
}

#pragma clang fp contract(off)

// Python's max(a, b): b if b > a else a
__device__ __forceinline__ double plateau_max(double a, double b) { return b > a ? b : a; }

__global__ void adam_plateau_kernel(const void* __restrict__ metric, int32_t metric_dtype,
                                    nqa_adam_plateau_state* __restrict__ state, nqa_adam_group* __restrict__ groups,
                                    int32_t n_groups) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  nqa_adam_plateau_state s = *state;
  const double current = metric_dtype == NQA_F64 ? *(const double*)metric : (double)*(const float*)metric;
  s.last_epoch += 1;
  bool better;
  if (s.mode_max == 0 && s.threshold_abs == 0) {
    const double rel_epsilon = 1.0 - s.threshold;
    better = current < s.best * rel_epsilon;
  } else if (s.mode_max == 0) {
    better = current < s.best - s.threshold;
  } else if (s.threshold_abs == 0) {
    const double rel_epsilon = s.threshold + 1.0;
    better = current > s.best * rel_epsilon;
  } else {
    better = current > s.best + s.threshold;
  }
  if (better) {
    s.best = current;
    s.num_bad_epochs = 0;
  } else {
    s.num_bad_epochs += 1;
  }
  if (s.cooldown_counter > 0) {
    s.cooldown_counter -= 1;
    s.num_bad_epochs = 0;
  }
  if (s.num_bad_epochs > s.patience) {
    for (int i = 0; i < n_groups; ++i) {
      const double old_lr = groups[i].lr;
      const double new_lr = plateau_max(old_lr * s.factor, groups[i].min_lr);
      if (old_lr - new_lr > s.eps) groups[i].lr = new_lr;
    }
    s.cooldown_counter = s.cooldown;
    s.num_bad_epochs = 0;
  }
  state->best = s.best;
  state->num_bad_epochs = s.num_bad_epochs;
  state->cooldown_counter = s.cooldown_counter;
  state->last_epoch = s.last_epoch;
}

}  // namespace nqa

extern "C" {

int nqa_adam_step(const nqa_adam_tensor* tensors, int64_t tensor_capacity, const nqa_mt_chunk* chunks, int64_t chunk_capacity,
                  const int64_t* counts, const nqa_adam_group* groups, int32_t n_groups, const nqa_adam_clip* clip,
                  nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_adam_step";
  const int rc = adam_check(name, tensors, chunks, chunk_capacity, counts);
  if (rc != NQA_OK) return rc;
  if (n_groups < 1 || !groups || !clip || tensor_capacity < 1 || tensor_capacity > INT32_MAX) {
    set_error(std::string(name) + ": the device records of the parameter groups (n_groups >= 1) and of the clipping are "
                                  "required, 1 <= tensor_capacity < 2^31");
    return NQA_ERR_INVALID;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (chunk_capacity > 0)
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)chunk_capacity), dim3(ADAM_THREADS), 0, s, tensors, chunks, counts, groups,
                       n_groups, clip);
  hipLaunchKernelGGL(adam_advance_kernel, dim3((unsigned)((tensor_capacity + 63) / 64)), dim3(64), 0, s, tensors, tensor_capacity,
                     counts);
  return launch_status(name);
}

int nqa_adam_grad_norm(const nqa_adam_tensor* tensors, const nqa_mt_chunk* chunks, int64_t chunk_capacity, const int64_t* counts,
                       double* partials, nqa_adam_clip* clip, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_adam_grad_norm";
  const int rc = adam_check(name, tensors, chunks, chunk_capacity, counts);
  if (rc != NQA_OK) return rc;
  if (!clip || (chunk_capacity > 0 && !partials)) {
    set_error(std::string(name) + ": partials [chunk_capacity] and the clip record are required");
    return NQA_ERR_INVALID;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (chunk_capacity > 0)
    hipLaunchKernelGGL(adam_sumsq_kernel, dim3((unsigned)chunk_capacity), dim3(ADAM_WAVE), 0, s, tensors, chunks, counts, partials);
  hipLaunchKernelGGL(adam_norm_kernel, dim3(1), dim3(ADAM_WAVE), 0, s, partials, chunk_capacity, counts, clip);
  return launch_status(name);
}

int nqa_adam_plateau(const void* metric, int32_t metric_dtype, nqa_adam_plateau_state* state, nqa_adam_group* groups,
                     int32_t n_groups, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_adam_plateau";
  if (!metric || !state || !groups || n_groups < 1 || (metric_dtype != NQA_F32 && metric_dtype != NQA_F64)) {
    set_error(std::string(name) + ": a float32 or float64 metric in device memory, the scheduler's record and the group records "
                                  "(n_groups >= 1) are required");
    return NQA_ERR_INVALID;
  }
  hipLaunchKernelGGL(adam_plateau_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), metric, metric_dtype, state,
                     groups, n_groups);
  return launch_status(name);
}

}  // extern "C"
