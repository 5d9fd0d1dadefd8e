// Schedule-free AdamW (Defazio et al., "The Road Less Scheduled"; the optimizer the reference's
// nequip/train/schedulefree.py::ScheduleFreeLightningModule is driven with) as multi-tensor launches.
//
// The published optimizer forms the scalars of a step on the host: the step index k, the warm-up factor, the beta2 bias
// correction, the running weight_sum and the interpolation weight c_{k+1} are Python numbers, and a hipGraph captured at step k
// replays step k for ever (the defect ema.hip describes for the EMA warm-up).  Here hyper-parameters AND state of every
// parameter group are a record in device memory and the kernel forms the scalars itself.
//
// Layout: the tensor table and chunk map of multi_tensor.h; a table entry is (parameter, .grad, z, exp_avg_sq, element count,
// dtype, group), and there is one nqa_sfree_group RECORD per parameter group.
//   sfree_step_kernel     every workgroup reads the record of its tensor's group and derives sched, bc2, lr_k, lr_max', weight
//                         and c from the OLD state (pure functions of it: no workgroup depends on another), in double, rounded
//                         once to the tensor's arithmetic type as ATen rounds a Python scalar; then per element
//                           v = b2 v + (1 - b2) g g;  gn = g / (sqrt(v / bc2) + eps) + wd y
//                           y = lerp(y, z, c) + lr_k (b1 (1 - c) - 1) gn;  z = z - lr_k gn          (ATen's lerp)
//                         with z read as y in the first step of a group (k == 0: z may hold anything, NaN included).  A tensor
//                         whose .grad is null is skipped, its state untouched.  .grad is only read.
//   sfree_advance_kernel  one thread per group commits k + 1, weight_sum, lr_max, scheduled_lr.  A SECOND launch on the same
//                         stream, the rule of ema.hip's advance: every workgroup of the step has read the old state before
//                         the single writer of a record starts.  No ticket, no atomics, no fence.
//   sfree_swap_kernel     the mode switch p = lerp(p, z, w): w = 1 - 1 / b1 to the averaged weights x, w = 1 - b1 back to y.
// Plain vector loads and stores, no LDS.  Nothing is read by the host.
//
// The three pow() of a step are formed by every wavefront (a chunk is 4 elements per lane): the exponents that occur by
// default (r == 0, weight_lr_power == 1 or 2) are products, which are what a correctly rounded pow returns for them.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "multi_tensor.h"

namespace nqa {

constexpr int SFREE_CHUNK = NQA_EMA_CHUNK;
constexpr int SFREE_THREADS = 256;
static_assert(sizeof(nqa_sfree_tensor) == 48 && sizeof(nqa_sfree_group) == 96 && sizeof(nqa_mt_chunk) == 16,
              "the host writes these tables as int64 words");
static_assert((SFREE_CHUNK * sizeof(float)) % 16 == 0, "a chunk must keep the 16-byte alignment of its tensor");

__device__ __forceinline__ double sfree_pow(double x, double e) {
  if (e == 0.0) return 1.0;
  if (e == 1.0) return x;
  if (e == 2.0) return x * x;
  return pow(x, e);
}

// the scalars of the step that follows the state in `g`, in double
struct SfreeScalars {
  double bc2, lr_k, lr_max, weight_sum, c;
};

__device__ __forceinline__ SfreeScalars sfree_scalars(const nqa_sfree_group& g) {
  SfreeScalars s;
  const double k1 = (double)(g.k + 1);
  const double sched = g.k < g.warmup_steps ? k1 / (double)g.warmup_steps : 1.0;
  s.bc2 = 1.0 - pow(g.beta2, k1);
  s.lr_k = g.lr * sched;
  s.lr_max = s.lr_k > g.lr_max ? s.lr_k : g.lr_max;
  const double weight = sfree_pow(k1, g.r) * sfree_pow(s.lr_max, g.weight_lr_power);
  s.weight_sum = g.weight_sum + weight;
  s.c = s.weight_sum == 0.0 ? 0.0 : weight / s.weight_sum;
  return s;
}

template <typename T>
struct SfreeStepOp {
  T b2, one_minus_b2, bc2, eps, wd, c, a, lr_k;
  bool first;
  __device__ SfreeStepOp(const nqa_sfree_group& g, const SfreeScalars& s)
      : b2((T)g.beta2), one_minus_b2((T)(1.0 - g.beta2)), bc2((T)s.bc2), eps((T)g.eps), wd((T)g.weight_decay), c((T)s.c),
        a((T)(s.lr_k * (g.beta1 * (1.0 - s.c) - 1.0))), lr_k((T)s.lr_k), first(g.k <= 0) {}
  __device__ __forceinline__ void operator()(T& y, T g, T& z, T& v) const {
    const T z_old = first ? y : z;
    const T v_new = b2 * v + one_minus_b2 * g * g;
    const T gn = g / (sqrt(v_new / bc2) + eps) + wd * y;
    y = lerp(y, z_old, c) + a * gn;
    z = z_old - lr_k * gn;
    v = v_new;
  }
};

// `len` elements at `offset` of the four tensors of one table entry
template <typename T>
__device__ __forceinline__ void sfree_step_chunk(const nqa_sfree_tensor& t, int64_t offset, int len, const SfreeStepOp<T> op) {
  NQA_GLOBAL T* y = (NQA_GLOBAL T*)t.param + offset;
  const NQA_GLOBAL T* g = (const NQA_GLOBAL T*)t.grad + offset;
  NQA_GLOBAL T* z = (NQA_GLOBAL T*)t.z + offset;
  NQA_GLOBAL T* v = (NQA_GLOBAL T*)t.exp_avg_sq + offset;
  chunk_walk<T, SFREE_THREADS>(len, aligned16(y, g, z, v), [&](int i, auto width) {
    constexpr int N = decltype(width)::value;
    T ye[N], ge[N], ze[N], ve[N];
    pack_load<T, N>(y + i, ye);
    pack_load<T, N>(g + i, ge);
    pack_load<T, N>(z + i, ze);
    pack_load<T, N>(v + i, ve);
#pragma unroll
    for (int j = 0; j < N; ++j) op(ye[j], ge[j], ze[j], ve[j]);
    pack_store<T, N>(y + i, ye);
    pack_store<T, N>(z + i, ze);
    pack_store<T, N>(v + i, ve);
  });
}

// p = lerp(p, z, w) over `len` elements
template <typename T>
__device__ __forceinline__ void sfree_swap_chunk(const nqa_sfree_tensor& t, int64_t offset, int len, T w) {
  NQA_GLOBAL T* p = (NQA_GLOBAL T*)t.param + offset;
  const NQA_GLOBAL T* z = (const NQA_GLOBAL T*)t.z + offset;
  chunk_walk<T, SFREE_THREADS>(len, aligned16(p, z), [&](int i, auto width) {
    constexpr int N = decltype(width)::value;
    T pe[N], ze[N];
    pack_load<T, N>(p + i, pe);
    pack_load<T, N>(z + i, ze);
#pragma unroll
    for (int j = 0; j < N; ++j) pe[j] = lerp<T>(pe[j], ze[j], w);
    pack_store<T, N>(p + i, pe);
  });
}

// the chunk of this workgroup: false past the count, for an entry that does not lie inside its tensor, or for a group that is
// not in the table of records
__device__ __forceinline__ bool sfree_chunk_of(const nqa_sfree_tensor* __restrict__ tensors, const nqa_mt_chunk* __restrict__ chunks,
                                               const int64_t* __restrict__ n_chunks, int32_t n_groups, nqa_sfree_tensor& t,
                                               int64_t& offset, int& len) {
  return chunk_of<SFREE_CHUNK>(tensors, chunks, n_chunks, t, offset, len) && t.group >= 0 && t.group < n_groups;
}

__global__ __launch_bounds__(SFREE_THREADS) void sfree_step_kernel(const nqa_sfree_tensor* __restrict__ tensors,
                                                                    const nqa_mt_chunk* __restrict__ chunks,
                                                                    const int64_t* __restrict__ n_chunks,
                                                                    const nqa_sfree_group* __restrict__ groups, int32_t n_groups) {
  nqa_sfree_tensor t;
  int64_t offset;
  int len;
  if (!sfree_chunk_of(tensors, chunks, n_chunks, n_groups, t, offset, len)) return;
  if (!t.grad || !t.z || !t.exp_avg_sq) return;  // (.grad is None: the parameter is skipped)
  const nqa_sfree_group g = groups[t.group];
  const SfreeScalars s = sfree_scalars(g);
  if (t.dtype == NQA_F64)
    sfree_step_chunk<double>(t, offset, len, SfreeStepOp<double>(g, s));
  else
    sfree_step_chunk<float>(t, offset, len, SfreeStepOp<float>(g, s));
}

__global__ void sfree_advance_kernel(nqa_sfree_group* __restrict__ groups, int32_t n_groups) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_groups) return;
  const nqa_sfree_group g = groups[i];
  const SfreeScalars s = sfree_scalars(g);
  groups[i].k = g.k + 1;
  groups[i].weight_sum = s.weight_sum;
  groups[i].lr_max = s.lr_max;
  groups[i].scheduled_lr = s.lr_k;
}

__global__ __launch_bounds__(SFREE_THREADS) void sfree_swap_kernel(const nqa_sfree_tensor* __restrict__ tensors,
                                                                    const nqa_mt_chunk* __restrict__ chunks,
                                                                    const int64_t* __restrict__ n_chunks,
                                                                    const nqa_sfree_group* __restrict__ groups, int32_t n_groups,
                                                                    int32_t to_eval) {
  nqa_sfree_tensor t;
  int64_t offset;
  int len;
  if (!sfree_chunk_of(tensors, chunks, n_chunks, n_groups, t, offset, len)) return;
  if (!t.z) return;
  const double b1 = groups[t.group].beta1;
  const double w = to_eval ? 1.0 - 1.0 / b1 : 1.0 - b1;
  if (t.dtype == NQA_F64)
    sfree_swap_chunk<double>(t, offset, len, w);
  else
    sfree_swap_chunk<float>(t, offset, len, (float)w);
}

static int sfree_check(const char* name, const void* tensors, const void* chunks, int64_t chunk_capacity, const void* n_chunks,
                       const void* groups, int32_t n_groups) {
  const int rc = check_tables(name, tensors, chunks, chunk_capacity, n_chunks);
  if (rc != NQA_OK) return rc;
  if (n_groups < 1 || !groups) {
    set_error(std::string(name) + ": the device records of the parameter groups are required, n_groups >= 1");
    return NQA_ERR_INVALID;
  }
  return NQA_OK;
}

}  // namespace nqa

extern "C" {

int nqa_sfree_step(const nqa_sfree_tensor* tensors, const nqa_mt_chunk* chunks, int64_t chunk_capacity, const int64_t* n_chunks,
                   nqa_sfree_group* groups, int32_t n_groups, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_sfree_step";
  const int rc = sfree_check(name, tensors, chunks, chunk_capacity, n_chunks, groups, n_groups);
  if (rc != NQA_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (chunk_capacity > 0)
    hipLaunchKernelGGL(sfree_step_kernel, dim3((unsigned)chunk_capacity), dim3(SFREE_THREADS), 0, s, tensors, chunks, n_chunks,
                       groups, n_groups);
  hipLaunchKernelGGL(sfree_advance_kernel, dim3((unsigned)((n_groups + 63) / 64)), dim3(64), 0, s, groups, n_groups);
  return launch_status(name);
}

int nqa_sfree_swap(const nqa_sfree_tensor* tensors, const nqa_mt_chunk* chunks, int64_t chunk_capacity, const int64_t* n_chunks,
                   const nqa_sfree_group* groups, int32_t n_groups, int32_t to_eval, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_sfree_swap";
  const int rc = sfree_check(name, tensors, chunks, chunk_capacity, n_chunks, groups, n_groups);
  if (rc != NQA_OK) return rc;
  if (chunk_capacity == 0) return NQA_OK;
  hipLaunchKernelGGL(sfree_swap_kernel, dim3((unsigned)chunk_capacity), dim3(SFREE_THREADS), 0, static_cast<hipStream_t>(stream),
                     tensors, chunks, n_chunks, groups, n_groups, to_eval);
  return launch_status(name);
}

}  // extern "C"
