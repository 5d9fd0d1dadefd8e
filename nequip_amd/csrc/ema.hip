// Exponential moving average of the model weights (nequip/train/ema.py::EMAWeights) as multi-tensor launches.
//
// The reference forms the decay of a step on the host, d = min(decay, (1 + n) / (10 + n)) with n the number of updates so
// far, and hands 1 - d to torch._foreach_lerp_ as a Python scalar: captured into the hipGraph of a training step that scalar
// is frozen, and every replay averages with the warm-up weight of the capture step.  Here n lives in device memory and the
// kernel forms the weight itself.
//
// Layout: the tensor table and chunk map of multi_tensor.h; a table entry is an (EMA pointer, parameter pointer) pair.
//   ema_update_kernel   n == 0: ema = param (the buffers may hold anything, NaN included).  Otherwise w = 1 - d in double,
//                       rounded to the tensor's arithmetic type (float / double, as ATen rounds a Python scalar), and
//                       ATen's lerp: w < 0.5 ? a + w (b - a) : b - (b - a) (1 - w).
//   advance_kernel      n += 1, one thread (multi_tensor.h).
//   ema_swap_kernel     every element pair is loaded and stored crosswise by the same lane: bit-exact, no temporary.
// The counter hazard: no workgroup of ema_update_kernel may see the advanced n.  The counter is therefore advanced by a SECOND
// launch on the same stream, not by the workgroups of the first: launches of one stream run in order (in a captured graph
// they become two kernel nodes joined by an edge), so every workgroup of the update has finished reading n before the single
// writer starts, and the next update's workgroups start after it.  No ticket, no atomics, no fence.
// No LDS.  Nothing is read by the host.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "multi_tensor.h"

namespace nqa {

constexpr int EMA_CHUNK = NQA_EMA_CHUNK;
constexpr int EMA_THREADS = 256;
static_assert(sizeof(nqa_ema_tensor) == 32 && sizeof(nqa_mt_chunk) == 16, "the host writes these tables as int64 words");
static_assert((EMA_CHUNK * sizeof(float)) % 16 == 0, "a chunk must keep the 16-byte alignment of its tensor");

template <typename T>
struct EmaUpdateOp {
  static constexpr bool writes_param = false;
  T w;
  bool copy;
  __device__ __forceinline__ void operator()(T& a, T& b) const { a = copy ? b : lerp(a, b, w); }
};

template <typename T>
struct EmaSwapOp {
  static constexpr bool writes_param = true;
  __device__ __forceinline__ void operator()(T& a, T& b) const {
    const T t = a;
    a = b;
    b = t;
  }
};

// `op(a, b)` rewrites one element pair in registers; `len` elements at `ema` / `param`
template <typename T, typename Op>
__device__ __forceinline__ void ema_chunk_apply(void* ema, void* param, int64_t offset, int len, Op op) {
  NQA_GLOBAL T* a = (NQA_GLOBAL T*)ema + offset;
  NQA_GLOBAL T* b = (NQA_GLOBAL T*)param + offset;
  chunk_walk<T, EMA_THREADS>(len, aligned16(a, b), [&](int i, auto width) {
    constexpr int N = decltype(width)::value;
    T x[N], y[N];
    pack_load<T, N>(a + i, x);
    pack_load<T, N>(b + i, y);
#pragma unroll
    for (int j = 0; j < N; ++j) op(x[j], y[j]);
    pack_store<T, N>(a + i, x);
    if (Op::writes_param) pack_store<T, N>(b + i, y);
  });
}

__global__ __launch_bounds__(EMA_THREADS) void ema_update_kernel(const nqa_ema_tensor* __restrict__ tensors,
                                                                  const nqa_mt_chunk* __restrict__ chunks,
                                                                  const int64_t* __restrict__ n_chunks,
                                                                  const int64_t* __restrict__ counter, double decay) {
  nqa_ema_tensor t;
  int64_t offset;
  int len;
  if (!chunk_of<EMA_CHUNK>(tensors, chunks, n_chunks, t, offset, len)) return;
  const int64_t n = *counter;
  const bool copy = n <= 0;
  const double warm = (1.0 + (double)n) / (10.0 + (double)n);
  const double w = 1.0 - (decay < warm ? decay : warm);
  if (t.dtype == NQA_F64)
    ema_chunk_apply<double>(t.ema, t.param, offset, len, EmaUpdateOp<double>{w, copy});
  else
    ema_chunk_apply<float>(t.ema, t.param, offset, len, EmaUpdateOp<float>{(float)w, copy});
}

__global__ __launch_bounds__(EMA_THREADS) void ema_swap_kernel(const nqa_ema_tensor* __restrict__ tensors,
                                                                const nqa_mt_chunk* __restrict__ chunks,
                                                                const int64_t* __restrict__ n_chunks) {
  nqa_ema_tensor t;
  int64_t offset;
  int len;
  if (!chunk_of<EMA_CHUNK>(tensors, chunks, n_chunks, t, offset, len)) return;
  if (t.dtype == NQA_F64)
    ema_chunk_apply<double>(t.ema, t.param, offset, len, EmaSwapOp<double>{});
  else
    ema_chunk_apply<float>(t.ema, t.param, offset, len, EmaSwapOp<float>{});
}

}  // namespace nqa

extern "C" {

int32_t nqa_ema_chunk_elems(void) { return nqa::EMA_CHUNK; }

int nqa_ema_update(const nqa_ema_tensor* tensors, const nqa_mt_chunk* chunks, int64_t chunk_capacity, const int64_t* n_chunks,
                   double decay, int64_t* counter, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_ema_update";
  const int rc = check_tables(name, tensors, chunks, chunk_capacity, n_chunks);
  if (rc != NQA_OK) return rc;
  if (!counter || !(decay >= 0.0 && decay <= 1.0)) {
    set_error(std::string(name) + ": the device counter is required, and a decay in [0, 1]");
    return NQA_ERR_INVALID;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (chunk_capacity > 0)
    hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)chunk_capacity), dim3(EMA_THREADS), 0, s, tensors, chunks, n_chunks,
                       counter, decay);
  hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(1), 0, s, counter);
  return launch_status(name);
}

int nqa_ema_swap(const nqa_ema_tensor* tensors, const nqa_mt_chunk* chunks, int64_t chunk_capacity, const int64_t* n_chunks,
                 nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_ema_swap";
  const int rc = check_tables(name, tensors, chunks, chunk_capacity, n_chunks);
  if (rc != NQA_OK) return rc;
  if (chunk_capacity == 0) return NQA_OK;
  hipLaunchKernelGGL(ema_swap_kernel, dim3((unsigned)chunk_capacity), dim3(EMA_THREADS), 0, static_cast<hipStream_t>(stream),
                     tensors, chunks, n_chunks);
  return launch_status(name);
}

}  // extern "C"
