// Exponential moving average of the model weights (nequip/train/ema.py::EMAWeights) as multi-tensor launches.
//
// The reference forms the decay of a step on the host, d = min(decay, (1 + n) / (10 + n)) with n the number of updates so
// far, and hands 1 - d to torch._foreach_lerp_ as a Python scalar: captured into the hipGraph of a training step that scalar
// is frozen, and every replay averages with the warm-up weight of the capture step.  Here n lives in device memory and the
// kernel forms the weight itself.
//
// Layout: a device table of TENSORS (EMA pointer, parameter pointer, element count, dtype) and a device map of CHUNKS (the
// tensor a chunk belongs to, the element offset at which it starts); a chunk is NQA_EMA_CHUNK elements of one tensor (the
// last one of a tensor is shorter), and one workgroup takes one chunk.  The number of chunks is read from device memory as
// well: the grid is the CAPACITY of the map and the workgroups past the count return, so that a captured launch stays right
// when the tables are rewritten in place.
//   ema_update_kernel   n == 0: ema = param (the buffers may hold anything, NaN included).  Otherwise w = 1 - d in double,
//                       rounded to the tensor's arithmetic type (float / double, as ATen rounds a Python scalar), and
//                       ATen's lerp: w < 0.5 ? a + w (b - a) : b - (b - a) (1 - w).
//   ema_advance_kernel  n += 1, one thread.
//   ema_swap_kernel     every element pair is loaded and stored crosswise by the same lane: bit-exact, no temporary.
// The counter hazard: no workgroup of ema_update_kernel may see the advanced n.  The counter is therefore advanced by a SECOND
// launch on the same stream, not by the workgroups of the first: launches of one stream run in order (in a captured graph
// they become two kernel nodes joined by an edge), so every workgroup of the update has finished reading n before the single
// writer starts, and the next update's workgroups start after it.  No ticket, no atomics, no fence.
// Accesses are 16 bytes per lane where BOTH pointers of a chunk are 16-byte aligned (chunks are a multiple of 16 bytes long:
// that is the alignment of the two tensors); a parameter that is a view at an odd element offset takes the element-wise
// path.  No LDS.  Nothing is read by the host.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "plan.h"

namespace nqa {

constexpr int EMA_CHUNK = NQA_EMA_CHUNK;
constexpr int EMA_THREADS = 256;
static_assert(sizeof(nqa_ema_tensor) == 32 && sizeof(nqa_ema_chunk) == 16, "the host writes these tables as int64 words");
static_assert((EMA_CHUNK * sizeof(float)) % 16 == 0, "a chunk must keep the 16-byte alignment of its tensor");

// The pointers come out of a device table, so the compiler cannot know that they are global memory: said here, the accesses
// are global_load / global_store and not the flat forms.
#define NQA_GLOBAL __attribute__((address_space(1)))

template <typename T>
struct EmaVec;
template <>
struct EmaVec<float> {
  typedef float type __attribute__((ext_vector_type(4)));
  static constexpr int N = 4;
};
template <>
struct EmaVec<double> {
  typedef double type __attribute__((ext_vector_type(2)));
  static constexpr int N = 2;
};

template <typename T>
__device__ __forceinline__ T ema_lerp(T a, T b, T w) {
  const T diff = b - a;
  return w < T(0.5) ? a + w * diff : b - diff * (T(1) - w);
}

template <typename T>
struct EmaUpdateOp {
  static constexpr bool writes_param = false;
  T w;
  bool copy;
  __device__ __forceinline__ void operator()(T& a, T& b) const { a = copy ? b : ema_lerp(a, b, w); }
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
  using V = typename EmaVec<T>::type;
  constexpr int N = EmaVec<T>::N;
  NQA_GLOBAL T* a = (NQA_GLOBAL T*)ema + offset;
  NQA_GLOBAL T* b = (NQA_GLOBAL T*)param + offset;
  const bool aligned = (((uintptr_t)a | (uintptr_t)b) & 15u) == 0;  // (the same for the whole workgroup)
  int done = 0;
  if (aligned) {
    const int n_vec = len / N;
    NQA_GLOBAL V* av = (NQA_GLOBAL V*)a;
    NQA_GLOBAL V* bv = (NQA_GLOBAL V*)b;
    for (int i = threadIdx.x; i < n_vec; i += EMA_THREADS) {
      V x = av[i], y = bv[i];
#pragma unroll
      for (int j = 0; j < N; ++j) {
        T xe = x[j], ye = y[j];
        op(xe, ye);
        x[j] = xe;
        y[j] = ye;
      }
      av[i] = x;
      if (Op::writes_param) bv[i] = y;
    }
    done = n_vec * N;
  }
  for (int i = done + threadIdx.x; i < len; i += EMA_THREADS) {
    T x = a[i], y = b[i];
    op(x, y);
    a[i] = x;
    if (Op::writes_param) b[i] = y;
  }
}

// the chunk of this workgroup: false past the count, or for an entry that does not lie inside its tensor
__device__ __forceinline__ bool ema_chunk_of(const nqa_ema_tensor* __restrict__ tensors, const nqa_ema_chunk* __restrict__ chunks,
                                             const int64_t* __restrict__ n_chunks, nqa_ema_tensor& t, int64_t& offset, int& len) {
  if ((int64_t)blockIdx.x >= *n_chunks) return false;
  const nqa_ema_chunk c = chunks[blockIdx.x];
  t = tensors[c.tensor];
  offset = c.offset;
  const int64_t left = t.numel - offset;
  if (offset < 0 || left <= 0) return false;
  len = left < EMA_CHUNK ? (int)left : EMA_CHUNK;
  return true;
}

__global__ __launch_bounds__(EMA_THREADS) void ema_update_kernel(const nqa_ema_tensor* __restrict__ tensors,
                                                                  const nqa_ema_chunk* __restrict__ chunks,
                                                                  const int64_t* __restrict__ n_chunks,
                                                                  const int64_t* __restrict__ counter, double decay) {
  nqa_ema_tensor t;
  int64_t offset;
  int len;
  if (!ema_chunk_of(tensors, chunks, n_chunks, t, offset, len)) return;
  const int64_t n = *counter;
  const bool copy = n <= 0;
  const double warm = (1.0 + (double)n) / (10.0 + (double)n);
  const double w = 1.0 - (decay < warm ? decay : warm);
  if (t.dtype == NQA_F64)
    ema_chunk_apply<double>(t.ema, t.param, offset, len, EmaUpdateOp<double>{w, copy});
  else
    ema_chunk_apply<float>(t.ema, t.param, offset, len, EmaUpdateOp<float>{(float)w, copy});
}

__global__ void ema_advance_kernel(int64_t* __restrict__ counter) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *counter += 1;
}

__global__ __launch_bounds__(EMA_THREADS) void ema_swap_kernel(const nqa_ema_tensor* __restrict__ tensors,
                                                                const nqa_ema_chunk* __restrict__ chunks,
                                                                const int64_t* __restrict__ n_chunks) {
  nqa_ema_tensor t;
  int64_t offset;
  int len;
  if (!ema_chunk_of(tensors, chunks, n_chunks, t, offset, len)) return;
  if (t.dtype == NQA_F64)
    ema_chunk_apply<double>(t.ema, t.param, offset, len, EmaSwapOp<double>{});
  else
    ema_chunk_apply<float>(t.ema, t.param, offset, len, EmaSwapOp<float>{});
}

static int ema_check(const char* name, const void* tensors, const void* chunks, int64_t chunk_capacity, const void* n_chunks) {
  if (chunk_capacity < 0 || chunk_capacity > INT32_MAX || (chunk_capacity > 0 && (!tensors || !chunks || !n_chunks))) {
    set_error(std::string(name) + ": device tables (tensors, chunks, chunk count) are required, 0 <= chunk_capacity < 2^31");
    return NQA_ERR_INVALID;
  }
  return NQA_OK;
}

static int ema_launch_status(const char* name) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error(std::string(name) + ": " + hipGetErrorString(e));
    return NQA_ERR_LAUNCH;
  }
  return NQA_OK;
}

}  // namespace nqa

extern "C" {

int32_t nqa_ema_chunk_elems(void) { return nqa::EMA_CHUNK; }

int nqa_ema_update(const nqa_ema_tensor* tensors, const nqa_ema_chunk* chunks, int64_t chunk_capacity, const int64_t* n_chunks,
                   double decay, int64_t* counter, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_ema_update";
  const int rc = ema_check(name, tensors, chunks, chunk_capacity, n_chunks);
  if (rc != NQA_OK) return rc;
  if (!counter || !(decay >= 0.0 && decay <= 1.0)) {
    set_error(std::string(name) + ": the device counter is required, and a decay in [0, 1]");
    return NQA_ERR_INVALID;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (chunk_capacity > 0)
    hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)chunk_capacity), dim3(EMA_THREADS), 0, s, tensors, chunks, n_chunks,
                       counter, decay);
  hipLaunchKernelGGL(ema_advance_kernel, dim3(1), dim3(1), 0, s, counter);
  return ema_launch_status(name);
}

int nqa_ema_swap(const nqa_ema_tensor* tensors, const nqa_ema_chunk* chunks, int64_t chunk_capacity, const int64_t* n_chunks,
                 nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_ema_swap";
  const int rc = ema_check(name, tensors, chunks, chunk_capacity, n_chunks);
  if (rc != NQA_OK) return rc;
  if (chunk_capacity == 0) return NQA_OK;
  hipLaunchKernelGGL(ema_swap_kernel, dim3((unsigned)chunk_capacity), dim3(EMA_THREADS), 0, static_cast<hipStream_t>(stream),
                     tensors, chunks, n_chunks);
  return ema_launch_status(name);
}

}  // extern "C"
