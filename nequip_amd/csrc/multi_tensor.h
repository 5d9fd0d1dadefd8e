// The multi-tensor chunk layer of ema.hip, schedulefree.hip, adam.hip, config.hip and training_stats.hip (internal; the public side is the
// "multi-tensor chunk layout" section of include/nequip_amd.h).
//
// Layout: a device table of TENSORS (one record per tensor, or per set of tensors of one shape that are walked together:
// pointers, element count, dtype) and a device map of CHUNKS (nqa_mt_chunk: the tensor a chunk belongs to, the element offset at
// which it starts); a chunk is CHUNK elements of one tensor (the last one of a tensor is shorter, a tensor without elements has
// none), and one workgroup takes one chunk.  The number of chunks is read from device memory as well: the grid is the CAPACITY
// of the map and the workgroups past the count return, so that a captured launch stays right when the tables are rewritten in
// place.
// Accesses are 16 bytes per lane where ALL pointers of a chunk are 16-byte aligned (chunks are a multiple of 16 bytes long: that
// is the alignment of the tensors); a tensor that is a view at an odd element offset takes the element-wise path.
// What stands between a rewritten table and an access out of bounds is chunk_span: nothing is read or written through an entry
// that does not lie inside its tensor.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <type_traits>

#include "launch_status.h"

namespace nqa {

// The pointers come out of a device table, so the compiler cannot know that they are global memory: said here, the accesses
// are global_load / global_store and not the flat forms.
#define NQA_GLOBAL __attribute__((address_space(1)))

template <typename T>
using Vec16 = T __attribute__((ext_vector_type(16 / sizeof(T))));

// N consecutive elements: one element, or whole 16-byte accesses at a 16-byte aligned address (one for four floats, two for
// four doubles)
template <typename T, int N>
__device__ __forceinline__ void pack_load(NQA_GLOBAL const T* p, T (&v)[N]) {
  constexpr int PER = 16 / sizeof(T);
  static_assert(N == 1 || N % PER == 0, "one element or whole 16-byte accesses");
  if constexpr (N == 1) {
    v[0] = *p;
  } else {
#pragma unroll
    for (int a = 0; a < N / PER; ++a) {
      const Vec16<T> x = ((NQA_GLOBAL const Vec16<T>*)p)[a];
#pragma unroll
      for (int j = 0; j < PER; ++j) v[a * PER + j] = x[j];
    }
  }
}

template <typename T, int N>
__device__ __forceinline__ void pack_store(NQA_GLOBAL T* p, const T (&v)[N]) {
  constexpr int PER = 16 / sizeof(T);
  static_assert(N == 1 || N % PER == 0, "one element or whole 16-byte accesses");
  if constexpr (N == 1) {
    *p = v[0];
  } else {
#pragma unroll
    for (int a = 0; a < N / PER; ++a) {
      Vec16<T> x;
#pragma unroll
      for (int j = 0; j < PER; ++j) x[j] = v[a * PER + j];
      ((NQA_GLOBAL Vec16<T>*)p)[a] = x;
    }
  }
}

// ATen's lerp
template <typename T>
__device__ __forceinline__ T lerp(T a, T b, T w) {
  const T diff = b - a;
  return w < T(0.5) ? a + w * diff : b - diff * (T(1) - w);
}

// the elements of a chunk entry: false for an entry that does not lie inside its tensor of `numel` elements
template <int CHUNK>
__device__ __forceinline__ bool chunk_span(const nqa_mt_chunk& c, int64_t numel, int64_t& offset, int& len) {
  offset = c.offset;
  const int64_t left = numel - offset;
  if (offset < 0 || left <= 0) return false;
  len = left < CHUNK ? (int)left : CHUNK;
  return true;
}

// the chunk of this workgroup: false past the count, or for an entry that does not lie inside its tensor
template <int CHUNK, typename Tensor>
__device__ __forceinline__ bool chunk_of(const Tensor* __restrict__ tensors, const nqa_mt_chunk* __restrict__ chunks,
                                         const int64_t* __restrict__ n_chunks, Tensor& t, int64_t& offset, int& len) {
  if ((int64_t)blockIdx.x >= *n_chunks) return false;
  const nqa_mt_chunk c = chunks[blockIdx.x];
  t = tensors[c.tensor];
  return chunk_span<CHUNK>(c, t.numel, offset, len);
}

// (the same for the whole workgroup; a null pointer is aligned)
template <typename... P>
__device__ __forceinline__ bool aligned16(P... p) {
  return ((... | (uintptr_t)p) & 15u) == 0;
}

// `f(i, width)` for the `len` elements of a chunk by THREADS lanes: the aligned body in packs of 16 / sizeof(T) elements
// starting at element i, the tail (everything, when not `aligned`) element by element.  `width` is a
// std::integral_constant: the one body of an operation is instantiated at both widths.
template <typename T, int THREADS, typename F>
__device__ __forceinline__ void chunk_walk(int len, bool aligned, F f) {
  constexpr int N = 16 / sizeof(T);
  int done = 0;
  if (aligned) {
    const int n_vec = len / N;
    for (int i = threadIdx.x; i < n_vec; i += THREADS) f(i * N, std::integral_constant<int, N>{});
    done = n_vec * N;
  }
  for (int i = done + threadIdx.x; i < len; i += THREADS) f(i, std::integral_constant<int, 1>{});
}

// counter += 1, one thread: a launch of its own on the stream of the launches that read the counter, so that none of their
// workgroups sees the advanced value
static __global__ void advance_kernel(int64_t* __restrict__ counter) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *counter += 1;
}

inline int check_tables(const char* name, const void* tensors, const void* chunks, int64_t chunk_capacity, const void* n_chunks) {
  if (chunk_capacity < 0 || chunk_capacity > INT32_MAX || (chunk_capacity > 0 && (!tensors || !chunks || !n_chunks))) {
    set_error(std::string(name) + ": device tables (tensors, chunks, chunk count) are required, 0 <= chunk_capacity < 2^31");
    return NQA_ERR_INVALID;
  }
  return NQA_OK;
}

}  // namespace nqa
