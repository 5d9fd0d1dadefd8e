// Per-tensor statistics of weights, gradients and Adam moments (nequip/train/callbacks/training_stats.py::TrainingStatsMonitor)
// as one multi-tensor reduction.
//
// The reference runs 13 reductions per parameter, each a chain of small ATen kernels that ends in `.item()`, and decides on the
// host (`step_count % log_freq`) whether a step logs: captured into the hipGraph of a training step that decision is frozen.
// Here the step count lives in device memory, every workgroup reads it and returns when the step does not log.
//
// Layout: the tensor table and chunk map of multi_tensor.h, with NQA_TSTATS_CHUNK elements per chunk; a table entry is (pointer,
// element count, dtype, transform f = identity | sqrt, the first chunk of the tensor).  counts = [chunks in use, tensors in use]
// is read from device memory: the grids are the CAPACITIES of the map and of the table, the workgroups past the counts return
// without reading anything else.
//   tstats_partial_kernel  one workgroup per chunk.  Every lane folds its elements y = f(x), promoted to double, by Welford
//                          updates into (count, mean, M2, sum of squares, min, max, absmin, absmax); the lanes of a wavefront are
//                          merged by a fixed shuffle tree (wave_merge_ordered, slot_reduce.h), the four wavefronts in wavefront
//                          order (Chan's formula); one workspace row per chunk.
//   tstats_final_kernel    one wavefront per tensor.  Lane b merges a contiguous run of the tensor's chunk rows in ascending
//                          order, the lanes are merged by the same tree (lane l takes lane l + off BEHIND itself, so the chunks
//                          stay in ascending order), lane 0 writes [min, max, mean, std, absmin, absmax, rms, count] and, for
//                          tensor 0, the step at which this table was written.
//   advance_kernel         count += 1, one thread (multi_tensor.h).
// The counter hazard is the one ema.hip describes: no workgroup of a reduce launch may see the advanced count, so the count is
// advanced by a launch of its own on the same stream.
// NaN: minimum and maximum keep a NaN (fmin / fmax would drop it), Welford and the sum of squares carry it: one NaN makes all
// seven statistics of the row NaN, as ATen does.  +-inf without NaN: min, max, absmin, absmax, rms are ATen's; Welford forms
// inf - inf, so mean and std are NaN where ATen's sum may give inf (std is NaN there as well): non-finite either way.
// No floating-point atomics, no allocation, nothing read by the host, a fixed merge order: the same inputs give the same bits.
// LDS: the four wavefront states of the first stage only.
#include <hip/hip_runtime.h>

#include "multi_tensor.h"
#include "slot_reduce.h"

namespace nqa {

constexpr int TS_CHUNK = NQA_TSTATS_CHUNK;
constexpr int TS_THREADS = 256;
constexpr int TS_ROW = 8;  // doubles per workspace row and per table row
static_assert(sizeof(nqa_tstats_tensor) == 32 && sizeof(nqa_mt_chunk) == 16, "the host writes these tables as int64 words");
static_assert((TS_CHUNK * sizeof(float)) % 16 == 0, "a chunk must keep the 16-byte alignment of its tensor");

struct TsAcc {
  double n, mean, m2, ss, mn, mx, amn, amx;  // (n as a double: exact below 2^53)
};

__device__ __forceinline__ TsAcc ts_empty() { return TsAcc{0.0, 0.0, 0.0, 0.0, INFINITY, -INFINITY, INFINITY, -INFINITY}; }

// one more element (Welford)
__device__ __forceinline__ void ts_push(TsAcc& a, double y) {
  a.n += 1.0;
  const double d = y - a.mean;
  a.mean += d / a.n;
  a.m2 += d * (y - a.mean);
  a.ss += y * y;
  const double ay = fabs(y);
  a.mn = sr_nanmin(a.mn, y);
  a.mx = sr_nanmax(a.mx, y);
  a.amn = sr_nanmin(a.amn, ay);
  a.amx = sr_nanmax(a.amx, ay);
}

// a followed by b (Chan); an empty side leaves the other one bit for bit
__device__ __forceinline__ TsAcc ts_merge(const TsAcc& a, const TsAcc& b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  TsAcc r;
  r.n = a.n + b.n;
  const double delta = b.mean - a.mean;
  const double w = b.n / r.n;
  r.mean = a.mean + delta * w;
  r.m2 = a.m2 + b.m2 + delta * delta * (a.n * w);
  r.ss = a.ss + b.ss;
  r.mn = sr_nanmin(a.mn, b.mn);
  r.mx = sr_nanmax(a.mx, b.mx);
  r.amn = sr_nanmin(a.amn, b.amn);
  r.amx = sr_nanmax(a.amx, b.amx);
  return r;
}

__device__ __forceinline__ void ts_store(double* __restrict__ row, const TsAcc& v) {
  row[0] = v.n;
  row[1] = v.mean;
  row[2] = v.m2;
  row[3] = v.ss;
  row[4] = v.mn;
  row[5] = v.mx;
  row[6] = v.amn;
  row[7] = v.amx;
}

__device__ __forceinline__ TsAcc ts_load(const double* __restrict__ row) {
  return TsAcc{row[0], row[1], row[2], row[3], row[4], row[5], row[6], row[7]};
}

// the elements of one chunk that this lane owns, folded in index order.  The loops of chunk_walk (multi_tensor.h) are written in
// place here: through the walker the same instructions come out with another register allocation (62 VGPRs for 61), and the
// captured logging step measured 0.4 us of 46 slower.
template <typename T, bool SQRT>
__device__ __forceinline__ TsAcc ts_chunk_fold(const void* data, int64_t offset, int len) {
  constexpr int N = 16 / sizeof(T);
  const NQA_GLOBAL T* x = (const NQA_GLOBAL T*)data + offset;
  TsAcc acc = ts_empty();
  auto fold = [&](int i, auto width) {
    constexpr int W = decltype(width)::value;
    T v[W];
    pack_load<T, W>(x + i, v);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const double y = (double)v[j];
      ts_push(acc, SQRT ? sqrt(y) : y);
    }
  };
  int done = 0;
  if (aligned16(x)) {
    const int n_vec = len / N;
    for (int i = threadIdx.x; i < n_vec; i += TS_THREADS) fold(i * N, std::integral_constant<int, N>{});
    done = n_vec * N;
  }
  for (int i = done + threadIdx.x; i < len; i += TS_THREADS) fold(i, std::integral_constant<int, 1>{});
  return acc;
}

__device__ __forceinline__ bool ts_logs(const int64_t* __restrict__ counter, int64_t log_freq, int64_t& count) {
  count = *counter;
  return count >= 0 && count % log_freq == 0;
}

__global__ __launch_bounds__(TS_THREADS) void tstats_partial_kernel(const nqa_tstats_tensor* __restrict__ tensors,
                                                                     const nqa_mt_chunk* __restrict__ chunks,
                                                                     const int64_t* __restrict__ counts,
                                                                     const int64_t* __restrict__ counter, int64_t log_freq,
                                                                     double* __restrict__ workspace) {
  __shared__ double waves[TS_THREADS / 64][TS_ROW];
  int64_t count;
  if (!ts_logs(counter, log_freq, count)) return;  // (uniform: the whole workgroup leaves before any barrier)
  if ((int64_t)blockIdx.x >= counts[0]) return;
  double* __restrict__ row = workspace + (int64_t)blockIdx.x * TS_ROW;
  const nqa_mt_chunk c = chunks[blockIdx.x];
  TsAcc acc = ts_empty();
  // an entry that does not lie inside a tensor in use leaves an empty row
  if (c.tensor >= 0 && (int64_t)c.tensor < counts[1]) {
    const nqa_tstats_tensor t = tensors[c.tensor];
    int64_t offset;
    int len;
    if (chunk_span<TS_CHUNK>(c, t.numel, offset, len)) {
      const bool root = t.transform == NQA_TSTATS_SQRT;
      if (t.dtype == NQA_F64)
        acc = root ? ts_chunk_fold<double, true>(t.data, offset, len) : ts_chunk_fold<double, false>(t.data, offset, len);
      else
        acc = root ? ts_chunk_fold<float, true>(t.data, offset, len) : ts_chunk_fold<float, false>(t.data, offset, len);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  acc = wave_merge_ordered(acc, lane, ts_merge);
  if (lane == 0) ts_store(waves[wave], acc);
  __syncthreads();
  if (threadIdx.x == 0) {
    TsAcc v = ts_load(waves[0]);
#pragma unroll
    for (int k = 1; k < TS_THREADS / 64; ++k) v = ts_merge(v, ts_load(waves[k]));
    ts_store(row, v);
  }
}

__global__ __launch_bounds__(64) void tstats_final_kernel(const nqa_tstats_tensor* __restrict__ tensors,
                                                          const int64_t* __restrict__ counts,
                                                          const int64_t* __restrict__ counter, int64_t log_freq,
                                                          const double* __restrict__ workspace, double* __restrict__ table,
                                                          int64_t* __restrict__ stamp) {
  int64_t count;
  if (!ts_logs(counter, log_freq, count)) return;
  if ((int64_t)blockIdx.x >= counts[1]) return;
  const nqa_tstats_tensor t = tensors[blockIdx.x];
  const int lane = threadIdx.x;
  if (blockIdx.x == 0 && lane == 0) *stamp = count;
  if (t.numel <= 0) return;
  const int64_t n_chunks = (t.numel + TS_CHUNK - 1) / TS_CHUNK;
  if (t.chunk0 < 0 || (int64_t)t.chunk0 + n_chunks > counts[0]) return;  // rows that were not written: nothing is read
  const int64_t per = (n_chunks + 63) / 64;
  const int64_t lo = lane * per, hi = lo + per < n_chunks ? lo + per : n_chunks;
  TsAcc v = ts_empty();
  for (int64_t k = lo; k < hi; ++k) v = ts_merge(v, ts_load(workspace + ((int64_t)t.chunk0 + k) * TS_ROW));
  v = wave_merge_ordered(v, lane, ts_merge);
  if (lane != 0) return;
  double* __restrict__ out = table + (int64_t)blockIdx.x * TS_ROW;
  out[0] = v.mn;
  out[1] = v.mx;
  out[2] = v.mean;
  out[3] = sqrt(v.m2 / (v.n - 1.0));  // unbiased; one element: 0 / 0
  out[4] = v.amn;
  out[5] = v.amx;
  out[6] = sqrt(v.ss / v.n);
  out[7] = v.n;
}

}  // namespace nqa

extern "C" {

int32_t nqa_tstats_chunk_elems(void) { return nqa::TS_CHUNK; }

int nqa_tstats_reduce(const nqa_tstats_tensor* tensors, int64_t tensor_capacity, const nqa_mt_chunk* chunks,
                      int64_t chunk_capacity, const int64_t* counts, const int64_t* counter, int64_t log_freq, double* workspace,
                      double* table, int64_t* stamp, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_tstats_reduce";
  if (tensor_capacity < 0 || tensor_capacity > INT32_MAX || chunk_capacity < 0 || chunk_capacity > INT32_MAX || log_freq < 1) {
    set_error(std::string(name) + ": 0 <= tensor_capacity, chunk_capacity < 2^31 and log_freq >= 1");
    return NQA_ERR_INVALID;
  }
  if (tensor_capacity == 0 || chunk_capacity == 0) return NQA_OK;
  if (!tensors || !chunks || !counts || !counter || !workspace || !table || !stamp) {
    set_error(std::string(name) + ": device tables (tensors, chunks, counts), counter, workspace, table and stamp are required");
    return NQA_ERR_INVALID;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(tstats_partial_kernel, dim3((unsigned)chunk_capacity), dim3(TS_THREADS), 0, s, tensors, chunks, counts,
                     counter, log_freq, workspace);
  hipLaunchKernelGGL(tstats_final_kernel, dim3((unsigned)tensor_capacity), dim3(64), 0, s, tensors, counts, counter, log_freq,
                     workspace, table, stamp);
  return launch_status(name);
}

int nqa_tstats_advance(int64_t* counter, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_tstats_advance";
  if (!counter) {
    set_error(std::string(name) + ": the device counter is required");
    return NQA_ERR_INVALID;
  }
  hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), counter);
  return launch_status(name);
}

}  // extern "C"
