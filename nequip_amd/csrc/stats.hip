// Dataset statistics on one fused reduction (nequip/data/stats_manager.py::DataStatisticsManager.forward, the metric classes of
// nequip/data/stats.py, nequip/data/modifier.py::NumNeighbors).
//
// The reference updates every entry on its own: one boolean-index selection per atom type (T^2 for edge fields),
// `masked_select` for NaNs, `torch.unique` for the neighbour counts and `torch.is_nonzero` on the running count -- a host
// synchronisation with data-dependent shapes each.  Here a STREAM is one distinct field tensor, a TERM one entry on a stream and
// a SLOT one group of a term (1, T for a per-type node term, T^2 for a per-type edge term).  Every slot keeps the same state
//   count (int64), mean, mean_lo, M2 = sum (y - mean)^2, min, max (float64)     of y = m(x), m = identity | abs | square,
// and every metric kind is formed from it on the host (mean, sqrt(mean), M2 / (count - 1), min, max, count).  The mean is the
// unevaluated sum mean + mean_lo: `mean` is a pivot near the data (the first element an owner sees; after a merge the rounded
// mean) and `mean_lo` the running mean of y - pivot, so that the difference of two means, which Chan's merge squares, is
// formed from small numbers -- with one double, means of 1e6 carry an error of 1e-10 each and a spread of 1e-2 leaves the
// merged M2 with nine digits.  Per batch:
//   stats_partial_kernel   NQA_STATS_GROUPS workgroups walk every stream once (grid stride, elements promoted to float64, the
//                          group index formed from atom_types / edge_index in the kernel) and leave one row of per-slot partial
//                          states each.  A sweep stages 256 elements and their group in LDS; PARTS owner threads per slot fold
//                          their share of the sweep in element order by Welford updates; the parts are merged in part order by
//                          Chan's formula.
//   stats_final_kernel     one wavefront per slot: lane b merges rows 4b .. 4b+3 in row order, the lanes are merged by a fixed
//                          shuffle tree, lane 0 merges the batch into the running state (a batch without an element for the
//                          slot leaves it untouched).
//   neighbor_count_kernel  counts edge_index[0] into a zeroed [N] int32 workspace (integer atomics: exact, order-independent),
//                          which the first kernel then reads as an integer stream.
// No floating-point atomics and a fixed merge order: two runs over the same batches give bit-identical state.  No sum of
// squares is ever differenced: the variance of total energies (1e5 with a spread of 1e-1) keeps its digits.  Nothing is read by
// the host, so an update captures into a hipGraph.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "launch_status.h"

namespace nqa {

constexpr int ST_MAX_STREAMS = NQA_STATS_MAX_STREAMS;
constexpr int ST_MAX_TERMS = NQA_STATS_MAX_TERMS;
constexpr int ST_MAX_SLOTS = NQA_STATS_MAX_SLOTS;
constexpr int ST_GROUPS = NQA_STATS_GROUPS;
constexpr int ST_MAX_PARTS = 16;  // owners per slot while the slots of a stream are few (halved until parts * slots <= 256)
static_assert(sizeof(nqa_stats_stream) == 64 && sizeof(nqa_stats_term) == 32, "mirrored by ctypes structures");
static_assert(ST_GROUPS % 64 == 0 && ST_GROUPS >= 64, "the second stage gives every lane the same number of rows");

struct StAcc {
  long long n;
  double hi, lo, m2, mn, mx;  // mean = hi + lo
};

// minimum / maximum that keep a NaN (torch.minimum / torch.maximum do)
__device__ __forceinline__ double st_nanmin(double a, double b) { return (a != a || b != b) ? (a + b) : fmin(a, b); }
__device__ __forceinline__ double st_nanmax(double a, double b) { return (a != a || b != b) ? (a + b) : fmax(a, b); }

__device__ __forceinline__ StAcc st_empty() { return StAcc{0, 0.0, 0.0, 0.0, INFINITY, -INFINITY}; }

// one more element (Welford on y - pivot; the first element is the pivot)
__device__ __forceinline__ void st_push(StAcc& a, double y) {
  if (a.n == 0) a.hi = y;
  a.n += 1;
  const double z = y - a.hi;
  const double d = z - a.lo;
  a.lo += d / (double)a.n;
  a.m2 += d * (z - a.lo);
  a.mn = st_nanmin(a.mn, y);
  a.mx = st_nanmax(a.mx, y);
}

// hi + lo again, with hi the rounded sum and lo what the rounding lost (Knuth's two-sum; a sum that is not finite keeps no
// remainder, so that an infinite mean stays infinite)
__device__ __forceinline__ void st_renorm(double& hi, double& lo) {
  const double s = hi + lo;
  const double b = s - hi;
  const double e = (hi - (s - b)) + (lo - b);
  hi = s;
  lo = (fabs(s) <= 1.7976931348623157e308) ? e : 0.0;
}

// a followed by b (Chan); an empty side leaves the other one bit for bit
__device__ __forceinline__ StAcc st_merge(const StAcc& a, const StAcc& b) {
  if (b.n == 0) return a;
  if (a.n == 0) return b;
  StAcc r;
  r.n = a.n + b.n;
  const double delta = (b.hi - a.hi) + (b.lo - a.lo);
  const double change = delta * ((double)b.n / (double)r.n);
  r.hi = a.hi;
  r.lo = a.lo + change;
  st_renorm(r.hi, r.lo);
  r.m2 = a.m2 + b.m2 + delta * change * (double)a.n;
  r.mn = st_nanmin(a.mn, b.mn);
  r.mx = st_nanmax(a.mx, b.mx);
  return r;
}

struct StatsArgs {
  nqa_stats_stream st[ST_MAX_STREAMS];
  nqa_stats_term terms[ST_MAX_TERMS];                               // ordered by stream
  int32_t term_begin[ST_MAX_STREAMS], term_count[ST_MAX_STREAMS];  // the terms of a stream are contiguous in the table
  int32_t slot_begin[ST_MAX_STREAMS], slot_count[ST_MAX_STREAMS];  // ... and so are their slots
  int32_t parts[ST_MAX_STREAMS];                                   // owners per slot
  int32_t n_streams, n_terms, n_slots;
  int32_t amax, lmax;  // most (parts * slots) / slots of one stream: the LDS layout
};

__device__ __forceinline__ double st_load(const void* __restrict__ p, int dtype, int64_t i) {
  switch (dtype) {
    case NQA_STATS_F32:
      return (double)static_cast<const float*>(p)[i];
    case NQA_STATS_F64:
      return static_cast<const double*>(p)[i];
    case NQA_STATS_I32:
      return (double)static_cast<const int32_t*>(p)[i];
    default:
      return (double)static_cast<const int64_t*>(p)[i];
  }
}

// the group of a row: -1 outside every per-type term's groups (such a row still enters the plain terms)
__device__ __forceinline__ int st_group(const nqa_stats_stream& st, int64_t row) {
  if (st.group_kind == NQA_STATS_GROUP_NODE) {
    const int64_t t = st.atom_types[row];
    return (t >= 0 && t < st.num_types) ? (int)t : -1;
  }
  if (st.group_kind == NQA_STATS_GROUP_EDGE) {
    const int64_t c = st.edge_index[row], nb = st.edge_index[st.rows + row];
    if (c < 0 || c >= st.num_atoms || nb < 0 || nb >= st.num_atoms) return -1;
    const int64_t tc = st.atom_types[c], tn = st.atom_types[nb];
    if (tc < 0 || tc >= st.num_types || tn < 0 || tn >= st.num_types) return -1;
    return (int)(tc * st.num_types + tn);
  }
  return 0;
}

__device__ __forceinline__ double st_modify(int mod, double x) {
  return mod == NQA_STATS_MOD_ABS ? fabs(x) : (mod == NQA_STATS_MOD_SQUARE ? x * x : x);
}

// ---- first stage ------------------------------------------------------------------------------------------------------------
// LDS: xs [256] float64 and grp [256] int32 (the sweep: -2 marks a lane past the end), the owners' accumulators [amax] x
// (count, mean, mean_lo, M2, min, max) -- one writing thread per entry --, slot_term / slot_group [lmax].
constexpr int ST_NO_ELEMENT = -2;

__global__ __launch_bounds__(256) void stats_partial_kernel(const StatsArgs a, long long* __restrict__ part_n,
                                                            double* __restrict__ part_hi, double* __restrict__ part_lo,
                                                            double* __restrict__ part_m2, double* __restrict__ part_min,
                                                            double* __restrict__ part_max) {
  extern __shared__ __attribute__((aligned(16))) char st_smem[];
  double* __restrict__ xs = reinterpret_cast<double*>(st_smem);
  long long* __restrict__ acc_n = reinterpret_cast<long long*>(xs + 256);
  double* __restrict__ acc_hi = reinterpret_cast<double*>(acc_n + a.amax);
  double* __restrict__ acc_lo = acc_hi + a.amax;
  double* __restrict__ acc_m2 = acc_lo + a.amax;
  double* __restrict__ acc_min = acc_m2 + a.amax;
  double* __restrict__ acc_max = acc_min + a.amax;
  int32_t* __restrict__ slot_term = reinterpret_cast<int32_t*>(acc_max + a.amax);
  int32_t* __restrict__ slot_group = slot_term + a.lmax;
  int32_t* __restrict__ grp = slot_group + a.lmax;
  const int tid = threadIdx.x;

  for (int s = 0; s < a.n_streams; ++s) {
    const nqa_stats_stream& st = a.st[s];
    const int tb = a.term_begin[s], tc = a.term_count[s], sb = a.slot_begin[s], sc = a.slot_count[s];
    const int parts = a.parts[s], share = 256 / parts;
    for (int k = tid; k < tc; k += 256) {
      const nqa_stats_term& t = a.terms[tb + k];
      for (int g = 0; g < t.n_groups; ++g) {
        slot_term[t.slot0 - sb + g] = k;
        slot_group[t.slot0 - sb + g] = g;
      }
    }
    for (int o = tid; o < parts * sc; o += 256) {
      acc_n[o] = 0;
      acc_hi[o] = 0.0;
      acc_lo[o] = 0.0;
      acc_m2[o] = 0.0;
      acc_min[o] = INFINITY;
      acc_max[o] = -INFINITY;
    }
    // (the loop's first barrier orders both initialisations before the first read)
    const int64_t total = st.rows * st.cols;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < total; base += (int64_t)gridDim.x * 256) {  // uniform trip count
      const int64_t idx = base + tid;
      double x = 0.0;
      int g = ST_NO_ELEMENT;
      if (idx < total) {
        const int64_t row = st.cols == 1 ? idx : idx / st.cols;
        x = st_load(st.data, st.dtype, idx);
        if (st.row_scale != nullptr) x *= st.row_scale[row];
        g = st_group(st, row);
      }
      xs[tid] = x;
      grp[tid] = g;
      __syncthreads();
      for (int o = tid; o < parts * sc; o += 256) {  // o = part * sc + slot: the owner of `share` elements for one slot
        const int part = o / sc, sl = o - part * sc;
        const nqa_stats_term& t = a.terms[tb + slot_term[sl]];
        const int gg = slot_group[sl], mod = t.mod;
        const bool grouped = t.n_groups > 1, drop_nan = t.ignore_nan != 0;
        StAcc v{acc_n[o], acc_hi[o], acc_lo[o], acc_m2[o], acc_min[o], acc_max[o]};
        const int i0 = part * share;
        for (int i = i0; i < i0 + share; ++i) {  // element order
          const int gi = grp[i];
          const double xi = xs[i];
          const bool hit = (grouped ? gi == gg : gi != ST_NO_ELEMENT) && !(drop_nan && xi != xi);
          if (hit) st_push(v, st_modify(mod, xi));
        }
        acc_n[o] = v.n;
        acc_hi[o] = v.hi;
        acc_lo[o] = v.lo;
        acc_m2[o] = v.m2;
        acc_min[o] = v.mn;
        acc_max[o] = v.mx;
      }
      __syncthreads();
    }
    __syncthreads();
    for (int sl = tid; sl < sc; sl += 256) {  // the parts in part order: one row of partial states per workgroup
      StAcc v{acc_n[sl], acc_hi[sl], acc_lo[sl], acc_m2[sl], acc_min[sl], acc_max[sl]};
      for (int part = 1; part < parts; ++part) {
        const int o = part * sc + sl;
        v = st_merge(v, StAcc{acc_n[o], acc_hi[o], acc_lo[o], acc_m2[o], acc_min[o], acc_max[o]});
      }
      const int64_t o = (int64_t)blockIdx.x * a.n_slots + sb + sl;
      part_n[o] = v.n;
      part_hi[o] = v.hi;
      part_lo[o] = v.lo;
      part_m2[o] = v.m2;
      part_min[o] = v.mn;
      part_max[o] = v.mx;
    }
    __syncthreads();  // the next stream reuses the LDS
  }
}

// ---- second stage: one wavefront per slot -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stats_final_kernel(const long long* __restrict__ part_n,
                                                          const double* __restrict__ part_f, long long* __restrict__ state_n,
                                                          double* __restrict__ state_f, int32_t n_slots) {
  // the five float64 planes (mean, mean_lo, M2, min, max) of the partial rows [GROUPS, slots] and of the state [slots]
  const int64_t pp = (int64_t)ST_GROUPS * n_slots;
  const double* __restrict__ part_hi = part_f;
  const double* __restrict__ part_lo = part_f + pp;
  const double* __restrict__ part_m2 = part_f + 2 * pp;
  const double* __restrict__ part_min = part_f + 3 * pp;
  const double* __restrict__ part_max = part_f + 4 * pp;
  double* __restrict__ state_hi = state_f;
  double* __restrict__ state_lo = state_f + n_slots;
  double* __restrict__ state_m2 = state_f + 2 * (int64_t)n_slots;
  double* __restrict__ state_min = state_f + 3 * (int64_t)n_slots;
  double* __restrict__ state_max = state_f + 4 * (int64_t)n_slots;
  constexpr int ROWS = ST_GROUPS / 64;
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= n_slots) return;  // (whole wavefronts: no barrier follows)
  StAcc v = st_empty();
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {  // row order
    const int64_t o = (int64_t)(lane * ROWS + r) * n_slots + s;
    v = st_merge(v, StAcc{part_n[o], part_hi[o], part_lo[o], part_m2[o], part_min[o], part_max[o]});
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {  // a fixed tree: lane l takes lane l + off behind itself
    StAcc w;
    w.n = __shfl_down(v.n, off);
    w.hi = __shfl_down(v.hi, off);
    w.lo = __shfl_down(v.lo, off);
    w.m2 = __shfl_down(v.m2, off);
    w.mn = __shfl_down(v.mn, off);
    w.mx = __shfl_down(v.mx, off);
    if (lane < off) v = st_merge(v, w);
  }
  if (lane != 0 || v.n == 0) return;  // no element in this batch: the slot is left as it is
  const StAcc r = st_merge(StAcc{state_n[s], state_hi[s], state_lo[s], state_m2[s], state_min[s], state_max[s]}, v);
  state_n[s] = r.n;
  state_hi[s] = r.hi;
  state_lo[s] = r.lo;
  state_m2[s] = r.m2;
  state_min[s] = r.mn;
  state_max[s] = r.mx;
}

// ---- neighbour counts -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void neighbor_count_kernel(const int64_t* __restrict__ center, int64_t num_edges,
                                                             int64_t num_atoms, int32_t* __restrict__ counts) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < num_edges; e += (int64_t)gridDim.x * 256) {
    const int64_t c = center[e];
    if (c >= 0 && c < num_atoms) atomicAdd(counts + c, 1);  // (an index outside the atoms counts for nobody)
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
static std::string st_range(int lo, int hi, const char* what) {
  return std::to_string(lo) + " to " + std::to_string(hi) + " " + what;
}
static int st_fail(const char* name, const std::string& what) {
  set_error(std::string(name) + ": " + what);
  return NQA_ERR_INVALID;
}

static int st_prepare(const char* name, const nqa_stats_stream* streams, int32_t n_streams, const nqa_stats_term* terms,
                      int32_t n_terms, StatsArgs& a) {
  if (n_streams < 1 || n_streams > ST_MAX_STREAMS) return st_fail(name, st_range(1, ST_MAX_STREAMS, "streams"));
  if (n_terms < 1 || n_terms > ST_MAX_TERMS) return st_fail(name, st_range(1, ST_MAX_TERMS, "terms"));
  if (!streams || !terms) return st_fail(name, "null descriptor table");
  a = StatsArgs{};
  for (int s = 0; s < n_streams; ++s) {
    const nqa_stats_stream& st = streams[s];
    if (st.rows < 0 || st.cols < 1 || st.dtype < NQA_STATS_F32 || st.dtype > NQA_STATS_I64 || (st.rows > 0 && !st.data))
      return st_fail(name, "invalid stream (rows >= 0, cols >= 1, float32 / float64 / int32 / int64 data)");
    if (st.group_kind < NQA_STATS_GROUP_NONE || st.group_kind > NQA_STATS_GROUP_EDGE)
      return st_fail(name, "unknown group kind");
    if (st.group_kind != NQA_STATS_GROUP_NONE && st.rows > 0) {
      const int cap = st.group_kind == NQA_STATS_GROUP_NODE ? NQA_STATS_MAX_NODE_TYPES : NQA_STATS_MAX_EDGE_TYPES;
      if (st.num_types < 1 || st.num_types > cap) return st_fail(name, st_range(1, cap, "atom types"));
      if (!st.atom_types) return st_fail(name, "a grouped stream needs atom_types");
      if (st.group_kind == NQA_STATS_GROUP_EDGE && (!st.edge_index || st.num_atoms < 0))
        return st_fail(name, "an edge stream needs edge_index and the number of atoms");
    }
    a.st[s] = st;
    a.term_begin[s] = -1;
  }
  int slot = 0, prev_stream = -1;
  for (int k = 0; k < n_terms; ++k) {
    const nqa_stats_term& t = terms[k];
    if (t.stream < 0 || t.stream >= n_streams || t.stream < prev_stream)
      return st_fail(name, "terms must be ordered by stream");
    if (t.mod < NQA_STATS_MOD_IDENTITY || t.mod > NQA_STATS_MOD_SQUARE) return st_fail(name, "unknown element modifier");
    const nqa_stats_stream& st = streams[t.stream];
    int want = 1;
    if (t.n_groups != 1) {
      if (st.group_kind == NQA_STATS_GROUP_NONE) return st_fail(name, "a per-type term needs a grouped stream");
      want = st.group_kind == NQA_STATS_GROUP_NODE ? st.num_types : st.num_types * st.num_types;
    }
    if (t.n_groups != want) return st_fail(name, "a term has 1 slot, T (node stream) or T * T (edge stream)");
    if (t.slot0 != slot) return st_fail(name, "slots must be contiguous in term order");
    if (t.stream != prev_stream) {
      a.term_begin[t.stream] = k;
      a.slot_begin[t.stream] = slot;
      prev_stream = t.stream;
    }
    a.term_count[t.stream] += 1;
    a.slot_count[t.stream] += t.n_groups;
    a.terms[k] = t;
    slot += t.n_groups;
    if (slot > ST_MAX_SLOTS) return st_fail(name, st_range(1, ST_MAX_SLOTS, "slots"));
  }
  for (int s = 0; s < n_streams; ++s) {
    if (a.term_begin[s] < 0) return st_fail(name, "a stream without terms");
    int parts = ST_MAX_PARTS;
    while (parts > 1 && parts * a.slot_count[s] > 256) parts >>= 1;
    a.parts[s] = parts;
    a.amax = parts * a.slot_count[s] > a.amax ? parts * a.slot_count[s] : a.amax;
    a.lmax = a.slot_count[s] > a.lmax ? a.slot_count[s] : a.lmax;
  }
  a.n_streams = n_streams;
  a.n_terms = n_terms;
  a.n_slots = slot;
  return NQA_OK;
}

}  // namespace nqa

extern "C" {

int32_t nqa_stats_groups(void) { return nqa::ST_GROUPS; }

int64_t nqa_stats_workspace_bytes(int32_t n_slots) {
  if (n_slots < 0 || n_slots > nqa::ST_MAX_SLOTS) return -1;
  return (int64_t)nqa::ST_GROUPS * n_slots * 48;
}

int nqa_stats_update(const nqa_stats_stream* streams, int32_t n_streams, const nqa_stats_term* terms, int32_t n_terms,
                     void* workspace, int64_t workspace_bytes, void* state, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_stats_update";
  StatsArgs a;
  const int rc = st_prepare(name, streams, n_streams, terms, n_terms, a);
  if (rc != NQA_OK) return rc;
  if (!workspace || workspace_bytes < nqa_stats_workspace_bytes(a.n_slots) || !state) {
    set_error(std::string(name) + ": workspace of nqa_stats_workspace_bytes and `state` are required");
    return NQA_ERR_WORKSPACE;
  }
  int64_t most = 0;
  for (int s = 0; s < n_streams; ++s) {
    const int64_t total = streams[s].rows * streams[s].cols;
    most = total > most ? total : most;
  }
  if (most == 0) return NQA_OK;  // no element anywhere: the state stays as it is
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t gs = (int64_t)ST_GROUPS * a.n_slots;
  long long* part_n = static_cast<long long*>(workspace);
  double* part_f = reinterpret_cast<double*>(part_n + gs);  // mean, mean_lo, M2, min, max: [GROUPS, slots] each
  long long* state_n = static_cast<long long*>(state);
  double* state_f = reinterpret_cast<double*>(state_n + a.n_slots);
  // at the limits: 2 KiB + 1024 * 48 + 1024 * 8 + 1 KiB = 59 KiB, inside the 64 KiB every launch is granted
  const size_t lds = 256 * 8 + (size_t)a.amax * 48 + (size_t)a.lmax * 8 + 256 * 4;
  static_assert(256 * 8 + ST_MAX_SLOTS * 48 + ST_MAX_SLOTS * 8 + 256 * 4 <= 64 * 1024, "LDS of the first stage");
  hipLaunchKernelGGL(stats_partial_kernel, dim3(ST_GROUPS), dim3(256), lds, s, a, part_n, part_f, part_f + gs,
                     part_f + 2 * gs, part_f + 3 * gs, part_f + 4 * gs);
  hipLaunchKernelGGL(stats_final_kernel, dim3((unsigned)((a.n_slots + 3) / 4)), dim3(256), 0, s, part_n, part_f, state_n,
                     state_f, a.n_slots);
  return launch_status(name);
}

int nqa_stats_neighbor_counts(const int64_t* edge_center, int64_t num_edges, int64_t num_atoms, int32_t* counts,
                              nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_stats_neighbor_counts";
  if (num_edges < 0 || num_atoms < 0) return st_fail(name, "negative size");
  if (num_atoms == 0) return NQA_OK;
  if (!counts || (num_edges > 0 && !edge_center)) return st_fail(name, "null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(counts, 0, (size_t)num_atoms * sizeof(int32_t), s) != hipSuccess) return launch_status(name);
  if (num_edges == 0) return launch_status(name);
  const int64_t blocks = (num_edges + 255) / 256;
  hipLaunchKernelGGL(neighbor_count_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, edge_center,
                     num_edges, num_atoms, counts);
  return launch_status(name);
}

}  // extern "C"
