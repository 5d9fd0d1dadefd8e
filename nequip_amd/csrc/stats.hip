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
//   stats_partial_kernel   the first stage of slot_reduce.h on NQA_STATS_GROUPS workgroups: elements promoted to float64, the
//                          group index formed from atom_types / edge_index in the kernel, Welford updates in element order,
//                          the parts merged by Chan's formula.
//   stats_final_kernel     one wavefront per slot: lane b merges rows 4b .. 4b+3 in row order, the lanes are merged by a fixed
//                          shuffle tree, lane 0 merges the batch into the running state (a batch without an element for the
//                          slot leaves it untouched).
//   neighbor_count_kernel  counts edge_index[0] into a zeroed [N] int32 workspace (integer atomics: exact, order-independent),
//                          which the first kernel then reads as an integer stream.
// No floating-point atomics and a fixed merge order: two runs over the same batches give bit-identical state.  No sum of
// squares is ever differenced: the variance of total energies (1e5 with a spread of 1e-1) keeps its digits.  Nothing is read by
// the host, so an update captures into a hipGraph.
#include <hip/hip_runtime.h>

#include "slot_reduce.h"

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

__device__ __forceinline__ StAcc st_empty() { return StAcc{0, 0.0, 0.0, 0.0, INFINITY, -INFINITY}; }

// an accumulator kept as six planes of `stride` entries each: count (int64), then mean, mean_lo, M2, min, max (float64)
__device__ __forceinline__ StAcc st_get(const long long* n, const double* f, int64_t stride, int64_t o) {
  return StAcc{n[o], f[o], f[stride + o], f[2 * stride + o], f[3 * stride + o], f[4 * stride + o]};
}
__device__ __forceinline__ void st_put(long long* n, double* f, int64_t stride, int64_t o, const StAcc& v) {
  n[o] = v.n;
  f[o] = v.hi;
  f[stride + o] = v.lo;
  f[2 * stride + o] = v.m2;
  f[3 * stride + o] = v.mn;
  f[4 * stride + o] = v.mx;
}

// one more element (Welford on y - pivot; the first element is the pivot)
__device__ __forceinline__ void st_push(StAcc& a, double y) {
  if (a.n == 0) a.hi = y;
  a.n += 1;
  const double z = y - a.hi;
  const double d = z - a.lo;
  a.lo += d / (double)a.n;
  a.m2 += d * (z - a.lo);
  a.mn = sr_nanmin(a.mn, y);
  a.mx = sr_nanmax(a.mx, y);
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
  r.mn = sr_nanmin(a.mn, b.mn);
  r.mx = sr_nanmax(a.mx, b.mx);
  return r;
}

struct StatsArgs {
  nqa_stats_stream st[ST_MAX_STREAMS];
  nqa_stats_term terms[ST_MAX_TERMS];  // ordered by stream
  SlotLayout<ST_MAX_STREAMS> lay;
  int32_t parts[ST_MAX_STREAMS];  // owners per slot
  int32_t amax;                   // most (parts * slots) of one stream (with lay.lmax: the LDS layout)
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

// ---- first stage: the policy of slot_sweep ------------------------------------------------------------------------------------
// LDS behind the slot map: xs [256] float64 and grp [256] int32 (the sweep: -2 marks a lane past the end), the owners'
// accumulators [amax] x (count, mean, mean_lo, M2, min, max).
constexpr int ST_NO_ELEMENT = -2;

struct StSweep {
  const StatsArgs& a;
  long long *__restrict__ part_n, *__restrict__ acc_n;
  double *__restrict__ part_f, *__restrict__ acc_f, *__restrict__ xs;  // planes of part_f: [GROUPS, slots], of acc_f: [amax]
  int32_t* __restrict__ grp;
  int s, tb, sc;
  static constexpr bool INIT_READS_SLOT_MAP = false;

  __device__ __forceinline__ StSweep(const StatsArgs& a_, char* lds, long long* pn, double* pf) : a(a_), part_n(pn), part_f(pf) {
    xs = reinterpret_cast<double*>(lds);
    acc_n = reinterpret_cast<long long*>(xs + 256);
    acc_f = reinterpret_cast<double*>(acc_n + a.amax);
    grp = reinterpret_cast<int32_t*>(acc_f + 5 * (size_t)a.amax);
  }
  __device__ __forceinline__ int64_t open(int stream) {
    s = stream, tb = a.lay.term_begin[s], sc = a.lay.slot_count[s];
    return a.st[s].rows * a.st[s].cols;
  }
  __device__ __forceinline__ int parts() const { return a.parts[s]; }
  __device__ __forceinline__ const nqa_stats_term& term(int k) const { return a.terms[tb + k]; }
  __device__ __forceinline__ StAcc load(int part, int sl) const { return st_get(acc_n, acc_f, a.amax, part * sc + sl); }
  __device__ __forceinline__ void init(int part, int sl, int) { st_put(acc_n, acc_f, a.amax, part * sc + sl, st_empty()); }
  __device__ __forceinline__ void stage(int64_t idx, bool in_range) {
    const nqa_stats_stream& st = a.st[s];
    double x = 0.0;
    int g = ST_NO_ELEMENT;
    if (in_range) {
      const int64_t row = st.cols == 1 ? idx : idx / st.cols;
      x = st_load(st.data, st.dtype, idx);
      if (st.row_scale != nullptr) x *= st.row_scale[row];
      g = st_group(st, row);
    }
    xs[threadIdx.x] = x;
    grp[threadIdx.x] = g;
  }
  __device__ __forceinline__ void fold(int part, int sl, int k, int gg, int i0, int share) {
    const nqa_stats_term& t = term(k);
    const int mod = t.mod;
    const bool grouped = t.n_groups > 1, drop_nan = t.ignore_nan != 0;
    StAcc v = load(part, sl);
    for (int i = i0; i < i0 + share; ++i) {  // element order
      const int gi = grp[i];
      const double xi = xs[i];
      const bool hit = (grouped ? gi == gg : gi != ST_NO_ELEMENT) && !(drop_nan && xi != xi);
      if (hit) st_push(v, st_modify(mod, xi));
    }
    st_put(acc_n, acc_f, a.amax, part * sc + sl, v);
  }
  __device__ __forceinline__ StAcc merge(const StAcc& x, const StAcc& y, int) const { return st_merge(x, y); }
  __device__ __forceinline__ void store(int64_t o, const StAcc& v, int) {
    st_put(part_n, part_f, (int64_t)ST_GROUPS * a.lay.n_slots, o, v);
  }
};

__global__ __launch_bounds__(256) void stats_partial_kernel(const StatsArgs a, long long* __restrict__ part_n,
                                                            double* __restrict__ part_f) {
  extern __shared__ __attribute__((aligned(16))) char st_smem[];
  StSweep p(a, st_smem + (size_t)a.lay.lmax * 8, part_n, part_f);
  slot_sweep(a.lay, reinterpret_cast<int32_t*>(st_smem), p);
}

// ---- second stage: one wavefront per slot -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stats_final_kernel(const long long* __restrict__ part_n,
                                                          const double* __restrict__ part_f, long long* __restrict__ state_n,
                                                          double* __restrict__ state_f, int32_t n_slots) {
  const int64_t pp = (int64_t)ST_GROUPS * n_slots;  // a plane of the partial rows [GROUPS, slots]; of the state: [slots]
  constexpr int ROWS = ST_GROUPS / 64;
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= n_slots) return;  // (whole wavefronts: no barrier follows)
  StAcc v = st_empty();
#pragma unroll
  for (int r = 0; r < ROWS; ++r)  // row order
    v = st_merge(v, st_get(part_n, part_f, pp, (int64_t)(lane * ROWS + r) * n_slots + s));
  v = wave_merge_ordered(v, lane, st_merge);
  if (lane != 0 || v.n == 0) return;  // no element in this batch: the slot is left as it is
  st_put(state_n, state_f, n_slots, s, st_merge(st_get(state_n, state_f, n_slots, s), v));
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
static int st_prepare(const char* name, const nqa_stats_stream* streams, int32_t n_streams, const nqa_stats_term* terms,
                      int32_t n_terms, StatsArgs& a) {
  int rc = slot_limits(name, n_streams, ST_MAX_STREAMS, n_terms, ST_MAX_TERMS, streams && terms);
  if (rc != NQA_OK) return rc;
  a = StatsArgs{};
  for (int s = 0; s < n_streams; ++s) {
    const nqa_stats_stream& st = streams[s];
    if (st.rows < 0 || st.cols < 1 || st.dtype < NQA_STATS_F32 || st.dtype > NQA_STATS_I64 || (st.rows > 0 && !st.data))
      return slot_fail(name, "invalid stream (rows >= 0, cols >= 1, float32 / float64 / int32 / int64 data)");
    if (st.group_kind < NQA_STATS_GROUP_NONE || st.group_kind > NQA_STATS_GROUP_EDGE)
      return slot_fail(name, "unknown group kind");
    if (st.group_kind != NQA_STATS_GROUP_NONE && st.rows > 0) {
      const int cap = st.group_kind == NQA_STATS_GROUP_NODE ? NQA_STATS_MAX_NODE_TYPES : NQA_STATS_MAX_EDGE_TYPES;
      if (st.num_types < 1 || st.num_types > cap) return slot_fail(name, slot_range(1, cap, "atom types"));
      if (!st.atom_types) return slot_fail(name, "a grouped stream needs atom_types");
      if (st.group_kind == NQA_STATS_GROUP_EDGE && (!st.edge_index || st.num_atoms < 0))
        return slot_fail(name, "an edge stream needs edge_index and the number of atoms");
    }
    a.st[s] = st;
  }
  rc = slot_layout_fill(name, terms, n_streams, n_terms, a.lay, [&](const nqa_stats_term& t, int slot) {
    if (t.mod < NQA_STATS_MOD_IDENTITY || t.mod > NQA_STATS_MOD_SQUARE) return slot_fail(name, "unknown element modifier");
    const nqa_stats_stream& st = streams[t.stream];
    int want = 1;
    if (t.n_groups != 1) {
      if (st.group_kind == NQA_STATS_GROUP_NONE) return slot_fail(name, "a per-type term needs a grouped stream");
      want = st.group_kind == NQA_STATS_GROUP_NODE ? st.num_types : st.num_types * st.num_types;
    }
    if (t.n_groups != want) return slot_fail(name, "a term has 1 slot, T (node stream) or T * T (edge stream)");
    if (slot + t.n_groups > ST_MAX_SLOTS) return slot_fail(name, slot_range(1, ST_MAX_SLOTS, "slots"));
    return (int)NQA_OK;
  });
  if (rc != NQA_OK) return rc;
  for (int k = 0; k < n_terms; ++k) a.terms[k] = terms[k];
  for (int s = 0; s < n_streams; ++s) {
    int parts = ST_MAX_PARTS;
    while (parts > 1 && parts * a.lay.slot_count[s] > 256) parts >>= 1;
    a.parts[s] = parts;
    a.amax = parts * a.lay.slot_count[s] > a.amax ? parts * a.lay.slot_count[s] : a.amax;
  }
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
  if (!workspace || workspace_bytes < nqa_stats_workspace_bytes(a.lay.n_slots) || !state) {
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
  const int64_t gs = (int64_t)ST_GROUPS * a.lay.n_slots;
  long long* part_n = static_cast<long long*>(workspace);
  double* part_f = reinterpret_cast<double*>(part_n + gs);  // mean, mean_lo, M2, min, max: [GROUPS, slots] each
  long long* state_n = static_cast<long long*>(state);
  double* state_f = reinterpret_cast<double*>(state_n + a.lay.n_slots);
  // at the limits: 2 KiB + 1024 * 48 + 1024 * 8 + 1 KiB = 59 KiB, inside the 64 KiB every launch is granted
  const size_t lds = 256 * 8 + (size_t)a.amax * 48 + (size_t)a.lay.lmax * 8 + 256 * 4;
  static_assert(256 * 8 + ST_MAX_SLOTS * 48 + ST_MAX_SLOTS * 8 + 256 * 4 <= 64 * 1024, "LDS of the first stage");
  hipLaunchKernelGGL(stats_partial_kernel, dim3(ST_GROUPS), dim3(256), lds, s, a, part_n, part_f);
  hipLaunchKernelGGL(stats_final_kernel, dim3((unsigned)((a.lay.n_slots + 3) / 4)), dim3(256), 0, s, part_n, part_f, state_n,
                     state_f, a.lay.n_slots);
  return launch_status(name);
}

int nqa_stats_neighbor_counts(const int64_t* edge_center, int64_t num_edges, int64_t num_atoms, int32_t* counts,
                              nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_stats_neighbor_counts";
  if (num_edges < 0 || num_atoms < 0) return slot_fail(name, "negative size");
  if (num_atoms == 0) return NQA_OK;
  if (!counts || (num_edges > 0 && !edge_center)) return slot_fail(name, "null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(counts, 0, (size_t)num_atoms * sizeof(int32_t), s) != hipSuccess) return launch_status(name);
  if (num_edges == 0) return launch_status(name);
  const int64_t blocks = (num_edges + 255) / 256;
  hipLaunchKernelGGL(neighbor_count_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, edge_center,
                     num_edges, num_atoms, counts);
  return launch_status(name);
}

}  // extern "C"
