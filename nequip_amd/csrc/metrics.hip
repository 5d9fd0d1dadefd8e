// Losses and error metrics of a training step on one fused reduction (nequip/train/metrics_manager.py, nequip/train/metrics.py,
// nequip/data/stats.py::_MeanX, nequip/data/modifier.py::PerAtomModifier).
//
// The reference evaluates every metric entry on its own: subtract, square / abs, reduce, with boolean indexing for `per_type`
// and `masked_select` for `ignore_nan` (data-dependent shapes: a host synchronisation each) and one `.item()` per entry.  Here
// a STREAM is one distinct (prediction, target) pair and a TERM one metric attached to a stream; a term owns one SLOT per
// group (1, or one per atom type).  Forward, two launches for any number of terms:
//   metrics_partial_kernel  the first stage of slot_reduce.h on NQA_METRICS_GROUPS workgroups (both sides promoted to float64
//                           before the subtraction); a row of partials holds per slot the sum of the modifier of the difference
//                           (float64), the count of contributing elements (int64) and the maximum of |d| (float64);
//   metrics_final_kernel    one workgroup adds the rows in row order (no floating-point atomics anywhere: bit-reproducible),
//                           forms every slot's batch value, the aggregate over types, weighted_sum, adds the batch to the
//                           running epoch state and writes every returned value into one float64 vector.
// Backward, one launch: metrics_bwd_kernel turns the upstream gradient over ALL returned values into one weight per slot
// (d value / d slot sum, from the saved slot sums and counts) and writes grad_pred once per stream.
// Nothing here depends on data read by the host: forward, state update and backward capture into a hipGraph.
#include <hip/hip_runtime.h>

#include "slot_reduce.h"

namespace nqa {

constexpr int MT_MAX_STREAMS = NQA_METRICS_MAX_STREAMS;
constexpr int MT_MAX_TERMS = NQA_METRICS_MAX_TERMS;
constexpr int MT_MAX_TYPES = NQA_METRICS_MAX_TYPES;
constexpr int MT_MAX_STRATA = NQA_METRICS_MAX_STRATA;
constexpr int MT_GROUPS = NQA_METRICS_GROUPS;
constexpr int MT_MAX_SLOTS = MT_MAX_TERMS * MT_MAX_TYPES;
constexpr int MT_PARTS = 4;  // owners per slot in the first stage: each adds 64 of the workgroup's 256 elements

struct MetricsArgs {
  nqa_metric_stream st[MT_MAX_STREAMS];
  SlotLayout<MT_MAX_STREAMS> lay;
  int32_t need_norm[MT_MAX_STREAMS];          // a stratified term: the target's row norm is needed
  const nqa_metric_term* __restrict__ terms;  // device table
  int32_t n_values, kmax;  // kmax: the most terms of one stream (with lay.lmax: the LDS layout of the first stage)
  int32_t ws_index, pad;
};

__device__ __forceinline__ double mt_load(const void* __restrict__ p, int dtype, int64_t i) {
  return dtype == NQA_F64 ? static_cast<const double*>(p)[i] : (double)static_cast<const float*>(p)[i];
}

// the stratum of a row: `norm >= bound[i]` and not `norm >= bound[i + 1]`, in the order the strata were given (the last
// match wins, a NaN norm matches none: that row's loss is 0)
__device__ __forceinline__ bool mt_stratum(const nqa_metric_term* __restrict__ t, double norm, double& delta) {
  bool found = false;
  for (int i = 0; i < t->n_strata; ++i) {
    const bool lo = norm >= t->bound[i];
    const bool hi = (i + 1 < t->n_strata) && (norm >= t->bound[i + 1]);
    if (lo && !hi) {
      delta = t->stratum_delta[i];
      found = true;
    }
  }
  return found;
}

__device__ __forceinline__ double mt_huber(double d, double delta) {
  const double a = fabs(d);
  return a < delta ? 0.5 * d * d : delta * (a - 0.5 * delta);  // strict <, as the reference
}
__device__ __forceinline__ double mt_sign(double d) { return (double)((0.0 < d) - (d < 0.0)); }
__device__ __forceinline__ double mt_huber_grad(double d, double delta) {
  return fabs(d) < delta ? d : delta * mt_sign(d);
}

// what an element adds to its slot (max-abs: what it is compared with)
__device__ __forceinline__ double mt_value(const nqa_metric_term* __restrict__ t, double d, double norm) {
  switch (t->kind) {
    case NQA_METRIC_MSE:
    case NQA_METRIC_RMSE:
      return d * d;
    case NQA_METRIC_MAE:
    case NQA_METRIC_MAXABS:
      return fabs(d);
    case NQA_METRIC_HUBER:
      return mt_huber(d, t->delta);
    default: {
      double delta = 0.0;
      return mt_stratum(t, norm, delta) ? mt_huber(d, delta) : 0.0;
    }
  }
}

// d (that value) / d d
__device__ __forceinline__ double mt_value_grad(const nqa_metric_term* __restrict__ t, double d, double norm) {
  switch (t->kind) {
    case NQA_METRIC_MSE:
    case NQA_METRIC_RMSE:
      return 2.0 * d;
    case NQA_METRIC_MAE:
      return mt_sign(d);
    case NQA_METRIC_HUBER:
      return mt_huber_grad(d, t->delta);
    case NQA_METRIC_STRATIFIED_HUBER: {
      double delta = 0.0;
      return mt_stratum(t, norm, delta) ? mt_huber_grad(d, delta) : 0.0;
    }
    default:
      return 0.0;
  }
}

// the batch (or epoch) value of a slot from its sum, count and maximum
__device__ __forceinline__ double mt_slot_value(const nqa_metric_term* __restrict__ t, double sum, int64_t cnt, double mx) {
  switch (t->kind) {
    case NQA_METRIC_MAXABS:
      return mx;
    case NQA_METRIC_RMSE:
      return sqrt(sum / (double)cnt);
    case NQA_METRIC_HUBER:
    case NQA_METRIC_STRATIFIED_HUBER:
      return t->reduce_sum ? sum : sum / (double)cnt;
    default:
      return sum / (double)cnt;  // (no element: 0 / 0 = NaN, as the reference)
  }
}

struct MtElement {
  double d, norm, scale;
  int g;
  bool tnan;
};

// one element of a stream: both sides promoted to float64, scaled, subtracted.  With a stratified term on the stream every
// ELEMENT reloads its whole target row for the norm (cols loads, so cols^2 per row, in the forward and in the backward):
// the rows are force vectors, cols = 3, and the reloads hit the lines the element's own load brought in.
__device__ __forceinline__ MtElement mt_element(const nqa_metric_stream& st, bool need_norm, int64_t idx) {
  MtElement e;
  const int64_t row = st.cols == 1 ? idx : idx / st.cols;
  double p = mt_load(st.pred, st.pred_dtype, idx);
  double t = mt_load(st.target, st.target_dtype, idx);
  e.tnan = t != t;
  e.scale = st.row_scale != nullptr ? st.row_scale[row] : 1.0;
  if (st.row_scale != nullptr) {
    p *= e.scale;
    t *= e.scale;
  }
  e.d = p - t;
  e.norm = 0.0;
  if (need_norm) {
    double n2 = 0.0;
    for (int c = 0; c < st.cols; ++c) {
      const double x = mt_load(st.target, st.target_dtype, row * st.cols + c) * e.scale;
      n2 += x * x;
    }
    e.norm = sqrt(n2);
  }
  e.g = 0;
  if (st.group != nullptr) {
    const int64_t g = st.group[row];
    e.g = (g >= 0 && g < MT_MAX_TYPES) ? (int)g : -1;  // outside every term's groups: contributes to none
  }
  return e;
}

// ---- forward, first stage: the policy of slot_sweep --------------------------------------------------------------------------
// LDS behind the slot map: vals [kmax, 256] float64 (one value per term of the stream and element of the sweep), acc_val /
// acc_cnt [MT_PARTS, lmax], grp / msk [256] (the group of an element and the terms it contributes to).
struct MtAcc {
  double v;  // the sum, or the maximum of a max-abs term
  int64_t c;
};

struct MtSweep {
  const MetricsArgs& a;
  double *__restrict__ part_sum, *__restrict__ part_max, *__restrict__ vals, *__restrict__ acc_val;
  int64_t *__restrict__ part_cnt, *__restrict__ acc_cnt;
  int32_t* __restrict__ grp;
  uint32_t* __restrict__ msk;
  const nqa_metric_term* __restrict__ terms;  // of the open stream
  int s, tc;
  static constexpr bool INIT_READS_SLOT_MAP = true;  // (a max-abs term starts from -inf)

  __device__ __forceinline__ MtSweep(const MetricsArgs& a_, char* lds, double* ps, int64_t* pc, double* pm) : a(a_) {
    part_sum = ps, part_cnt = pc, part_max = pm;
    vals = reinterpret_cast<double*>(lds);
    acc_val = vals + (size_t)a.kmax * 256;
    acc_cnt = reinterpret_cast<int64_t*>(acc_val + (size_t)MT_PARTS * a.lay.lmax);
    grp = reinterpret_cast<int32_t*>(acc_cnt + (size_t)MT_PARTS * a.lay.lmax);
    msk = reinterpret_cast<uint32_t*>(grp + 256);
  }
  __device__ __forceinline__ int64_t open(int stream) {
    s = stream, terms = a.terms + a.lay.term_begin[s], tc = a.lay.term_count[s];
    return a.st[s].rows * a.st[s].cols;
  }
  __device__ __forceinline__ int parts() const { return MT_PARTS; }
  __device__ __forceinline__ const nqa_metric_term& term(int k) const { return terms[k]; }
  __device__ __forceinline__ bool is_max(int k) const { return terms[k].kind == NQA_METRIC_MAXABS; }
  __device__ __forceinline__ void init(int part, int sl, int k) {
    acc_val[part * a.lay.lmax + sl] = is_max(k) ? -INFINITY : 0.0;
    acc_cnt[part * a.lay.lmax + sl] = 0;
  }
  __device__ __forceinline__ void stage(int64_t idx, bool in_range) {
    const int tid = threadIdx.x;
    uint32_t m = 0;
    int g = 0;
    if (in_range) {
      const MtElement e = mt_element(a.st[s], a.need_norm[s] != 0, idx);
      g = e.g;
      for (int k = 0; k < tc; ++k) {
        const nqa_metric_term* __restrict__ t = terms + k;
        if (t->ignore_nan && e.tnan) continue;  // masked on the TARGET, as the reference
        m |= 1u << k;
        vals[k * 256 + tid] = mt_value(t, e.d, e.norm);
      }
    }
    msk[tid] = m;
    grp[tid] = g;
  }
  __device__ __forceinline__ void fold(int part, int sl, int k, int gg, int i0, int share) {
    const bool grouped = terms[k].n_groups > 1, mx = is_max(k);
    double v = acc_val[part * a.lay.lmax + sl];
    int64_t c = acc_cnt[part * a.lay.lmax + sl];
    // every load is unconditional (so that the LDS reads of an unrolled block are in flight together) and a value that
    // does not belong to the slot -- possibly a stale one -- is dropped by a select, never by arithmetic
#pragma unroll 8
    for (int i = i0; i < i0 + share; ++i) {
      const bool hit = ((msk[i] >> k) & 1u) && (!grouped || grp[i] == gg);
      const double x = vals[k * 256 + i];
      const double vn = mx ? sr_nanmax(v, x) : v + x;
      v = hit ? vn : v;
      c += hit ? 1 : 0;
    }
    acc_val[part * a.lay.lmax + sl] = v;
    acc_cnt[part * a.lay.lmax + sl] = c;
  }
  __device__ __forceinline__ MtAcc load(int part, int sl) const {
    return {acc_val[part * a.lay.lmax + sl], acc_cnt[part * a.lay.lmax + sl]};
  }
  __device__ __forceinline__ MtAcc merge(const MtAcc& x, const MtAcc& y, int k) const {
    return MtAcc{is_max(k) ? sr_nanmax(x.v, y.v) : x.v + y.v, x.c + y.c};
  }
  __device__ __forceinline__ void store(int64_t o, const MtAcc& r, int k) {
    part_sum[o] = is_max(k) ? 0.0 : r.v;
    part_max[o] = is_max(k) ? r.v : -INFINITY;
    part_cnt[o] = r.c;
  }
};

__global__ __launch_bounds__(256) void metrics_partial_kernel(const MetricsArgs a, double* __restrict__ part_sum,
                                                              int64_t* __restrict__ part_cnt,
                                                              double* __restrict__ part_max) {
  extern __shared__ __attribute__((aligned(16))) char mt_smem[];
  MtSweep p(a, mt_smem + (size_t)a.lay.lmax * 8, part_sum, part_cnt, part_max);
  slot_sweep(a.lay, reinterpret_cast<int32_t*>(mt_smem), p);
}

// ---- forward, second stage: one workgroup -----------------------------------------------------------------------------------
struct MetricsFinalArgs {
  const nqa_metric_term* __restrict__ terms;
  const double* __restrict__ part_sum;
  const int64_t* __restrict__ part_cnt;
  const double* __restrict__ part_max;
  double* __restrict__ state_sum;  // [n_slots] running epoch state, or NULL
  int64_t* __restrict__ state_cnt;
  double* __restrict__ state_max;
  double* __restrict__ saved_sum;  // [n_slots] this batch, for the backward
  int64_t* __restrict__ saved_cnt;
  double* __restrict__ values;     // [n_values]
  int32_t n_terms, n_slots, groups, ws_index;
};

__global__ __launch_bounds__(256) void metrics_final_kernel(const MetricsFinalArgs f) {
  __shared__ double slot_val[MT_MAX_SLOTS];
  __shared__ int32_t slot_term[MT_MAX_SLOTS];
  __shared__ double term_val[MT_MAX_TERMS];
  const int tid = threadIdx.x;
  for (int k = tid; k < f.n_terms; k += 256)
    for (int g = 0; g < f.terms[k].n_groups; ++g) slot_term[f.terms[k].slot0 + g] = k;
  __syncthreads();
  // a wavefront per slot: lane b loads row b (all rows in flight at once), then the rows are added in row order out of
  // the lanes' registers; every lane forms the same sums, lane 0 stores them
  static_assert(MT_GROUPS <= 64, "one lane per row of partials");
  const int lane = tid & 63;
  for (int s = tid >> 6; s < f.n_slots; s += 4) {
    const nqa_metric_term* __restrict__ t = f.terms + slot_term[s];
    double ps = 0.0, pm = -INFINITY;
    long long pc = 0;
    if (lane < f.groups) {
      ps = f.part_sum[(int64_t)lane * f.n_slots + s];
      pc = f.part_cnt[(int64_t)lane * f.n_slots + s];
      pm = f.part_max[(int64_t)lane * f.n_slots + s];
    }
    double sum = 0.0, mx = -INFINITY;
    int64_t cnt = 0;
    for (int b = 0; b < f.groups; ++b) {  // row order
      sum += __shfl(ps, b);
      cnt += __shfl(pc, b);
      mx = sr_nanmax(mx, __shfl(pm, b));
    }
    if (lane != 0) continue;
    f.saved_sum[s] = sum;
    f.saved_cnt[s] = cnt;
    if (f.state_sum != nullptr) {
      f.state_sum[s] += sum;
      f.state_cnt[s] += cnt;
      f.state_max[s] = sr_nanmax(f.state_max[s], mx);
    }
    const double v = mt_slot_value(t, sum, cnt, mx);
    slot_val[s] = v;
    if (t->n_groups > 1) f.values[t->out0 + (s - t->slot0)] = v;
  }
  __syncthreads();
  for (int k = tid; k < f.n_terms; k += 256) {
    const nqa_metric_term* __restrict__ t = f.terms + k;
    double tv;
    if (t->n_groups == 1) {
      tv = slot_val[t->slot0];
      f.values[t->out0] = tv;
    } else {  // the types whose value is not NaN, equally or by their coefficients
      double num = 0.0, den = 0.0;
      for (int g = 0; g < t->n_groups; ++g) {
        const double v = slot_val[t->slot0 + g];
        if (v == v) {
          const double c = t->has_group_coeffs ? t->group_coeff[g] : 1.0;
          num += c * v;
          den += c;
        }
      }
      tv = num / den;
      f.values[t->out0 + t->n_groups] = tv;
    }
    term_val[k] = tv;
  }
  __syncthreads();
  if (tid == 0 && f.ws_index >= 0) {
    double ws = 0.0;
    for (int k = 0; k < f.n_terms; ++k)
      if (f.terms[k].has_coeff) ws += term_val[k] * f.terms[k].coeff;
    f.values[f.ws_index] = ws;
  }
}

// ---- backward: one launch ---------------------------------------------------------------------------------------------------
// w[slot] = d L / d (slot sum): the upstream of the slot's own value, of its term's aggregate and of weighted_sum, times
// 1 / count (mean), 1 / (2 rmse count) (root), 1 (sum); max-abs terms are metrics, computed detached: 0.  A value nothing
// upstream uses gets an exact 0 (not 0 * inf), and an element only reads the weights that are not 0.  One case is left as
// autograd has it in the reference and in the ATen form: a root-mean-square term whose value is EXACTLY 0 and that something
// upstream does use has the weight up / (2 * 0 * count) = inf against element gradients 2 d = 0, so its grad_pred is NaN
// (the derivative of sqrt at 0).
__global__ __launch_bounds__(256) void metrics_bwd_kernel(const MetricsArgs a, const double* __restrict__ saved_sum,
                                                          const int64_t* __restrict__ saved_cnt,
                                                          const double* __restrict__ gout) {
  extern __shared__ __attribute__((aligned(16))) char mt_smem[];
  double* __restrict__ w = reinterpret_cast<double*>(mt_smem);  // [n_slots]
  // every workgroup forms all the slot weights for itself from the device table and the saved sums: at most 512 slots of
  // a few operations each, cheaper than a launch of its own that would write them once
  const int tid = threadIdx.x;
  for (int k = tid; k < a.lay.n_terms; k += 256) {
    const nqa_metric_term* __restrict__ t = a.terms + k;
    const int ng = t->n_groups;
    const double gws = (a.ws_index >= 0 && t->has_coeff) ? gout[a.ws_index] * t->coeff : 0.0;
    double den = 0.0;
    if (ng > 1)
      for (int g = 0; g < ng; ++g) {
        const double v = mt_slot_value(t, saved_sum[t->slot0 + g], saved_cnt[t->slot0 + g], 0.0);
        if (v == v) den += t->has_group_coeffs ? t->group_coeff[g] : 1.0;
      }
    for (int g = 0; g < ng; ++g) {
      const int s = t->slot0 + g;
      const double sum = saved_sum[s];
      const int64_t cnt = saved_cnt[s];
      const double v = mt_slot_value(t, sum, cnt, 0.0);
      double up;
      if (ng == 1) {
        up = gout[t->out0] + gws;
      } else {
        up = gout[t->out0 + g];
        const double gagg = gout[t->out0 + ng] + gws;
        if (v == v && gagg != 0.0) up += gagg * (t->has_group_coeffs ? t->group_coeff[g] : 1.0) / den;
      }
      double r = 0.0;
      if (t->kind != NQA_METRIC_MAXABS && up != 0.0 && cnt > 0) {
        if (t->kind == NQA_METRIC_RMSE)
          r = up * (0.5 / (v * (double)cnt));
        else if ((t->kind == NQA_METRIC_HUBER || t->kind == NQA_METRIC_STRATIFIED_HUBER) && t->reduce_sum)
          r = up;
        else
          r = up / (double)cnt;
      }
      w[s] = r;
    }
  }
  __syncthreads();
  for (int s = 0; s < a.lay.n_streams; ++s) {
    const nqa_metric_stream& st = a.st[s];
    if (st.grad_pred == nullptr) continue;
    const int tb = a.lay.term_begin[s], tc = a.lay.term_count[s];
    const bool need_norm = a.need_norm[s] != 0;
    const int64_t total = st.rows * st.cols;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + tid; idx < total; idx += (int64_t)gridDim.x * 256) {
      const MtElement e = mt_element(st, need_norm, idx);
      double acc = 0.0;
      for (int k = 0; k < tc; ++k) {
        const nqa_metric_term* __restrict__ t = a.terms + tb + k;
        if (t->ignore_nan && e.tnan) continue;  // a masked element: exactly zero
        int sl = t->slot0;
        if (t->n_groups > 1) {
          if (e.g < 0 || e.g >= t->n_groups) continue;
          sl += e.g;
        }
        const double wv = w[sl];
        if (wv != 0.0) acc += wv * mt_value_grad(t, e.d, e.norm);
      }
      acc *= e.scale;
      if (st.pred_dtype == NQA_F64)
        static_cast<double*>(st.grad_pred)[idx] = acc;
      else
        static_cast<float*>(st.grad_pred)[idx] = (float)acc;
    }
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// checks the descriptors and fills the launch arguments; `terms` is the HOST copy of the device table
static int mt_prepare(const char* name, const nqa_metric_stream* streams, int32_t n_streams, const nqa_metric_term* terms,
                      const nqa_metric_term* terms_device, int32_t n_terms, int32_t n_values, int32_t ws_index,
                      MetricsArgs& a) {
  int rc = slot_limits(name, n_streams, MT_MAX_STREAMS, n_terms, MT_MAX_TERMS, streams && terms && terms_device);
  if (rc != NQA_OK) return rc;
  if (n_values < 1 || ws_index < -1 || ws_index >= n_values) return slot_fail(name, "weighted_sum index outside the values");
  a = MetricsArgs{};
  for (int s = 0; s < n_streams; ++s) {
    const nqa_metric_stream& st = streams[s];
    if (st.rows < 0 || st.cols < 1 || (st.pred_dtype != NQA_F32 && st.pred_dtype != NQA_F64) ||
        (st.target_dtype != NQA_F32 && st.target_dtype != NQA_F64) || (st.rows > 0 && (!st.pred || !st.target)))
      return slot_fail(name, "invalid stream (rows >= 0, cols >= 1, float32 / float64 data)");
    a.st[s] = st;
  }
  rc = slot_layout_fill(name, terms, n_streams, n_terms, a.lay, [&](const nqa_metric_term& t, int) {
    if (t.kind < NQA_METRIC_MSE || t.kind > NQA_METRIC_STRATIFIED_HUBER) return slot_fail(name, "unknown metric kind");
    if (t.n_groups < 1 || t.n_groups > MT_MAX_TYPES) return slot_fail(name, slot_range(1, MT_MAX_TYPES, "groups per term"));
    if (t.n_groups > 1 && streams[t.stream].group == nullptr && streams[t.stream].rows > 0)
      return slot_fail(name, "a grouped term needs the stream's group index");
    if (t.kind == NQA_METRIC_STRATIFIED_HUBER && (t.n_strata < 2 || t.n_strata > MT_MAX_STRATA))
      return slot_fail(name, slot_range(2, MT_MAX_STRATA, "strata"));
    const int outs = t.n_groups > 1 ? t.n_groups + 1 : 1;
    if (t.out0 < 0 || t.out0 + outs > n_values) return slot_fail(name, "value index outside the values");
    if (t.kind == NQA_METRIC_STRATIFIED_HUBER) a.need_norm[t.stream] = 1;
    return (int)NQA_OK;
  });
  if (rc != NQA_OK) return rc;
  for (int s = 0; s < n_streams; ++s) a.kmax = a.lay.term_count[s] > a.kmax ? a.lay.term_count[s] : a.kmax;
  a.terms = terms_device;
  a.n_values = n_values;
  a.ws_index = ws_index;
  return NQA_OK;
}

}  // namespace nqa

extern "C" {

int32_t nqa_metrics_groups(void) { return nqa::MT_GROUPS; }

int64_t nqa_metrics_workspace_bytes(int32_t n_slots) {
  if (n_slots < 0 || n_slots > nqa::MT_MAX_SLOTS) return -1;
  return (int64_t)nqa::MT_GROUPS * n_slots * 24;
}

int nqa_metrics_fwd(const nqa_metric_stream* streams, int32_t n_streams, const nqa_metric_term* terms,
                    const nqa_metric_term* terms_device, int32_t n_terms, int32_t n_values, int32_t weighted_sum_index,
                    void* workspace, int64_t workspace_bytes, void* state, void* saved, double* values, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_metrics_fwd";
  MetricsArgs a;
  const int rc = mt_prepare(name, streams, n_streams, terms, terms_device, n_terms, n_values, weighted_sum_index, a);
  if (rc != NQA_OK) return rc;
  if (!workspace || workspace_bytes < nqa_metrics_workspace_bytes(a.lay.n_slots) || !saved || !values) {
    set_error(std::string(name) + ": workspace of nqa_metrics_workspace_bytes, `saved` and `values` are required");
    return NQA_ERR_WORKSPACE;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t gs = (int64_t)MT_GROUPS * a.lay.n_slots;
  double* part_sum = static_cast<double*>(workspace);
  int64_t* part_cnt = reinterpret_cast<int64_t*>(part_sum + gs);
  double* part_max = reinterpret_cast<double*>(part_cnt + gs);
  const size_t lds = (size_t)a.kmax * 256 * 8 + (size_t)MT_PARTS * a.lay.lmax * 16 + (size_t)a.lay.lmax * 8 + 256 * 8;
  if (lds > 64 * 1024) {  // (set at every such call: cheap, and right on every device and from every thread)
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&metrics_partial_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
      (void)hipGetLastError();
      set_error(std::string(name) + ": the first stage needs " + std::to_string(lds) + " bytes of LDS for " +
                std::to_string(a.kmax) + " terms / " + std::to_string(a.lay.lmax) +
                " slots on one stream, which this device does not grant");
      return NQA_ERR_LAUNCH;
    }
  }
  hipLaunchKernelGGL(metrics_partial_kernel, dim3(MT_GROUPS), dim3(256), lds, s, a, part_sum, part_cnt, part_max);
  MetricsFinalArgs f{};
  f.terms = terms_device;
  f.part_sum = part_sum;
  f.part_cnt = part_cnt;
  f.part_max = part_max;
  if (state != nullptr) {
    f.state_sum = static_cast<double*>(state);
    f.state_cnt = reinterpret_cast<int64_t*>(f.state_sum + a.lay.n_slots);
    f.state_max = reinterpret_cast<double*>(f.state_cnt + a.lay.n_slots);
  }
  f.saved_sum = static_cast<double*>(saved);
  f.saved_cnt = reinterpret_cast<int64_t*>(f.saved_sum + a.lay.n_slots);
  f.values = values;
  f.n_terms = a.lay.n_terms;
  f.n_slots = a.lay.n_slots;
  f.groups = MT_GROUPS;
  f.ws_index = weighted_sum_index;
  hipLaunchKernelGGL(metrics_final_kernel, dim3(1), dim3(256), 0, s, f);
  return launch_status(name);
}

int nqa_metrics_bwd(const nqa_metric_stream* streams, int32_t n_streams, const nqa_metric_term* terms,
                    const nqa_metric_term* terms_device, int32_t n_terms, int32_t n_values, int32_t weighted_sum_index,
                    const void* saved, const double* grad_values, nqa_stream stream) {
  using namespace nqa;
  const char* name = "nqa_metrics_bwd";
  MetricsArgs a;
  const int rc = mt_prepare(name, streams, n_streams, terms, terms_device, n_terms, n_values, weighted_sum_index, a);
  if (rc != NQA_OK) return rc;
  if (!saved || !grad_values) return slot_fail(name, "`saved` and `grad_values` are required");
  int64_t most = 0;
  for (int s = 0; s < n_streams; ++s)
    if (streams[s].grad_pred != nullptr && streams[s].rows * streams[s].cols > most) most = streams[s].rows * streams[s].cols;
  if (most == 0) return NQA_OK;
  const int64_t blocks = (most + 255) / 256;
  const double* saved_sum = static_cast<const double*>(saved);
  const int64_t* saved_cnt = reinterpret_cast<const int64_t*>(saved_sum + a.lay.n_slots);
  hipLaunchKernelGGL(metrics_bwd_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256),
                     (size_t)a.lay.n_slots * 8, static_cast<hipStream_t>(stream), a, saved_sum, saved_cnt, grad_values);
  return launch_status(name);
}

}  // extern "C"
