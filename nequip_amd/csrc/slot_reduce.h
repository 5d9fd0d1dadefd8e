// The STREAM / TERM / SLOT reduction of metrics.hip and stats.hip, and the helpers training_stats.hip shares with them.
//
// A STREAM is one tensor (or pair of tensors) walked once, a TERM one quantity reduced over a stream, a SLOT one group of a term;
// the term table is ordered by stream and its slots are contiguous in term order.  The first stage (`slot_sweep`) leaves ONE row
// of per-slot partial accumulators per workgroup in the workspace, the user's second stage merges the rows in row order: no
// floating-point atomics and a fixed merge order everywhere, so the same inputs give the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "launch_status.h"

namespace nqa {

// minimum / maximum that keep a NaN (torch.minimum / torch.maximum do; fmin / fmax would drop it)
__device__ __forceinline__ double sr_nanmin(double a, double b) { return (a != a || b != b) ? (a + b) : fmin(a, b); }
__device__ __forceinline__ double sr_nanmax(double a, double b) { return (a != a || b != b) ? (a + b) : fmax(a, b); }

// the lanes of a wavefront by a fixed tree: lane l takes lane l + off BEHIND itself, so lane 0 ends with all 64 in lane order.
// `Acc` travels through the shuffles as 8-byte words, whatever its fields are.
template <typename Acc, typename Merge>
__device__ __forceinline__ Acc wave_merge_ordered(Acc acc, int lane, Merge merge) {
  constexpr int WORDS = sizeof(Acc) / 8;
  static_assert(sizeof(Acc) % 8 == 0, "an accumulator of 8-byte words");
  struct Words { long long w[WORDS]; };
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    Words v, w;
    __builtin_memcpy(&v, &acc, sizeof(Acc));
#pragma unroll
    for (int i = 0; i < WORDS; ++i) w.w[i] = __shfl_down(v.w[i], off);
    Acc behind;
    __builtin_memcpy(&behind, &w, sizeof(Acc));
    if (lane < off) acc = merge(acc, behind);
  }
  return acc;
}

// ---- the slot layout of a term table ----------------------------------------------------------------------------------------
template <int MAX_STREAMS>
struct SlotLayout {
  int32_t term_begin[MAX_STREAMS], term_count[MAX_STREAMS];  // the terms of a stream are contiguous in the table
  int32_t slot_begin[MAX_STREAMS], slot_count[MAX_STREAMS];  // ... and so are their slots
  int32_t n_streams, n_terms, n_slots, lmax;  // lmax: the most slots of one stream
};

inline std::string slot_range(int lo, int hi, const char* what) {
  return std::to_string(lo) + " to " + std::to_string(hi) + " " + what;
}
inline int slot_fail(const char* name, const std::string& what) {
  set_error(std::string(name) + ": " + what);
  return NQA_ERR_INVALID;
}

// what every entry point checks before it looks at a table
inline int slot_limits(const char* name, int32_t n_streams, int max_streams, int32_t n_terms, int max_terms, bool tables) {
  if (n_streams < 1 || n_streams > max_streams) return slot_fail(name, slot_range(1, max_streams, "streams"));
  if (n_terms < 1 || n_terms > max_terms) return slot_fail(name, slot_range(1, max_terms, "terms"));
  if (!tables) return slot_fail(name, "null descriptor table");
  return NQA_OK;
}

// fills `lay` from a HOST term table with `stream`, `n_groups` and `slot0`.  `check(t, slot)` is the user's own check of a term
// (it must bound n_groups), called once the term is known to lie on a stream; `slot` is the number of slots before it.
template <int MAX_STREAMS, typename Term, typename Check>
int slot_layout_fill(const char* name, const Term* terms, int32_t n_streams, int32_t n_terms, SlotLayout<MAX_STREAMS>& lay,
                     Check check) {
  lay = SlotLayout<MAX_STREAMS>{};
  for (int s = 0; s < n_streams; ++s) lay.term_begin[s] = -1;
  int prev_stream = -1;
  for (int k = 0; k < n_terms; ++k) {
    const Term& t = terms[k];
    if (t.stream < 0 || t.stream >= n_streams || t.stream < prev_stream)
      return slot_fail(name, "terms must be ordered by stream");  // (the slot map of the first stage relies on it)
    const int rc = check(t, lay.n_slots);
    if (rc != NQA_OK) return rc;
    if (t.slot0 != lay.n_slots) return slot_fail(name, "slots must be contiguous in term order");
    if (t.stream != prev_stream) {
      lay.term_begin[t.stream] = k;
      lay.slot_begin[t.stream] = lay.n_slots;
      prev_stream = t.stream;
    }
    lay.term_count[t.stream] += 1;
    lay.slot_count[t.stream] += t.n_groups;
    lay.n_slots += t.n_groups;
  }
  for (int s = 0; s < n_streams; ++s) {
    if (lay.term_begin[s] < 0) return slot_fail(name, "a stream without terms");
    lay.lmax = lay.slot_count[s] > lay.lmax ? lay.slot_count[s] : lay.lmax;
  }
  lay.n_streams = n_streams;
  lay.n_terms = n_terms;
  return NQA_OK;
}

// ---- the first stage --------------------------------------------------------------------------------------------------------
// 256 threads; every workgroup walks every stream once by a grid stride.  A sweep stages 256 elements in LDS; owner thread
// o = part * slots + slot folds the `share` = 256 / parts elements of its part into its own accumulator in element order (one
// writing thread per accumulator: plain read-modify-write); the parts are merged in part order into the workgroup's row.
// `slot_map` is 2 * lay.lmax int32 of LDS: the term and the group of every slot of the stream.  The Policy owns everything else:
//   open(s), parts()             the stream to walk: its number of elements, and the owners per slot on it (256 / 2^i)
//   term(k)                      term k of the stream (n_groups, slot0)
//   init(part, slot, k)          an empty accumulator; INIT_READS_SLOT_MAP says whether it depends on k
//   stage(idx, in_range)         what this lane leaves in LDS for element idx (nothing that counts when !in_range)
//   fold(part, slot, k, g, i0, share)   the owner's accumulator over the staged elements i0 .. i0 + share - 1, group g of term k
//   load(part, slot), merge(a, b, k), store(row_index, acc, k)   the row of partials
template <int MAX_STREAMS, typename Policy>
__device__ __forceinline__ void slot_sweep(const SlotLayout<MAX_STREAMS>& lay, int32_t* __restrict__ slot_map, Policy& p) {
  int32_t *__restrict__ slot_term = slot_map, *__restrict__ slot_group = slot_map + lay.lmax;
  const int tid = threadIdx.x;
  for (int s = 0; s < lay.n_streams; ++s) {
    const int tc = lay.term_count[s], sb = lay.slot_begin[s], sc = lay.slot_count[s];
    const int64_t total = p.open(s);
    const int parts = p.parts(), share = 256 / parts;
    for (int k = tid; k < tc; k += 256) {
      const auto& t = p.term(k);
      for (int g = 0; g < t.n_groups; ++g) {
        slot_term[t.slot0 - sb + g] = k;
        slot_group[t.slot0 - sb + g] = g;
      }
    }
    if (Policy::INIT_READS_SLOT_MAP) __syncthreads();  // (a barrier per stream that the others do not pay)
    for (int o = tid; o < parts * sc; o += 256) p.init(o / sc, o % sc, slot_term[o % sc]);
    // (the loop's first barrier, or the one behind the loop, orders slot map and initialisation before their first read)
    for (int64_t base = (int64_t)blockIdx.x * 256; base < total; base += (int64_t)gridDim.x * 256) {
      const int64_t idx = base + tid;  // a uniform trip count: every thread reaches both barriers, with or without an element
      p.stage(idx, idx < total);
      __syncthreads();
      for (int o = tid; o < parts * sc; o += 256) {
        const int part = o / sc, sl = o - part * sc;
        p.fold(part, sl, slot_term[sl], slot_group[sl], part * share, share);
      }
      __syncthreads();  // the next sweep overwrites what the owners have just read
    }
    __syncthreads();
    for (int sl = tid; sl < sc; sl += 256) {  // the parts in part order: one row of partials per workgroup
      const int k = slot_term[sl];
      auto v = p.load(0, sl);
      for (int part = 1; part < parts; ++part) v = p.merge(v, p.load(part, sl), k);
      p.store((int64_t)blockIdx.x * lay.n_slots + sb + sl, v, k);
    }
    __syncthreads();  // the next stream reuses the LDS
  }
}

}  // namespace nqa
