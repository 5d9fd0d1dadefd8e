// Cell-list neighbour list on the device (the caller-side step immediately before the hot path).
//
// Replaces _compute_neighborlist_single_frame (nequip/data/_nl.py:63-165), which hands the positions to a CPU library
// (matscipy `neighbour_list("ijS", ...)` by default) and copies the result back: all ordered pairs (i, j, S) with
//     | pos[j] - pos[i] + S @ cell | < r_max,      excluding i == j with S == 0,
// `edge_index[0] = i` (the convolution centre), `edge_index[1] = j`, S integer lattice shifts (0 along non-periodic
// directions), positions anywhere (not necessarily inside the cell), any triclinic cell, cells smaller than the cutoff
// (several images of the same atom), mixed periodicity.
//
// Device algorithm (float64 throughout, like the reference libraries):
//   1. plan   : fractional coordinates s = pos @ cell^-1; periodic directions are wrapped into [0,1) (the integer part is
//               remembered per atom), non-periodic ones get a bounding box.  Bins per direction = floor(extent / r_max)
//               (>= 1, coarsened until the grid fits the workspace), so a bin is at least r_max thick unless the whole
//               cell is thinner -- then ceil(r_max / thickness) bins/images are searched on either side.
//   2. bin    : bin id per atom and a histogram of the bins (the atomic's return value = the atom's arrival slot in its bin);
//               prefix sum over the bins; atoms dropped into their bins by arrival slot; one wavefront per bin then puts its
//               atoms in ascending order (rank sort: a bin holds ~10 atoms) and gathers their coordinates.  The arrival
//               order is arbitrary, the result is not: bins hold their atoms in ascending index order.
//   3. count  : one wavefront per atom walks the (2R+1)^3 neighbouring bins (with image bookkeeping), 64 candidates at a
//               time (ballot + population count), counts hits;
//               exclusive scan -> rowptr.  The host reads rowptr[N] (the one unavoidable synchronisation: E is data
//               dependent) and allocates the outputs.
//   4. fill   : same walk, writes (i, j, S) at rowptr[i] + k.  Edges come out grouped by centre atom in ascending order
//               (= the dst-sorted order the tensor-product kernels want) and deterministically ordered within an atom.
//
// Forms of the list: F frames in one pass (the batched list: one header per frame, B = N + 8 F bins), T atom types with a cutoff
// per (centre type, neighbour type) (the typed list: two more workspace fields), a fixed number of edge slots (the
// capacity-padded fill).  They share the workspace layout (nl_layout(N, F, T), below) and the host code: one count driver and one
// fill driver at the end of this file, where the table of the entry points is.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "nequip_amd.h"
#include "plan.h"

namespace nqa {

struct NLHeader {
  double cell[9];   // rows = lattice vectors (identity for a missing cell)
  double inv[9];    // cell^-1 (s = pos @ inv)
  double lo[3];     // fractional origin of the grid per direction (0 for periodic ones)
  double width[3];  // fractional width of one bin
  int32_t nb[3];    // bins per direction
  int32_t reach[3]; // bins searched on either side
  int32_t pbc[3];
  int32_t nbins;    // nb[0]*nb[1]*nb[2]
  double rmax2;
  int32_t pad_axis;  // capacity-padded lists: padding edges are self images (i <- i) shifted by +-(pad_k0 + t) cells along
  int32_t pad_k0;    // this lattice vector, pad_k0 * |a| > r_max: longer than the cutoff, so they carry no interaction
};

// Workspace layout of every form of the list (all offsets 256-byte aligned): N atoms; F frames (0: the single-frame list, one
// header, B = N + 8 bins; F >= 1: the batched list, one header per frame, B = N + 8 F bins, plus bin_off and atom_frame);
// T atom types (0: untyped; T >= 1: plus type_sorted and rc2 behind everything else, so a typed workspace begins with the
// untyped one).  NL_ABSENT marks a field the form does not have.
constexpr int64_t NL_ABSENT = -1;

struct NLLayout {
  int64_t header, bin_off, atom_frame, sfrac, ioff, key, val, bin_count, rowptr_bin, atom_sorted, atom_arrival, s_sorted,
      o_sorted, counts, type_sorted, rc2, total;
};

static int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

static NLLayout nl_layout(int64_t N, int64_t F, int64_t T) {
  const int64_t frames = F > 0 ? F : 1, B = N + 8 * frames;
  NLLayout L{};
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    const int64_t o = off;
    off = align256(off + bytes);
    return o;
  };
  L.header = take(frames * (int64_t)sizeof(NLHeader));
  L.bin_off = F > 0 ? take(F * 4) : NL_ABSENT;     // first bin of every frame
  L.atom_frame = F > 0 ? take(N * 4) : NL_ABSENT;  // frame of every atom
  L.sfrac = take(N * 3 * 8);                       // wrapped fractional coordinates
  L.ioff = take(N * 3 * 4);                        // integer parts removed by the wrapping
  L.key = take(N * 4);                             // bin id per atom
  L.val = take(N * 4);                             // arrival slot of the atom in its bin
  L.bin_count = take((B + 1) * 4);                 // atoms per bin (zeroed by the plan kernel)
  L.rowptr_bin = take((B + 1) * 4);
  L.atom_sorted = take(N * 4);                     // atom indices in bin order, ascending within a bin
  L.atom_arrival = take(N * 4);                    // atom indices in bin order, arrival order within a bin
  L.s_sorted = take(N * 3 * 8);
  L.o_sorted = take(N * 3 * 4);
  L.counts = take((N + 1) * 4);
  L.type_sorted = T > 0 ? take(N * 4) : NL_ABSENT;  // type of atom_sorted[k]: read coalesced by the walk, next to s_sorted
  L.rc2 = T > 0 ? take(T * T * 8) : NL_ABSENT;      // squared cutoffs [T, T], formed once per count
  L.total = off;
  return L;
}

// The workspace as typed pointers (nullptr for an absent field): the one place where a layout offset becomes a pointer.  The
// fills only read through it.
struct NLWork {
  NLHeader* hdr;
  int32_t *bin_off, *atom_frame;
  double* sfrac;
  int32_t *ioff, *key, *val, *bin_count, *rowptr_bin, *atom_sorted, *atom_arrival;
  double* s_sorted;
  int32_t *o_sorted, *counts, *type_sorted;
  double* rc2;
};

template <typename T>
static T* nl_at(char* w, int64_t offset) {
  return offset == NL_ABSENT ? nullptr : reinterpret_cast<T*>(w + offset);
}

static NLWork nl_work(const void* workspace, const NLLayout& L) {
  char* w = static_cast<char*>(const_cast<void*>(workspace));
  NLWork W{};
  W.hdr = nl_at<NLHeader>(w, L.header);
  W.bin_off = nl_at<int32_t>(w, L.bin_off);
  W.atom_frame = nl_at<int32_t>(w, L.atom_frame);
  W.sfrac = nl_at<double>(w, L.sfrac);
  W.ioff = nl_at<int32_t>(w, L.ioff);
  W.key = nl_at<int32_t>(w, L.key);
  W.val = nl_at<int32_t>(w, L.val);
  W.bin_count = nl_at<int32_t>(w, L.bin_count);
  W.rowptr_bin = nl_at<int32_t>(w, L.rowptr_bin);
  W.atom_sorted = nl_at<int32_t>(w, L.atom_sorted);
  W.atom_arrival = nl_at<int32_t>(w, L.atom_arrival);
  W.s_sorted = nl_at<double>(w, L.s_sorted);
  W.o_sorted = nl_at<int32_t>(w, L.o_sorted);
  W.counts = nl_at<int32_t>(w, L.counts);
  W.type_sorted = nl_at<int32_t>(w, L.type_sorted);
  W.rc2 = nl_at<double>(w, L.rc2);
  return W;
}

__device__ __forceinline__ void inv3(const double* c, double* inv) {
  const double det = c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) +
                     c[2] * (c[3] * c[7] - c[4] * c[6]);
  const double r = 1.0 / det;
  inv[0] = (c[4] * c[8] - c[5] * c[7]) * r;
  inv[1] = (c[2] * c[7] - c[1] * c[8]) * r;
  inv[2] = (c[1] * c[5] - c[2] * c[4]) * r;
  inv[3] = (c[5] * c[6] - c[3] * c[8]) * r;
  inv[4] = (c[0] * c[8] - c[2] * c[6]) * r;
  inv[5] = (c[2] * c[3] - c[0] * c[5]) * r;
  inv[6] = (c[3] * c[7] - c[4] * c[6]) * r;
  inv[7] = (c[1] * c[6] - c[0] * c[7]) * r;
  inv[8] = (c[0] * c[4] - c[1] * c[3]) * r;
}

// Thread-0 part of a plan: header of one frame from its (completed) cell, its inverse and the bounding box [mn, mx] of its
// fractional coordinates.  Shared by the single-frame and the batched plan, so a frame gets the same grid in both.
__device__ void nl_size_grid(const double* c, const double* inv, const double* mn, const double* mx,
                             const int32_t* __restrict__ pbc, double r_max, int64_t N, int64_t bin_capacity,
                             NLHeader* __restrict__ h) {
  for (int i = 0; i < 9; ++i) {
    h->cell[i] = c[i];
    h->inv[i] = inv[i];
  }
  // perpendicular height of the cell along direction d = 1 / | column d of cell^-1 |
  int64_t nb[3];
  double heights[3];
  for (int d = 0; d < 3; ++d) {
    const double height = 1.0 / sqrt(inv[d] * inv[d] + inv[3 + d] * inv[3 + d] + inv[6 + d] * inv[6 + d]);
    const bool per = pbc != nullptr && pbc[d] != 0;
    h->pbc[d] = per ? 1 : 0;
    double lo, extent;  // fractional
    if (per) {
      lo = 0.0;
      extent = 1.0;
    } else {
      lo = N > 0 ? mn[d] : 0.0;
      extent = N > 0 ? (mx[d] - mn[d]) : 0.0;
      extent = extent * (1.0 + 1e-9) + 1e-9;  // the topmost atom must fall inside the last bin
    }
    int64_t n = (int64_t)floor(extent * height / r_max);
    if (n < 1) n = 1;
    if (n > 1024) n = 1024;
    nb[d] = n;
    h->lo[d] = lo;
    h->width[d] = extent;  // divided by nb below
    h->reach[d] = 0;       // filled below (needs the final nb)
    heights[d] = height;
  }
  while (nb[0] * nb[1] * nb[2] > bin_capacity) {  // coarser bins are always valid
    int big = 0;
    if (nb[1] > nb[big]) big = 1;
    if (nb[2] > nb[big]) big = 2;
    nb[big] = (nb[big] + 1) / 2;
  }
  for (int d = 0; d < 3; ++d) {
    const double height = heights[d];
    const double extent = h->width[d];
    h->nb[d] = (int32_t)nb[d];
    h->width[d] = extent / (double)nb[d];
    const double thick = h->width[d] * height;  // real-space thickness of one bin
    int reach = (int)ceil(r_max / thick);
    if (!h->pbc[d] && reach > nb[d] - 1) reach = (int)(nb[d] - 1);  // nothing beyond the box
    h->reach[d] = reach;
  }
  h->nbins = (int32_t)(nb[0] * nb[1] * nb[2]);
  h->rmax2 = r_max * r_max;
  // padding edges (nqa_neighbor_list_fill_padded): the shortest lattice vector among the periodic directions (any direction
  // when there is none), repeated often enough to leave the cutoff sphere
  int axis = -1;
  double best = 0.0;
  for (int pass = 0; pass < 2 && axis < 0; ++pass) {
    for (int d = 0; d < 3; ++d) {
      if (pass == 0 && !h->pbc[d]) continue;
      const double len = sqrt(c[3 * d] * c[3 * d] + c[3 * d + 1] * c[3 * d + 1] + c[3 * d + 2] * c[3 * d + 2]);
      if (axis < 0 || len < best) {
        axis = d;
        best = len;
      }
    }
  }
  h->pad_axis = axis;
  h->pad_k0 = (int32_t)floor(r_max / best) + 1;
}

// One workgroup: bounding box of the fractional coordinates, then thread 0 sizes the grid.
__global__ __launch_bounds__(1024) void nl_plan_kernel(const double* __restrict__ pos, const double* __restrict__ cell,
                                                       const int32_t* __restrict__ pbc, double r_max, int64_t N,
                                                       int64_t bin_capacity, NLHeader* __restrict__ h,
                                                       int32_t* __restrict__ bin_count) {
  __shared__ double smin[3][1024], smax[3][1024];
  for (int64_t b = threadIdx.x; b <= bin_capacity; b += 1024) bin_count[b] = 0;
  __shared__ double c[9], inv[9];
  const int tid = threadIdx.x;
  if (tid == 0) {
    bool any = false;
    for (int i = 0; i < 9; ++i) {
      c[i] = cell ? cell[i] : 0.0;
      any = any || c[i] != 0.0;
    }
    // ase.geometry.complete_cell analogue for the cases the reference meets here: a missing / all-zero cell becomes the
    // identity (only legal without periodicity)
    if (!any) {
      for (int i = 0; i < 9; ++i) c[i] = (i % 4 == 0) ? 1.0 : 0.0;
    }
    inv3(c, inv);
  }
  __syncthreads();
  double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
  for (int64_t i = tid; i < N; i += 1024) {
    const double x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
    for (int d = 0; d < 3; ++d) {
      const double s = x * inv[d] + y * inv[3 + d] + z * inv[6 + d];
      mn[d] = fmin(mn[d], s);
      mx[d] = fmax(mx[d], s);
    }
  }
  for (int d = 0; d < 3; ++d) {
    smin[d][tid] = mn[d];
    smax[d][tid] = mx[d];
  }
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if (tid < off) {
      for (int d = 0; d < 3; ++d) {
        smin[d][tid] = fmin(smin[d][tid], smin[d][tid + off]);
        smax[d][tid] = fmax(smax[d][tid], smax[d][tid + off]);
      }
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const double mn0[3] = {smin[0][0], smin[1][0], smin[2][0]}, mx0[3] = {smax[0][0], smax[1][0], smax[2][0]};
  nl_size_grid(c, inv, mn0, mx0, pbc, r_max, N, bin_capacity, h);
}

// Bin of atom i in the grid `h` (global bin id = bin_base + bin within the grid); fractional coordinates wrapped along periodic
// directions, the integer parts kept in ioff.
__device__ __forceinline__ void nl_bin_atom(int64_t i, const double* __restrict__ pos, const NLHeader* __restrict__ h,
                                            int32_t bin_base, double* __restrict__ sfrac, int32_t* __restrict__ ioff,
                                            int32_t* __restrict__ key, int32_t* __restrict__ val,
                                            int32_t* __restrict__ bin_count) {
  const double x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
  int b[3];
  for (int d = 0; d < 3; ++d) {
    double s = x * h->inv[d] + y * h->inv[3 + d] + z * h->inv[6 + d];
    int o = 0;
    if (h->pbc[d]) {
      const double fl = floor(s);
      o = (int)fl;
      s -= fl;
      if (s >= 1.0) {  // s was -epsilon: rounds to 1.0
        s -= 1.0;
        o += 1;
      }
    }
    int bi = (int)floor((s - h->lo[d]) / h->width[d]);
    if (bi < 0) bi = 0;
    if (bi > h->nb[d] - 1) bi = h->nb[d] - 1;
    b[d] = bi;
    sfrac[3 * i + d] = s;
    ioff[3 * i + d] = o;
  }
  const int32_t bin = bin_base + (b[0] * h->nb[1] + b[1]) * h->nb[2] + b[2];
  key[i] = bin;
  val[i] = atomicAdd(&bin_count[bin], 1);
}

__global__ __launch_bounds__(256) void nl_bin_kernel(const double* __restrict__ pos, int64_t N,
                                                     const NLHeader* __restrict__ h, double* __restrict__ sfrac,
                                                     int32_t* __restrict__ ioff, int32_t* __restrict__ key,
                                                     int32_t* __restrict__ val, int32_t* __restrict__ bin_count) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  nl_bin_atom(i, pos, h, 0, sfrac, ioff, key, val, bin_count);
}

__global__ __launch_bounds__(256) void nl_place_kernel(int64_t N, const int32_t* __restrict__ key,
                                                       const int32_t* __restrict__ val,
                                                       const int32_t* __restrict__ rowptr_bin,
                                                       int32_t* __restrict__ atom_arrival) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < N) atom_arrival[rowptr_bin[key[i]] + val[i]] = (int32_t)i;
}

// One wavefront per bin: rank of every atom of the bin among the bin's atom indices = its final position; coordinates follow.
__global__ __launch_bounds__(256) void nl_order_kernel(int64_t B, const int32_t* __restrict__ rowptr_bin,
                                                       const int32_t* __restrict__ atom_arrival,
                                                       const double* __restrict__ sfrac, const int32_t* __restrict__ ioff,
                                                       int32_t* __restrict__ atom_sorted, double* __restrict__ s_sorted,
                                                       int32_t* __restrict__ o_sorted) {
  const int64_t b = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  const int k0 = rowptr_bin[b], k1 = rowptr_bin[b + 1];
  for (int kb = k0; kb < k1; kb += 64) {
    const int k = kb + lane;
    const int a = k < k1 ? atom_arrival[k] : 0x7fffffff;
    int rank = 0;
    for (int t = k0; t < k1; ++t) rank += atom_arrival[t] < a ? 1 : 0;
    if (k < k1) {
      const int pos = k0 + rank;
      atom_sorted[pos] = a;
      for (int d = 0; d < 3; ++d) {
        s_sorted[3 * (int64_t)pos + d] = sfrac[3 * (int64_t)a + d];
        o_sorted[3 * (int64_t)pos + d] = ioff[3 * (int64_t)a + d];
      }
    }
  }
}

// Shared walk of count and fill, one WAVEFRONT per atom: the neighbouring bins are visited in a fixed order and the atoms of a
// bin are tested 64 at a time, one per lane; a hit's position in the atom's edge row is the number of hits before it (ballot +
// population count), i.e. exactly the order in which a single thread walking the same bins would emit them.
// FILL == false: returns the number of neighbours of atom i (the same value in every lane).
// TYPED: a candidate must also lie within the cutoff of its (centre type, neighbour type) pair, r2 <= rc2_row[type_j]: the test
// is part of the one `hit` expression, so count and fill agree and the typed list is the untyped one with edges removed.
// rc2_row = the centre type's row of squared cutoffs (wavefront-uniform), type_sorted = neighbour types in bin order, both
// already forced into range by nl_typed_prep_kernel.
template <bool FILL, bool TYPED = false>
__device__ __forceinline__ int nl_walk(int64_t i, int lane, const NLHeader* __restrict__ h, const double* __restrict__ sfrac,
                                       const int32_t* __restrict__ ioff, const int32_t* __restrict__ rowptr_bin,
                                       const int32_t* __restrict__ atom_sorted, const double* __restrict__ s_sorted,
                                       const int32_t* __restrict__ o_sorted, int64_t base, int64_t E,
                                       int64_t* __restrict__ edge_index, double* __restrict__ shift,
                                       int32_t* __restrict__ src32 = nullptr,
                                       const int32_t* __restrict__ type_sorted = nullptr,
                                       const double* __restrict__ rc2_row = nullptr) {
  const double si[3] = {sfrac[3 * i], sfrac[3 * i + 1], sfrac[3 * i + 2]};
  const int oi[3] = {ioff[3 * i], ioff[3 * i + 1], ioff[3 * i + 2]};
  int bi[3];
  for (int d = 0; d < 3; ++d) {
    int b = (int)floor((si[d] - h->lo[d]) / h->width[d]);
    b = b < 0 ? 0 : (b > h->nb[d] - 1 ? h->nb[d] - 1 : b);
    bi[d] = b;
  }
  const double* __restrict__ c = h->cell;
  int cnt = 0;
  for (int dx = -h->reach[0]; dx <= h->reach[0]; ++dx) {
    int bx = bi[0] + dx, nx = 0;
    if (h->pbc[0]) {
      nx = (bx >= 0) ? bx / h->nb[0] : -((-bx + h->nb[0] - 1) / h->nb[0]);
      bx -= nx * h->nb[0];
    } else if (bx < 0 || bx >= h->nb[0]) {
      continue;
    }
    for (int dy = -h->reach[1]; dy <= h->reach[1]; ++dy) {
      int by = bi[1] + dy, ny = 0;
      if (h->pbc[1]) {
        ny = (by >= 0) ? by / h->nb[1] : -((-by + h->nb[1] - 1) / h->nb[1]);
        by -= ny * h->nb[1];
      } else if (by < 0 || by >= h->nb[1]) {
        continue;
      }
      // bins that follow each other along z lie next to each other in the sorted atom array: the z range is walked as runs
      // of bins of one periodic image (one run, two across a cell boundary, more only for cells thinner than the cutoff), 64
      // candidates of a run at a time -- the same candidate order as bin by bin, with fuller wavefronts
      int z = bi[2] - h->reach[2], zhi = bi[2] + h->reach[2];
      if (!h->pbc[2]) {
        z = z < 0 ? 0 : z;
        zhi = zhi > h->nb[2] - 1 ? h->nb[2] - 1 : zhi;
      }
      while (z <= zhi) {
        int nz = 0;
        if (h->pbc[2]) nz = (z >= 0) ? z / h->nb[2] : -((-z + h->nb[2] - 1) / h->nb[2]);
        int zend = (nz + 1) * h->nb[2] - 1;  // last bin of this image
        zend = zend < zhi ? zend : zhi;
        const int64_t row = ((int64_t)bx * h->nb[1] + by) * h->nb[2] - (int64_t)nz * h->nb[2];
        const int k1 = rowptr_bin[row + zend + 1];
        for (int kb = rowptr_bin[row + z]; kb < k1; kb += 64) {
          const int k = kb + lane;
          bool hit = false;
          int j = 0;
          if (k < k1) {
            // (s_j - s_i) + n: the reverse edge computes (s_i - s_j) - n, the exact negative in floating point, so both
            // directions of a pair see the SAME squared length and the list is symmetric by construction
            const double fx = (s_sorted[3 * k] - si[0]) + nx;
            const double fy = (s_sorted[3 * k + 1] - si[1]) + ny;
            const double fz = (s_sorted[3 * k + 2] - si[2]) + nz;
            const double rx = fx * c[0] + fy * c[3] + fz * c[6];
            const double ry = fx * c[1] + fy * c[4] + fz * c[7];
            const double rz = fx * c[2] + fy * c[5] + fz * c[8];
            const double r2 = rx * rx + ry * ry + rz * rz;
            j = atom_sorted[k];
            hit = (r2 < h->rmax2) && !(j == i && nx == 0 && ny == 0 && nz == 0);
            if (TYPED) hit = hit && r2 <= rc2_row[type_sorted[k]];
          }
          const uint64_t m = __builtin_amdgcn_ballot_w64(hit);
          if (FILL && hit) {
            const int64_t e = base + cnt + __popcll(m & ((1ull << lane) - 1ull));
            edge_index[e] = i;
            edge_index[E + e] = j;
            if (src32 != nullptr) src32[e] = j;
            // pos_j - pos_i + S @ cell = (s_j + n - s_i) @ cell with pos = (s + o) @ cell  =>  S = n - o_j + o_i
            shift[3 * e + 0] = (double)(nx - o_sorted[3 * k] + oi[0]);
            shift[3 * e + 1] = (double)(ny - o_sorted[3 * k + 1] + oi[1]);
            shift[3 * e + 2] = (double)(nz - o_sorted[3 * k + 2] + oi[2]);
          }
          cnt += __popcll(m);
        }
        z = zend + 1;
      }
    }
  }
  return cnt;
}

__global__ __launch_bounds__(256) void nl_count_kernel(int64_t N, const NLHeader* __restrict__ h,
                                                       const double* __restrict__ sfrac, const int32_t* __restrict__ ioff,
                                                       const int32_t* __restrict__ rowptr_bin,
                                                       const int32_t* __restrict__ atom_sorted,
                                                       const double* __restrict__ s_sorted,
                                                       const int32_t* __restrict__ o_sorted, int32_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // one wavefront per atom
  if (i >= N) return;
  const int lane = threadIdx.x & 63;
  const int cnt = nl_walk<false>(i, lane, h, sfrac, ioff, rowptr_bin, atom_sorted, s_sorted, o_sorted, 0, 0, nullptr, nullptr);
  if (lane == 0) counts[i] = cnt;
}

// exclusive scan of counts[0..N) into rowptr[0..N], one workgroup: every thread sums a contiguous slice, the 1024 slice sums
// are scanned across the workgroup (wavefront shuffles + one pass over the 16 wavefront totals), every thread rewrites its slice
__global__ __launch_bounds__(1024) void nl_scan_kernel(int64_t N, const int32_t* __restrict__ counts,
                                                       int32_t* __restrict__ rowptr, int32_t* __restrict__ overflow) {
  __shared__ int64_t wave_total[16];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t per = (N + 1023) / 1024;
  const int64_t lo = tid * per < N ? tid * per : N, hi = lo + per < N ? lo + per : N;
  int64_t sum = 0;
  for (int64_t i = lo; i < hi; ++i) sum += counts[i];
  int64_t incl = sum;  // inclusive scan over the wavefront
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int64_t t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (lane == 63) wave_total[wv] = incl;
  __syncthreads();
  int64_t before = 0;
  for (int w = 0; w < wv; ++w) before += wave_total[w];
  int64_t run = before + incl - sum;
  for (int64_t i = lo; i < hi; ++i) {
    rowptr[i] = (int32_t)run;
    run += counts[i];
  }
  if (tid == 1023) {
    const int64_t total = before + incl;
    rowptr[N] = (int32_t)total;
    if (total > 2147483647LL && overflow != nullptr) *overflow |= 1;
  }
}

__global__ __launch_bounds__(256) void nl_fill_kernel(int64_t N, int64_t E, const NLHeader* __restrict__ h,
                                                      const double* __restrict__ sfrac, const int32_t* __restrict__ ioff,
                                                      const int32_t* __restrict__ rowptr_bin,
                                                      const int32_t* __restrict__ atom_sorted,
                                                      const double* __restrict__ s_sorted,
                                                      const int32_t* __restrict__ o_sorted,
                                                      const int32_t* __restrict__ rowptr, int64_t* __restrict__ edge_index,
                                                      double* __restrict__ shift) {
  const int64_t i = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // one wavefront per atom
  if (i >= N) return;
  nl_walk<true>(i, (int)(threadIdx.x & 63), h, sfrac, ioff, rowptr_bin, atom_sorted, s_sorted, o_sorted, rowptr[i], E,
                edge_index, shift);
}

// ---- capacity-padded list (no host read-back of the edge count: the whole MD step can live in one hipGraph) -----------------
// E_cap - E_real padding edges (E_cap even) are dealt out to the atoms as self-image PAIRS (i <- i, +S_t), (i <- i, -S_t),
// S_t = (pad_k0 + t) cells along pad_axis: atom i gets q + (i < rem) pairs, q = pairs / N, rem = pairs % N, behind its real
// edges.  They are longer than r_max, i.e. outside the polynomial cutoff: zero radial embedding, zero weights (the radial MLP is
// bias-free), zero derivative.  A list that does not fit (E_real > E_cap, or E_cap - E_real odd) is replaced by padding only
// and reported through status[0]: every index stays in range, the caller re-runs with a larger capacity.
struct NLPadPlan {
  bool bad;
  int64_t q, rem;
};
__device__ __forceinline__ NLPadPlan nl_pad_plan(const int32_t* __restrict__ rowptr, int64_t N, int64_t E_cap) {
  const int64_t E_real = rowptr[N];
  int64_t tail = E_cap - E_real;
  NLPadPlan p;
  p.bad = tail < 0 || (tail & 1) != 0;
  if (p.bad) tail = E_cap;
  const int64_t pairs = tail / 2;
  p.q = pairs / N;
  p.rem = pairs % N;
  return p;
}
__device__ __forceinline__ int64_t nl_pads_before(const NLPadPlan& p, int64_t i) { return 2 * (i * p.q + (i < p.rem ? i : p.rem)); }

__global__ __launch_bounds__(256) void nl_pad_rowptr_kernel(int64_t N, int64_t E_cap, const int32_t* __restrict__ rowptr,
                                                            int32_t* __restrict__ rowptr_out, int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > N) return;
  const NLPadPlan p = nl_pad_plan(rowptr, N, E_cap);
  rowptr_out[i] = (int32_t)((p.bad ? 0 : (int64_t)rowptr[i]) + nl_pads_before(p, i));
  if (i == 0 && status != nullptr) {
    status[0] = p.bad ? 1 : 0;
    status[1] = rowptr[N];
  }
}

__global__ __launch_bounds__(256) void nl_fill_padded_kernel(int64_t N, int64_t E_cap, const NLHeader* __restrict__ h,
                                                             const double* __restrict__ sfrac, const int32_t* __restrict__ ioff,
                                                             const int32_t* __restrict__ rowptr_bin,
                                                             const int32_t* __restrict__ atom_sorted,
                                                             const double* __restrict__ s_sorted,
                                                             const int32_t* __restrict__ o_sorted,
                                                             const int32_t* __restrict__ rowptr,
                                                             int64_t* __restrict__ edge_index, double* __restrict__ shift,
                                                             int32_t* __restrict__ src32) {
  const int64_t i = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // one wavefront per atom
  if (i >= N) return;
  const int lane = threadIdx.x & 63;
  const NLPadPlan p = nl_pad_plan(rowptr, N, E_cap);
  const int64_t base = (p.bad ? 0 : (int64_t)rowptr[i]) + nl_pads_before(p, i);
  int cnt = 0;
  if (!p.bad)
    cnt = nl_walk<true>(i, lane, h, sfrac, ioff, rowptr_bin, atom_sorted, s_sorted, o_sorted, base, E_cap, edge_index, shift,
                        src32);
  const int64_t npad = p.q + (i < p.rem ? 1 : 0);
  const int axis = h->pad_axis;
  for (int64_t t = lane; t < npad; t += 64) {
    const double k = (double)(h->pad_k0 + t);
    for (int sgn = 0; sgn < 2; ++sgn) {
      const int64_t e = base + cnt + 2 * t + sgn;
      edge_index[e] = i;
      edge_index[E_cap + e] = i;
      if (src32 != nullptr) src32[e] = (int32_t)i;
      for (int d = 0; d < 3; ++d) shift[3 * e + d] = d == axis ? (sgn ? -k : k) : 0.0;
    }
  }
}

// ---- batched list: F frames in one set of launches, one host read per batch ------------------------------------------------
// Frame f owns the atoms [frame_ptr[f], frame_ptr[f+1]) and the bins [bin_off[f], bin_off[f] + n_f + 8), bin_off[f] =
// frame_ptr[f] + 8 f: the bin budget the single-frame plan gives a frame of n_f atoms, so every frame is coarsened by the same
// rule and gets the same grid, the same bin order of its atoms and therefore the same edge order as the single-frame list.  The
// bins of all frames are contiguous, so ONE scan over the N + 8F bins sorts the whole batch by (frame, bin, atom index), and the
// count / fill walks of the single-frame list run unchanged, one wavefront per atom over the whole batch, on the header and the
// bin range of the atom's frame.  Atom indices stay global: edges never leave their frame (a frame's bins hold only its atoms).
enum : int32_t {
  NL_BAD_OVERFLOW = 1,        // more than 2^31 - 1 edges
  NL_BAD_PERIODIC_ZERO = 2,   // zero lattice vector along a periodic direction
  NL_BAD_DEPENDENT = 4,       // linearly dependent lattice vectors
  NL_BAD_FRAME_PTR = 8,       // frame_ptr is not a partition of [0, N)
  NL_BAD_PERIODIC_NO_CELL = 16,
  NL_BAD_TYPE = 32,           // typed lists: an atom type outside [0, num_types)
};

__device__ __forceinline__ int64_t nl_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// A device restatement of _complete_cell_host (nequip_amd/data/_nl.py), the ase.geometry.complete_cell analogue the single-frame
// path runs on the host: missing (zero) lattice vectors along non-periodic directions become unit vectors orthogonal to the
// present ones (Gram-Schmidt over the present vectors in index order; one missing: cross product of the two; two missing: the
// coordinate axis with the largest orthogonal component, then the cross product).  An all-zero cell becomes the identity.  Same
// steps in the same order, but not the same rounding: the host's dot products and norms go through numpy / BLAS, whose
// summation order and FMA use are not fixed, so a completed vector may differ from the host's by an ulp (complete cells and
// missing cells pass through unchanged, so only slabs and wires are affected).  Such a difference changes the list only for an
// atom within rounding of a bin face along the completed direction.  Returns NL_BAD_* flags (then c is the identity).
__device__ int32_t nl_complete_cell(double* c, const int32_t* __restrict__ pbc) {
#pragma clang fp contract(off)
  double norms[3];
  bool missing[3];
  int nmiss = 0;
  for (int i = 0; i < 3; ++i) {
    norms[i] = sqrt(c[3 * i] * c[3 * i] + c[3 * i + 1] * c[3 * i + 1] + c[3 * i + 2] * c[3 * i + 2]);
    missing[i] = norms[i] < 1e-12;
    nmiss += missing[i] ? 1 : 0;
  }
  auto det = [&]() {
    return c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6]);
  };
  auto identity = [&]() {
    for (int i = 0; i < 9; ++i) c[i] = (i % 4 == 0) ? 1.0 : 0.0;
  };
  int32_t bad = 0;
  if (nmiss == 0) {
    if (fabs(det()) < 1e-12 * fmax(1.0, norms[0] * norms[1] * norms[2])) bad = NL_BAD_DEPENDENT;
  } else {
    for (int i = 0; i < 3; ++i)
      if (missing[i] && pbc != nullptr && pbc[i] != 0) bad = NL_BAD_PERIODIC_ZERO;
    if (!bad && nmiss < 3) {
      double basis[3][3];
      int nb = 0;
      for (int i = 0; i < 3 && !bad; ++i) {
        if (missing[i]) continue;
        double v[3] = {c[3 * i], c[3 * i + 1], c[3 * i + 2]};
        for (int k = 0; k < nb; ++k) {
          const double d = v[0] * basis[k][0] + v[1] * basis[k][1] + v[2] * basis[k][2];
          for (int t = 0; t < 3; ++t) v[t] -= d * basis[k][t];
        }
        const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        if (n < 1e-12 * norms[i]) bad = NL_BAD_DEPENDENT;
        for (int t = 0; t < 3; ++t) basis[nb][t] = v[t] / n;
        ++nb;
      }
      for (int i = 0; i < 3 && !bad; ++i) {
        if (!missing[i]) continue;
        double v[3];
        if (nb == 2) {
          v[0] = basis[0][1] * basis[1][2] - basis[0][2] * basis[1][1];
          v[1] = basis[0][2] * basis[1][0] - basis[0][0] * basis[1][2];
          v[2] = basis[0][0] * basis[1][1] - basis[0][1] * basis[1][0];
        } else {
          double best = -1.0;
          for (int a = 0; a < 3; ++a) {
            double w[3] = {a == 0 ? 1.0 : 0.0, a == 1 ? 1.0 : 0.0, a == 2 ? 1.0 : 0.0};
            for (int k = 0; k < nb; ++k) {
              const double d = w[0] * basis[k][0] + w[1] * basis[k][1] + w[2] * basis[k][2];
              for (int t = 0; t < 3; ++t) w[t] -= d * basis[k][t];
            }
            const double n = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
            if (best < 0.0 || n > best) {
              best = n;
              for (int t = 0; t < 3; ++t) v[t] = w[t];
            }
          }
        }
        const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        for (int t = 0; t < 3; ++t) {
          c[3 * i + t] = v[t] / n;
          basis[nb][t] = v[t] / n;
        }
        ++nb;
      }
      if (!bad && fabs(det()) < 1e-12) bad = NL_BAD_DEPENDENT;
    } else if (!bad) {
      identity();
    }
  }
  if (bad) identity();  // a harmless grid for a frame the host rejects after the count
  return bad;
}

// One workgroup per frame: completes the frame's cell, zeroes its bins, reduces the bounding box of its fractional coordinates,
// then thread 0 sizes the frame's grid exactly as the single-frame plan does (nl_size_grid).
__global__ __launch_bounds__(256) void nl_batched_plan_kernel(const double* __restrict__ pos, const double* __restrict__ cell,
                                                              const int32_t* __restrict__ pbc,
                                                              const int64_t* __restrict__ frame_ptr, double r_max, int64_t N,
                                                              int64_t F, NLHeader* __restrict__ hdr,
                                                              int32_t* __restrict__ bin_off, int32_t* __restrict__ bin_count,
                                                              int32_t* __restrict__ status) {
  __shared__ double smin[3][256], smax[3][256];
  __shared__ double c[9], inv[9];
  __shared__ int32_t pbc_f[3];
  const int64_t f = blockIdx.x;
  const int tid = threadIdx.x;
  // Offsets clamped into [0, N], so every frame's bins lie inside [0, N + 8F) whatever frame_ptr holds (the host rejects a bad
  // frame_ptr after the count, from the status word).  Every bin count of [0, N + 8F] is zeroed even then: the frames' ranges
  // follow each other without gaps (a frame starts at or before the end of the previous one), block 0 zeroes the head in
  // front of frame 0 (frame_ptr[0] > 0) and block F-1 the tail behind the last frame (frame_ptr[F] < N).  The counts then sum
  // to N, so the bin scan, place and in-bin order stay inside their N-atom arrays.
  const int64_t a0 = nl_clamp(frame_ptr[f], 0, N), a1 = nl_clamp(frame_ptr[f + 1], a0, N);
  const int64_t boff = a0 + 8 * f, nbins = (a1 - a0) + 8;
  for (int64_t b = tid; b < nbins; b += 256) bin_count[boff + b] = 0;
  if (f == 0)
    for (int64_t b = tid; b < boff; b += 256) bin_count[b] = 0;
  if (f == F - 1)
    for (int64_t b = boff + nbins + tid; b <= N + 8 * F; b += 256) bin_count[b] = 0;
  if (tid == 0) {
    int32_t bad = 0;
    if (frame_ptr[f + 1] < frame_ptr[f] || (f == 0 && frame_ptr[0] != 0) || (f == F - 1 && frame_ptr[F] != N))
      bad |= NL_BAD_FRAME_PTR;
    for (int d = 0; d < 3; ++d) pbc_f[d] = pbc != nullptr ? pbc[3 * f + d] : 0;
    for (int i = 0; i < 9; ++i) c[i] = cell != nullptr ? cell[9 * f + i] : 0.0;
    if (cell == nullptr && (pbc_f[0] || pbc_f[1] || pbc_f[2])) bad |= NL_BAD_PERIODIC_NO_CELL;
    const int32_t cbad = nl_complete_cell(c, pbc_f);
    bad |= cbad;
    if (bad) pbc_f[0] = pbc_f[1] = pbc_f[2] = 0;
    inv3(c, inv);
    bin_off[f] = (int32_t)boff;
    if (bad) atomicOr(status, bad);
  }
  __syncthreads();
  double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
  for (int64_t i = a0 + tid; i < a1; i += 256) {
    const double x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
    for (int d = 0; d < 3; ++d) {
      const double s = x * inv[d] + y * inv[3 + d] + z * inv[6 + d];
      mn[d] = fmin(mn[d], s);
      mx[d] = fmax(mx[d], s);
    }
  }
  for (int d = 0; d < 3; ++d) {
    smin[d][tid] = mn[d];
    smax[d][tid] = mx[d];
  }
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      for (int d = 0; d < 3; ++d) {
        smin[d][tid] = fmin(smin[d][tid], smin[d][tid + off]);
        smax[d][tid] = fmax(smax[d][tid], smax[d][tid + off]);
      }
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const double mn0[3] = {smin[0][0], smin[1][0], smin[2][0]}, mx0[3] = {smax[0][0], smax[1][0], smax[2][0]};
  nl_size_grid(c, inv, mn0, mx0, pbc_f, r_max, a1 - a0, nbins, hdr + f);
}

// Frame of every atom (last f with frame_ptr[f] <= i, binary search over the F + 1 offsets), then the single-frame binning in
// that frame's grid and bin range.
__global__ __launch_bounds__(256) void nl_batched_bin_kernel(const double* __restrict__ pos, const int64_t* __restrict__ frame_ptr,
                                                             int64_t N, int64_t F, const NLHeader* __restrict__ hdr,
                                                             const int32_t* __restrict__ bin_off,
                                                             int32_t* __restrict__ atom_frame, double* __restrict__ sfrac,
                                                             int32_t* __restrict__ ioff, int32_t* __restrict__ key,
                                                             int32_t* __restrict__ val, int32_t* __restrict__ bin_count) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  int64_t lo = 0, hi = F - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (frame_ptr[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  atom_frame[i] = (int32_t)lo;
  nl_bin_atom(i, pos, hdr + lo, bin_off[lo], sfrac, ioff, key, val, bin_count);
}

__global__ __launch_bounds__(256) void nl_batched_count_kernel(int64_t N, const NLHeader* __restrict__ hdr,
                                                               const int32_t* __restrict__ bin_off,
                                                               const int32_t* __restrict__ atom_frame,
                                                               const double* __restrict__ sfrac,
                                                               const int32_t* __restrict__ ioff,
                                                               const int32_t* __restrict__ rowptr_bin,
                                                               const int32_t* __restrict__ atom_sorted,
                                                               const double* __restrict__ s_sorted,
                                                               const int32_t* __restrict__ o_sorted,
                                                               int32_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // one wavefront per atom
  if (i >= N) return;
  const int lane = threadIdx.x & 63;
  const int f = __builtin_amdgcn_readfirstlane(atom_frame[i]);
  const int cnt = nl_walk<false>(i, lane, hdr + f, sfrac, ioff, rowptr_bin + bin_off[f], atom_sorted, s_sorted, o_sorted, 0, 0,
                                 nullptr, nullptr);
  if (lane == 0) counts[i] = cnt;
}

__global__ __launch_bounds__(256) void nl_batched_fill_kernel(int64_t N, int64_t E, const NLHeader* __restrict__ hdr,
                                                              const int32_t* __restrict__ bin_off,
                                                              const int32_t* __restrict__ atom_frame,
                                                              const double* __restrict__ sfrac, const int32_t* __restrict__ ioff,
                                                              const int32_t* __restrict__ rowptr_bin,
                                                              const int32_t* __restrict__ atom_sorted,
                                                              const double* __restrict__ s_sorted,
                                                              const int32_t* __restrict__ o_sorted,
                                                              const int32_t* __restrict__ rowptr, int64_t* __restrict__ edge_index,
                                                              double* __restrict__ shift) {
  const int64_t i = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // one wavefront per atom
  if (i >= N) return;
  const int f = __builtin_amdgcn_readfirstlane(atom_frame[i]);
  nl_walk<true>(i, (int)(threadIdx.x & 63), hdr + f, sfrac, ioff, rowptr_bin + bin_off[f], atom_sorted, s_sorted, o_sorted,
                rowptr[i], E, edge_index, shift);
}

// ---- typed lists: per-(centre type, neighbour type) cutoffs ------------------------------------------------------------------
// The typed entry points run the untyped pipeline (plan, bin, order: the grid is the r_max grid, so the candidate order is that
// of the untyped list) and then walk with the extra test r2 <= rc[type_i][type_j]^2.  Their workspace is the untyped one
// followed by type_sorted int32 [N] and rc2 float64 [T, T] (nl_layout with T >= 1).

// rc2 = cutoff_table^2 (symmetrise: of max(rc[a][b], rc[b][a])) and type_sorted[k] = type of atom_sorted[k].  A type outside
// [0, T) is reported through `status` and replaced by 0, so that no walk ever indexes outside the table.
__global__ __launch_bounds__(256) void nl_typed_prep_kernel(int64_t N, int64_t T, const int64_t* __restrict__ atom_types,
                                                            const double* __restrict__ cutoff_table, int32_t symmetrise,
                                                            const int32_t* __restrict__ atom_sorted,
                                                            int32_t* __restrict__ type_sorted, double* __restrict__ rc2,
                                                            int32_t* __restrict__ status) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < T * T) {
    double rc = cutoff_table[k];
    if (symmetrise) rc = fmax(rc, cutoff_table[(k % T) * T + k / T]);
    rc2[k] = rc * rc;
  }
  if (k < N) {
    int64_t t = atom_types[atom_sorted[k]];
    if (t < 0 || t >= T) {
      atomicOr(status, NL_BAD_TYPE);
      t = 0;
    }
    type_sorted[k] = (int32_t)t;
  }
}

__device__ __forceinline__ const double* nl_rc2_row(const double* __restrict__ rc2, const int64_t* __restrict__ atom_types,
                                                    int64_t i, int64_t T) {
  int64_t t = atom_types[i];
  t = (t < 0 || t >= T) ? 0 : t;  // (reported by nl_typed_prep_kernel)
  const int ti = __builtin_amdgcn_readfirstlane((int)t);
  return rc2 + (int64_t)ti * T;
}

// atom_frame == nullptr: one frame (hdr, rowptr_bin as they are); otherwise the batched walk on the atom's frame.
__global__ __launch_bounds__(256) void nl_typed_count_kernel(int64_t N, const NLHeader* __restrict__ hdr,
                                                             const int32_t* __restrict__ bin_off,
                                                             const int32_t* __restrict__ atom_frame,
                                                             const double* __restrict__ sfrac, const int32_t* __restrict__ ioff,
                                                             const int32_t* __restrict__ rowptr_bin,
                                                             const int32_t* __restrict__ atom_sorted,
                                                             const double* __restrict__ s_sorted,
                                                             const int32_t* __restrict__ o_sorted,
                                                             const int64_t* __restrict__ atom_types, int64_t T,
                                                             const int32_t* __restrict__ type_sorted,
                                                             const double* __restrict__ rc2, int32_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // one wavefront per atom
  if (i >= N) return;
  const int lane = threadIdx.x & 63;
  if (atom_frame != nullptr) {
    const int f = __builtin_amdgcn_readfirstlane(atom_frame[i]);
    hdr += f;
    rowptr_bin += bin_off[f];
  }
  const int cnt = nl_walk<false, true>(i, lane, hdr, sfrac, ioff, rowptr_bin, atom_sorted, s_sorted, o_sorted, 0, 0, nullptr,
                                       nullptr, nullptr, type_sorted, nl_rc2_row(rc2, atom_types, i, T));
  if (lane == 0) counts[i] = cnt;
}

__global__ __launch_bounds__(256) void nl_typed_fill_kernel(int64_t N, int64_t E, const NLHeader* __restrict__ hdr,
                                                            const int32_t* __restrict__ bin_off,
                                                            const int32_t* __restrict__ atom_frame,
                                                            const double* __restrict__ sfrac, const int32_t* __restrict__ ioff,
                                                            const int32_t* __restrict__ rowptr_bin,
                                                            const int32_t* __restrict__ atom_sorted,
                                                            const double* __restrict__ s_sorted,
                                                            const int32_t* __restrict__ o_sorted,
                                                            const int64_t* __restrict__ atom_types, int64_t T,
                                                            const int32_t* __restrict__ type_sorted,
                                                            const double* __restrict__ rc2, const int32_t* __restrict__ rowptr,
                                                            int64_t* __restrict__ edge_index, double* __restrict__ shift) {
  const int64_t i = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // one wavefront per atom
  if (i >= N) return;
  if (atom_frame != nullptr) {
    const int f = __builtin_amdgcn_readfirstlane(atom_frame[i]);
    hdr += f;
    rowptr_bin += bin_off[f];
  }
  nl_walk<true, true>(i, (int)(threadIdx.x & 63), hdr, sfrac, ioff, rowptr_bin, atom_sorted, s_sorted, o_sorted, rowptr[i], E,
                      edge_index, shift, nullptr, type_sorted, nl_rc2_row(rc2, atom_types, i, T));
}

// nl_fill_padded_kernel with the typed walk (the padding edges are longer than r_max, hence beyond every type cutoff); its own
// copy of the kernel, padding loop included, so that the untyped kernel's text stays what it was.
__global__ __launch_bounds__(256) void nl_typed_fill_padded_kernel(
    int64_t N, int64_t E_cap, const NLHeader* __restrict__ h, const double* __restrict__ sfrac, const int32_t* __restrict__ ioff,
    const int32_t* __restrict__ rowptr_bin, const int32_t* __restrict__ atom_sorted, const double* __restrict__ s_sorted,
    const int32_t* __restrict__ o_sorted, const int64_t* __restrict__ atom_types, int64_t T,
    const int32_t* __restrict__ type_sorted, const double* __restrict__ rc2, const int32_t* __restrict__ rowptr,
    int64_t* __restrict__ edge_index, double* __restrict__ shift, int32_t* __restrict__ src32) {
  const int64_t i = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // one wavefront per atom
  if (i >= N) return;
  const int lane = threadIdx.x & 63;
  const NLPadPlan p = nl_pad_plan(rowptr, N, E_cap);
  const int64_t base = (p.bad ? 0 : (int64_t)rowptr[i]) + nl_pads_before(p, i);
  int cnt = 0;
  if (!p.bad)
    cnt = nl_walk<true, true>(i, lane, h, sfrac, ioff, rowptr_bin, atom_sorted, s_sorted, o_sorted, base, E_cap, edge_index,
                              shift, src32, type_sorted, nl_rc2_row(rc2, atom_types, i, T));
  const int64_t npad = p.q + (i < p.rem ? 1 : 0);
  const int axis = h->pad_axis;
  for (int64_t t = lane; t < npad; t += 64) {
    const double k = (double)(h->pad_k0 + t);
    for (int sgn = 0; sgn < 2; ++sgn) {
      const int64_t e = base + cnt + 2 * t + sgn;
      edge_index[e] = i;
      edge_index[E_cap + e] = i;
      if (src32 != nullptr) src32[e] = (int32_t)i;
      for (int d = 0; d < 3; ++d) shift[3 * e + d] = d == axis ? (sgn ? -k : k) : 0.0;
    }
  }
}

// ---- host side: one count driver and one fill driver behind the 14 entry points ---------------------------------------------
// Every entry point is a form of the same list; the optional operand groups (nullptr: absent) say which:
//
//   entry point                                   | batched (NLFrames) | typed (NLTyped) | padded (NLPadded)
//   nqa_neighbor_list_count                       |         -          |        -        |
//   nqa_neighbor_list_count_typed                 |         -          |        x        |
//   nqa_neighbor_list_batched_count               |         x          |        -        |
//   nqa_neighbor_list_batched_count_typed         |         x          |        x        |
//   nqa_neighbor_list_fill                        |         -          |        -        |        -
//   nqa_neighbor_list_fill_typed                  |         -          |        x        |        -
//   nqa_neighbor_list_fill_padded                 |         -          |        -        |        x
//   nqa_neighbor_list_fill_padded_typed           |         -          |        x        |        x
//   nqa_neighbor_list_batched_fill                |         x          |        -        |        -
//   nqa_neighbor_list_batched_fill_typed          |         x          |        x        |        -
//
// and the four *_workspace_bytes are nl_layout(N, F or 0, T or 0).total.  A padded list is filled after a single-frame count.
//
// Launches of a count, in order (N == 0: plan and the final scan only):
//   plan   nl_plan_kernel (1 x 1024)                  | batched: status word zeroed, nl_batched_plan_kernel (F x 256)
//   bin    nl_bin_kernel                              | batched: nl_batched_bin_kernel
//   scan of the B bins, place, order                  : the same kernels in every form
//   typed: nl_typed_prep_kernel, then nl_typed_count_kernel (bin_off = atom_frame = nullptr for one frame)
//   untyped: nl_count_kernel                          | batched: nl_batched_count_kernel
//   scan of the N counts into rowptr (sets the overflow bit where there is a status word)
// A fill is one launch of nl_fill_kernel, nl_batched_fill_kernel or nl_typed_fill_kernel (single and batched); a padded fill is
// nl_pad_rowptr_kernel and then nl_fill_padded_kernel or nl_typed_fill_padded_kernel.
static int nl_status(const char* fn) {
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    set_error(std::string(fn) + ": " + hipGetErrorString(err));
    return NQA_ERR_LAUNCH;
  }
  return NQA_OK;
}

// Frames of a batched list.  The fills read F only.
struct NLFrames {
  const int64_t* frame_ptr;
  int64_t F;
};

// Typed operands.  The fills read atom_types and T only.
struct NLTyped {
  const int64_t* atom_types;
  const double* cutoff_table;
  int64_t T;
  int32_t symmetrise;
};

// Outputs of a capacity-padded fill beside the edges.
struct NLPadded {
  int32_t* rowptr_padded;
  int32_t* src_sorted;
  int32_t* status;
};

static bool nl_num_types_ok(int64_t T) { return T >= 1 && T <= 32768; }

// `status`: required by the batched and the typed forms, nullptr for the plain single-frame count.  The batched forms zero it
// here, once the arguments are accepted; the single-frame typed entry point zeroes it before it comes here.
static int nl_count(const char* fn, const double* pos, const double* cell, const int32_t* pbc, double r_max, int64_t N,
                    void* workspace, int64_t workspace_bytes, int32_t* rowptr, int32_t* status, nqa_stream stream,
                    const NLFrames* fr, const NLTyped* ty) {
  bool ok = N >= 0 && r_max > 0.0 && rowptr && (N == 0 || pos) && (status || (!fr && !ty));
  if (fr) ok = ok && fr->F >= 1 && fr->F <= 2147483647LL && N + 8 * fr->F <= 2147483646LL && fr->frame_ptr;
  if (ty) ok = ok && ty->cutoff_table && nl_num_types_ok(ty->T) && (N == 0 || ty->atom_types);
  if (!ok) {
    set_error(std::string(fn) + ": invalid argument");
    return NQA_ERR_INVALID;
  }
  const int64_t F = fr ? fr->F : 0, B = N + 8 * (fr ? F : 1);
  const NLLayout L = nl_layout(N, F, ty ? ty->T : 0);
  if (!workspace || workspace_bytes < L.total) {
    set_error(std::string(fn) + ": workspace missing or too small");
    return NQA_ERR_WORKSPACE;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const NLWork W = nl_work(workspace, L);
  if (fr) {
    if (hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess) return nl_status(fn);
    hipLaunchKernelGGL(nl_batched_plan_kernel, dim3((unsigned)F), dim3(256), 0, s, pos, cell, pbc, fr->frame_ptr, r_max, N, F,
                       W.hdr, W.bin_off, W.bin_count, status);
  } else {
    hipLaunchKernelGGL(nl_plan_kernel, dim3(1), dim3(1024), 0, s, pos, cell, pbc, r_max, N, B, W.hdr, W.bin_count);
  }
  if (N > 0) {
    const unsigned g256 = (unsigned)((N + 255) / 256), g4 = (unsigned)((N + 3) / 4);
    if (fr)
      hipLaunchKernelGGL(nl_batched_bin_kernel, dim3(g256), dim3(256), 0, s, pos, fr->frame_ptr, N, F, W.hdr, W.bin_off,
                         W.atom_frame, W.sfrac, W.ioff, W.key, W.val, W.bin_count);
    else
      hipLaunchKernelGGL(nl_bin_kernel, dim3(g256), dim3(256), 0, s, pos, N, W.hdr, W.sfrac, W.ioff, W.key, W.val, W.bin_count);
    hipLaunchKernelGGL(nl_scan_kernel, dim3(1), dim3(1024), 0, s, B, W.bin_count, W.rowptr_bin, (int32_t*)nullptr);
    hipLaunchKernelGGL(nl_place_kernel, dim3(g256), dim3(256), 0, s, N, W.key, W.val, W.rowptr_bin, W.atom_arrival);
    hipLaunchKernelGGL(nl_order_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, B, W.rowptr_bin, W.atom_arrival, W.sfrac,
                       W.ioff, W.atom_sorted, W.s_sorted, W.o_sorted);
    if (ty) {
      const int64_t n = N > ty->T * ty->T ? N : ty->T * ty->T;
      hipLaunchKernelGGL(nl_typed_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, N, ty->T, ty->atom_types,
                         ty->cutoff_table, ty->symmetrise, W.atom_sorted, W.type_sorted, W.rc2, status);
      hipLaunchKernelGGL(nl_typed_count_kernel, dim3(g4), dim3(256), 0, s, N, W.hdr, W.bin_off, W.atom_frame, W.sfrac, W.ioff,
                         W.rowptr_bin, W.atom_sorted, W.s_sorted, W.o_sorted, ty->atom_types, ty->T, W.type_sorted, W.rc2,
                         W.counts);
    } else if (fr) {
      hipLaunchKernelGGL(nl_batched_count_kernel, dim3(g4), dim3(256), 0, s, N, W.hdr, W.bin_off, W.atom_frame, W.sfrac, W.ioff,
                         W.rowptr_bin, W.atom_sorted, W.s_sorted, W.o_sorted, W.counts);
    } else {
      hipLaunchKernelGGL(nl_count_kernel, dim3(g4), dim3(256), 0, s, N, W.hdr, W.sfrac, W.ioff, W.rowptr_bin, W.atom_sorted,
                         W.s_sorted, W.o_sorted, W.counts);
    }
  }
  hipLaunchKernelGGL(nl_scan_kernel, dim3(1), dim3(1024), 0, s, N, W.counts, rowptr, status);  // status |= 1 on overflow
  return nl_status(fn);
}

// `E`: the number of edges, or the (even) capacity of a padded list.
static int nl_fill(const char* fn, const void* workspace, const int32_t* rowptr, int64_t N, int64_t E, int64_t* edge_index,
                   double* shift, nqa_stream stream, const NLFrames* fr, const NLTyped* ty, const NLPadded* pad) {
  bool ok = workspace && rowptr && E >= 0 && (E == 0 || (edge_index && shift));
  if (fr) ok = ok && fr->F >= 1;
  if (ty) ok = ok && nl_num_types_ok(ty->T) && (N <= 0 || ty->atom_types);
  if (pad)
    ok = ok && N > 0 && (E & 1) == 0 && E <= 2147483646LL && pad->rowptr_padded;
  else
    ok = ok && N >= 0;
  if (!ok) {
    const char* needs = !pad ? "" : ty ? " (needs atoms, types and an even capacity below 2^31)"
                                       : " (needs atoms and an even capacity below 2^31)";
    set_error(std::string(fn) + ": invalid argument" + needs);
    return NQA_ERR_INVALID;
  }
  if (!pad && (N == 0 || E == 0)) return NQA_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const NLWork W = nl_work(workspace, nl_layout(N, fr ? fr->F : 0, ty ? ty->T : 0));
  const dim3 g4((unsigned)((N + 3) / 4));
  if (pad) {
    hipLaunchKernelGGL(nl_pad_rowptr_kernel, dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, s, N, E, rowptr,
                       pad->rowptr_padded, pad->status);
    if (ty)
      hipLaunchKernelGGL(nl_typed_fill_padded_kernel, g4, dim3(256), 0, s, N, E, W.hdr, W.sfrac, W.ioff, W.rowptr_bin,
                         W.atom_sorted, W.s_sorted, W.o_sorted, ty->atom_types, ty->T, W.type_sorted, W.rc2, rowptr, edge_index,
                         shift, pad->src_sorted);
    else
      hipLaunchKernelGGL(nl_fill_padded_kernel, g4, dim3(256), 0, s, N, E, W.hdr, W.sfrac, W.ioff, W.rowptr_bin, W.atom_sorted,
                         W.s_sorted, W.o_sorted, rowptr, edge_index, shift, pad->src_sorted);
  } else if (ty) {
    hipLaunchKernelGGL(nl_typed_fill_kernel, g4, dim3(256), 0, s, N, E, W.hdr, W.bin_off, W.atom_frame, W.sfrac, W.ioff,
                       W.rowptr_bin, W.atom_sorted, W.s_sorted, W.o_sorted, ty->atom_types, ty->T, W.type_sorted, W.rc2, rowptr,
                       edge_index, shift);
  } else if (fr) {
    hipLaunchKernelGGL(nl_batched_fill_kernel, g4, dim3(256), 0, s, N, E, W.hdr, W.bin_off, W.atom_frame, W.sfrac, W.ioff,
                       W.rowptr_bin, W.atom_sorted, W.s_sorted, W.o_sorted, rowptr, edge_index, shift);
  } else {
    hipLaunchKernelGGL(nl_fill_kernel, g4, dim3(256), 0, s, N, E, W.hdr, W.sfrac, W.ioff, W.rowptr_bin, W.atom_sorted,
                       W.s_sorted, W.o_sorted, rowptr, edge_index, shift);
  }
  return nl_status(fn);
}

}  // namespace nqa

using namespace nqa;

extern "C" {

int64_t nqa_neighbor_list_workspace_bytes(int64_t num_atoms) {
  if (num_atoms < 0) return -1;
  return nl_layout(num_atoms, 0, 0).total;
}

int64_t nqa_neighbor_list_typed_workspace_bytes(int64_t num_atoms, int64_t num_types) {
  if (num_atoms < 0 || !nl_num_types_ok(num_types)) return -1;
  return nl_layout(num_atoms, 0, num_types).total;
}

int64_t nqa_neighbor_list_batched_workspace_bytes(int64_t num_atoms, int64_t num_frames) {
  if (num_atoms < 0 || num_frames < 1) return -1;
  return nl_layout(num_atoms, num_frames, 0).total;
}

int64_t nqa_neighbor_list_batched_typed_workspace_bytes(int64_t num_atoms, int64_t num_frames, int64_t num_types) {
  if (num_atoms < 0 || num_frames < 1 || !nl_num_types_ok(num_types)) return -1;
  return nl_layout(num_atoms, num_frames, num_types).total;
}

int nqa_neighbor_list_count(const double* pos, const double* cell, const int32_t* pbc, double r_max, int64_t num_atoms,
                            void* workspace, int64_t workspace_bytes, int32_t* rowptr, nqa_stream stream) {
  return nl_count("nqa_neighbor_list_count", pos, cell, pbc, r_max, num_atoms, workspace, workspace_bytes, rowptr, nullptr,
                  stream, nullptr, nullptr);
}

int nqa_neighbor_list_count_typed(const double* pos, const double* cell, const int32_t* pbc, double r_max,
                                  const int64_t* atom_types, const double* cutoff_table, int64_t num_types, int32_t symmetrise,
                                  int64_t num_atoms, void* workspace, int64_t workspace_bytes, int32_t* rowptr, int32_t* status,
                                  nqa_stream stream) {
  const NLTyped ty{atom_types, cutoff_table, num_types, symmetrise};
  if (status != nullptr &&
      hipMemsetAsync(status, 0, sizeof(int32_t), static_cast<hipStream_t>(stream)) != hipSuccess)
    return nl_status("nqa_neighbor_list_count_typed");
  return nl_count("nqa_neighbor_list_count_typed", pos, cell, pbc, r_max, num_atoms, workspace, workspace_bytes, rowptr, status,
                  stream, nullptr, &ty);
}

int nqa_neighbor_list_batched_count(const double* pos, const double* cell, const int32_t* pbc, const int64_t* frame_ptr,
                                    double r_max, int64_t num_atoms, int64_t num_frames, void* workspace,
                                    int64_t workspace_bytes, int32_t* rowptr, int32_t* status, nqa_stream stream) {
  const NLFrames fr{frame_ptr, num_frames};
  return nl_count("nqa_neighbor_list_batched_count", pos, cell, pbc, r_max, num_atoms, workspace, workspace_bytes, rowptr, status,
                  stream, &fr, nullptr);
}

int nqa_neighbor_list_batched_count_typed(const double* pos, const double* cell, const int32_t* pbc, const int64_t* frame_ptr,
                                          double r_max, const int64_t* atom_types, const double* cutoff_table,
                                          int64_t num_types, int64_t num_atoms, int64_t num_frames, void* workspace,
                                          int64_t workspace_bytes, int32_t* rowptr, int32_t* status, nqa_stream stream) {
  const NLFrames fr{frame_ptr, num_frames};
  const NLTyped ty{atom_types, cutoff_table, num_types, 0};
  return nl_count("nqa_neighbor_list_batched_count_typed", pos, cell, pbc, r_max, num_atoms, workspace, workspace_bytes, rowptr,
                  status, stream, &fr, &ty);
}

int nqa_neighbor_list_fill(const void* workspace, const int32_t* rowptr, int64_t num_atoms, int64_t num_edges,
                           int64_t* edge_index, double* edge_cell_shift, nqa_stream stream) {
  return nl_fill("nqa_neighbor_list_fill", workspace, rowptr, num_atoms, num_edges, edge_index, edge_cell_shift, stream, nullptr,
                 nullptr, nullptr);
}

int nqa_neighbor_list_fill_typed(const void* workspace, const int32_t* rowptr, const int64_t* atom_types, int64_t num_atoms,
                                 int64_t num_types, int64_t num_edges, int64_t* edge_index, double* edge_cell_shift,
                                 nqa_stream stream) {
  const NLTyped ty{atom_types, nullptr, num_types, 0};
  return nl_fill("nqa_neighbor_list_fill_typed", workspace, rowptr, num_atoms, num_edges, edge_index, edge_cell_shift, stream,
                 nullptr, &ty, nullptr);
}

int nqa_neighbor_list_fill_padded(const void* workspace, const int32_t* rowptr, int64_t num_atoms, int64_t edge_capacity,
                                  int32_t* rowptr_padded, int64_t* edge_index, double* edge_cell_shift, int32_t* src_sorted,
                                  int32_t* status, nqa_stream stream) {
  const NLPadded pad{rowptr_padded, src_sorted, status};
  return nl_fill("nqa_neighbor_list_fill_padded", workspace, rowptr, num_atoms, edge_capacity, edge_index, edge_cell_shift,
                 stream, nullptr, nullptr, &pad);
}

int nqa_neighbor_list_fill_padded_typed(const void* workspace, const int32_t* rowptr, const int64_t* atom_types,
                                        int64_t num_atoms, int64_t num_types, int64_t edge_capacity, int32_t* rowptr_padded,
                                        int64_t* edge_index, double* edge_cell_shift, int32_t* src_sorted, int32_t* status,
                                        nqa_stream stream) {
  const NLTyped ty{atom_types, nullptr, num_types, 0};
  const NLPadded pad{rowptr_padded, src_sorted, status};
  return nl_fill("nqa_neighbor_list_fill_padded_typed", workspace, rowptr, num_atoms, edge_capacity, edge_index, edge_cell_shift,
                 stream, nullptr, &ty, &pad);
}

int nqa_neighbor_list_batched_fill(const void* workspace, const int32_t* rowptr, int64_t num_atoms, int64_t num_frames,
                                   int64_t num_edges, int64_t* edge_index, double* edge_cell_shift, nqa_stream stream) {
  const NLFrames fr{nullptr, num_frames};
  return nl_fill("nqa_neighbor_list_batched_fill", workspace, rowptr, num_atoms, num_edges, edge_index, edge_cell_shift, stream,
                 &fr, nullptr, nullptr);
}

int nqa_neighbor_list_batched_fill_typed(const void* workspace, const int32_t* rowptr, const int64_t* atom_types,
                                         int64_t num_atoms, int64_t num_frames, int64_t num_types, int64_t num_edges,
                                         int64_t* edge_index, double* edge_cell_shift, nqa_stream stream) {
  const NLFrames fr{nullptr, num_frames};
  const NLTyped ty{atom_types, nullptr, num_types, 0};
  return nl_fill("nqa_neighbor_list_batched_fill_typed", workspace, rowptr, num_atoms, num_edges, edge_index, edge_cell_shift,
                 stream, &fr, &ty, nullptr);
}

}  // extern "C"
