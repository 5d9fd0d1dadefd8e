// ZBL core-repulsion pair term (nequip/nn/pair_potential.py:230-389, _ZBL / ZBL) in one pass over the centre-atom CSR.
//
// Per edge e = (i <- j), r = |edge_vec_e|, u = r / rmax(type_i, type_j):
//   E_e = (0.5 qqr2e * Z_i Z_j / r) * psi(x) * cutoff(u),   x = (Z_i^0.23 + Z_j^0.23) r / 0.46850,
//   psi = sum_k c_k exp(d_k x)   (the LAMMPS pair_zbl constants),   cutoff = the PolynomialCutoff(p) polynomial masked by u < 1
// and the per-atom energy of centre i is pe_in[i] + sum_{e: centre(e) = i} E_e.
//
// Layout: 16 lanes per centre atom (four atoms per wavefront).  Lane s walks the atom's CSR row at slots s, s + 16, ... and
// the 16 partial sums are combined by a fixed xor tree: no atomics, and the summation order depends only on the CSR, so two
// evaluations of the same list give bit-identical per-atom energies.  The backward / second-order kernels walk the same rows
// and write each edge's row of the [E, 3] outputs once (every edge has exactly one centre).
//
// Precision (the reference's dtypes): everything is float64 except where the reference rounds to the model dtype -- Z and
// Z^0.23 come in as model-dtype values (a default-dtype buffer), the sum Z_i^0.23 + Z_j^0.23 is formed in the model dtype,
// and the cutoff polynomial (float64) is rounded to the model dtype before it multiplies the float64 energy; the first-order
// backward rounds that value's cotangent (g_pe * energy) to the model dtype as autograd does.  The second order is float64.
// Edges with u >= 1 (beyond the cutoff, padding edges of a fixed-capacity list) contribute an exact zero to every output.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "plan.h"

namespace nqa {

struct ZblArgs {
  const double* __restrict__ vec;        // [E, 3]
  const int32_t* __restrict__ rowptr;    // [N + 1] centre-atom CSR
  const int32_t* __restrict__ eid;       // [E] edge id per CSR slot
  const int32_t* __restrict__ nbr;       // [E] neighbour atom per CSR slot
  const int64_t* __restrict__ types;     // [N]
  const double* __restrict__ zt;         // [T, 2]: Z, Z^0.23 (model-dtype values)
  const double* __restrict__ rmax_edge;  // [E] per-edge 1/rmax or NULL
  const double* __restrict__ pe_in;      // fwd: [n_out] or NULL
  double* __restrict__ pe_out;           // fwd: [n_out]
  const double* __restrict__ g_pe;       // bwd / bwd_bwd: [n_out]
  const double* __restrict__ cot;        // bwd_bwd: [E, 3] cotangent of the edge-vector gradient
  double* __restrict__ g_vec;            // bwd: [E, 3];  bwd_bwd: second-order edge-vector gradient [E, 3] or NULL
  double* __restrict__ gg_pe;            // bwd_bwd: [n_out] or NULL
  const double* __restrict__ qq;         // one float64 on the device: 0.5 qqr2e (the module's buffer)
  double rmax_recip, p;
  int64_t N, n_out;
  int32_t f32;
};

struct ZblTerm {
  double e, d1, d2;  // E(r), dE/dr, d2E/dr2
  double dr_eng, eng, dcut;  // E' = dr_eng + eng * dcut: (d eng/dr) cut, the uncut energy, d cut/dr
};

// ORDER 0: e only; 1: e, d1; 2: e, d1, d2.  Operation order of the value as in _ZBL.forward / PolynomialCutoff.forward.
template <int ORDER>
__device__ __forceinline__ ZblTerm zbl_term(double r, double zi, double pzi, double zj, double pzj, double s_r, double p,
                                            double qq, bool f32) {
  ZblTerm t{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const double u = r * s_r;
  if (!(u < 1.0)) return t;
  constexpr double a0 = 0.46850;
  constexpr double c1 = 0.02817, c2 = 0.28022, c3 = 0.50986, c4 = 0.18175;
  constexpr double d1 = -0.20162, d2 = -0.40290, d3 = -0.94229, d4 = -3.19980;
  double zs = pzi + pzj;  // exact in float64; rounded once when the reference adds in float32
  if (f32) zs = (double)(float)zs;
  const double x = (zs * r) / a0;
  const double x1 = exp(d1 * x), x2 = exp(d2 * x), x3 = exp(d3 * x), x4 = exp(d4 * x);
  const double psi = c1 * x1 + c2 * x2 + c3 * x3 + c4 * x4;
  const double zz = zi * zj;  // integers below 2^24: exact in either dtype
  const double eng = (qq * (zz / r)) * psi;
  const double ca = (p + 1.0) * (p + 2.0) / 2.0, cb = p * (p + 2.0), cc = p * (p + 1.0) / 2;
  double cut = 1.0;
  cut = cut - ca * pow(u, p);
  cut = cut + cb * pow(u, p + 1.0);
  cut = cut - cc * pow(u, p + 2.0);
  if (f32) cut = (double)(float)cut;
  t.e = eng * cut;
  if (ORDER >= 1) {
    const double k = zs / a0;  // dx/dr
    const double dpsi = c1 * d1 * x1 + c2 * d2 * x2 + c3 * d3 * x3 + c4 * d4 * x4;
    const double b_r = qq * zz / r;
    const double deng = b_r * (k * dpsi - psi / r);
    const double P = pow(u, p - 2.0);  // p >= 2
    const double dcut = s_r * P * u * (-ca * p + u * (cb * (p + 1.0) - cc * (p + 2.0) * u));
    t.d1 = deng * cut + eng * dcut;
    t.dr_eng = deng * cut;
    t.eng = eng;
    t.dcut = dcut;
    if (ORDER >= 2) {
      const double d2psi = c1 * d1 * d1 * x1 + c2 * d2 * d2 * x2 + c3 * d3 * d3 * x3 + c4 * d4 * d4 * x4;
      const double d2eng = b_r * (k * k * d2psi - 2.0 * k * dpsi / r + 2.0 * psi / (r * r));
      const double d2cut =
          s_r * s_r * P * (-ca * p * (p - 1.0) + u * (cb * (p + 1.0) * p - cc * (p + 2.0) * (p + 1.0) * u));
      t.d2 = d2eng * cut + 2.0 * deng * dcut + eng * d2cut;
    }
  }
  return t;
}

// MODE 0: forward (pe_out), 1: backward (g_vec), 2: second order (gg_pe and / or g_vec)
template <int MODE>
__global__ __launch_bounds__(256) void zbl_kernel(const ZblArgs a) {
  const int sub = threadIdx.x & 15;
  const int64_t n = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
  const bool ok = n < a.N;
  const bool own = n < a.n_out;
  double acc = 0.0;
  if (ok) {
    const int ti = (int)a.types[n];
    const double zi = a.zt[2 * ti], pzi = a.zt[2 * ti + 1];
    const double gp = (MODE != 0 && own && a.g_pe != nullptr) ? a.g_pe[n] : 0.0;
    const double qq = *a.qq;
    const int32_t end = a.rowptr[n + 1];
    for (int32_t k = a.rowptr[n] + sub; k < end; k += 16) {
      const int64_t e = a.eid[k];
      const int tj = (int)a.types[a.nbr[k]];
      const double vx = a.vec[3 * e], vy = a.vec[3 * e + 1], vz = a.vec[3 * e + 2];
      const double r = sqrt(vx * vx + vy * vy + vz * vz);
      const double s_r = a.rmax_edge != nullptr ? a.rmax_edge[e] : a.rmax_recip;
      const ZblTerm t = zbl_term<MODE>(r, zi, pzi, a.zt[2 * tj], a.zt[2 * tj + 1], s_r, a.p, qq, a.f32 != 0);
      if (MODE == 0) {
        acc += t.e;
      } else if (MODE == 1) {
        // the float32 reference's autograd rounds the cotangent of its float32 cutoff value, g_pe * eng, to float32
        const double gd1 = a.f32 ? gp * t.dr_eng + (double)(float)(gp * t.eng) * t.dcut : gp * t.d1;
        const double f = t.d1 != 0.0 ? gd1 / r : 0.0;
        a.g_vec[3 * e] = f * vx;
        a.g_vec[3 * e + 1] = f * vy;
        a.g_vec[3 * e + 2] = f * vz;
      } else {
        const bool live = t.d1 != 0.0 || t.d2 != 0.0;
        const double cx = a.cot[3 * e], cy = a.cot[3 * e + 1], cz = a.cot[3 * e + 2];
        const double hx = live ? vx / r : 0.0, hy = live ? vy / r : 0.0, hz = live ? vz / r : 0.0;
        const double hc = hx * cx + hy * cy + hz * cz;
        acc += t.d1 * hc;
        if (a.g_vec != nullptr) {
          // g_pe * (E'' h (h . c) + E'/r (c - h (h . c)))
          const double s = live ? t.d1 / r : 0.0;
          const double w = t.d2 * hc;
          a.g_vec[3 * e] = gp * (w * hx + s * (cx - hx * hc));
          a.g_vec[3 * e + 1] = gp * (w * hy + s * (cy - hy * hc));
          a.g_vec[3 * e + 2] = gp * (w * hz + s * (cz - hz * hc));
        }
      }
    }
  }
  if (MODE != 1) {
    acc += __shfl_xor(acc, 8);
    acc += __shfl_xor(acc, 4);
    acc += __shfl_xor(acc, 2);
    acc += __shfl_xor(acc, 1);
    if (ok && own && sub == 0) {
      if (MODE == 0) {
        a.pe_out[n] = a.pe_in != nullptr ? acc + a.pe_in[n] : acc;
      } else if (a.gg_pe != nullptr) {
        a.gg_pe[n] = acc;
      }
    }
  }
}

template <int MODE>
int zbl_launch(const ZblArgs& a, const char* what, hipStream_t s) {
  if (a.N > 0) hipLaunchKernelGGL(zbl_kernel<MODE>, dim3((unsigned)((a.N * 16 + 255) / 256)), dim3(256), 0, s, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return NQA_ERR_LAUNCH;
  }
  return NQA_OK;
}

bool zbl_geometry(ZblArgs& a, const double* edge_vec, const int32_t* rowptr_dst, const int32_t* edge_id_dst,
                  const int32_t* src_sorted, const int64_t* atom_types, const double* z_table,
                  const double* rmax_recip_edge, double rmax_recip, double p, int32_t round_f32, const double* qqr2e_half,
                  int64_t num_nodes, int64_t num_out, const char* what) {
  if (num_nodes < 0 || num_out < 0 || num_out > num_nodes || !(p >= 2.0) ||
      (rmax_recip_edge == nullptr && !(rmax_recip > 0.0)) ||
      (num_nodes > 0 && (!edge_vec || !rowptr_dst || !edge_id_dst || !src_sorted || !atom_types || !z_table || !qqr2e_half))) {
    set_error(std::string(what) + ": invalid argument");
    return false;
  }
  a.vec = edge_vec;
  a.rowptr = rowptr_dst;
  a.eid = edge_id_dst;
  a.nbr = src_sorted;
  a.types = atom_types;
  a.zt = z_table;
  a.rmax_edge = rmax_recip_edge;
  a.rmax_recip = rmax_recip;
  a.p = p;
  a.qq = qqr2e_half;
  a.f32 = round_f32;
  a.N = num_nodes;
  a.n_out = num_out;
  return true;
}

}  // namespace nqa

extern "C" {

int nqa_zbl_fwd(const double* edge_vec, const int32_t* rowptr_dst, const int32_t* edge_id_dst, const int32_t* src_sorted,
                const int64_t* atom_types, const double* z_table, const double* rmax_recip_edge, double rmax_recip, double p,
                int32_t round_f32, const double* qqr2e_half, int64_t num_nodes, int64_t num_out, const double* pe_in,
                double* pe_out, nqa_stream stream) {
  using namespace nqa;
  ZblArgs a{};
  if (!zbl_geometry(a, edge_vec, rowptr_dst, edge_id_dst, src_sorted, atom_types, z_table, rmax_recip_edge, rmax_recip, p,
                    round_f32, qqr2e_half, num_nodes, num_out, "nqa_zbl_fwd"))
    return NQA_ERR_INVALID;
  if (num_out > 0 && !pe_out) {
    set_error("nqa_zbl_fwd: pe_out is required");
    return NQA_ERR_INVALID;
  }
  a.pe_in = pe_in;
  a.pe_out = pe_out;
  return zbl_launch<0>(a, "nqa_zbl_fwd", static_cast<hipStream_t>(stream));
}

int nqa_zbl_bwd(const double* edge_vec, const int32_t* rowptr_dst, const int32_t* edge_id_dst, const int32_t* src_sorted,
                const int64_t* atom_types, const double* z_table, const double* rmax_recip_edge, double rmax_recip, double p,
                int32_t round_f32, const double* qqr2e_half, int64_t num_nodes, int64_t num_out, const double* g_pe,
                double* g_edge_vec, nqa_stream stream) {
  using namespace nqa;
  ZblArgs a{};
  if (!zbl_geometry(a, edge_vec, rowptr_dst, edge_id_dst, src_sorted, atom_types, z_table, rmax_recip_edge, rmax_recip, p,
                    round_f32, qqr2e_half, num_nodes, num_out, "nqa_zbl_bwd"))
    return NQA_ERR_INVALID;
  if (num_nodes > 0 && (!g_pe || !g_edge_vec)) {
    set_error("nqa_zbl_bwd: g_pe and g_edge_vec are required");
    return NQA_ERR_INVALID;
  }
  a.g_pe = g_pe;
  a.g_vec = g_edge_vec;
  return zbl_launch<1>(a, "nqa_zbl_bwd", static_cast<hipStream_t>(stream));
}

int nqa_zbl_bwd_bwd(const double* edge_vec, const int32_t* rowptr_dst, const int32_t* edge_id_dst,
                    const int32_t* src_sorted, const int64_t* atom_types, const double* z_table,
                    const double* rmax_recip_edge, double rmax_recip, double p, int32_t round_f32, const double* qqr2e_half,
                    int64_t num_nodes, int64_t num_out, const double* g_pe, const double* cot_edge_vec, double* gg_pe,
                    double* g_edge_vec2, nqa_stream stream) {
  using namespace nqa;
  ZblArgs a{};
  if (!zbl_geometry(a, edge_vec, rowptr_dst, edge_id_dst, src_sorted, atom_types, z_table, rmax_recip_edge, rmax_recip, p,
                    round_f32, qqr2e_half, num_nodes, num_out, "nqa_zbl_bwd_bwd"))
    return NQA_ERR_INVALID;
  if (num_nodes > 0 && (!cot_edge_vec || (g_edge_vec2 && !g_pe))) {
    set_error("nqa_zbl_bwd_bwd: cot_edge_vec is required, and g_pe with g_edge_vec2");
    return NQA_ERR_INVALID;
  }
  a.g_pe = g_pe;
  a.cot = cot_edge_vec;
  a.gg_pe = gg_pe;
  a.g_vec = g_edge_vec2;
  return zbl_launch<2>(a, "nqa_zbl_bwd_bwd", static_cast<hipStream_t>(stream));
}

}  // extern "C"
