/*
 * nequip_amd.h -- C ABI of libnequip_amd.so, the MI355X (gfx950) implementation of the NequIP
 * message-passing hot path.
 *
 * The reference (mir-group/nequip v0.19.0) is pure Python and has no FFI; its seam for accelerated
 * kernels is the torch.nn.Module contract of `TensorProductScatter` plus the `enable_*` model
 * modifiers (nequip/nn/_tp_scatter_base.py:9-109, adapters nequip/nn/_tp_scatter_oeq.py:4-57 and
 * nequip/nn/_tp_scatter_cueq.py:66-122).  This header is the native boundary that sits *under* that
 * contract: every entry point below names the reference interface it replaces.  The Python host side
 * (nequip_amd/nn/...) binds these symbols with ctypes and mirrors the reference module API on top.
 *
 * Conventions
 *  - Every data pointer is a *borrowed device pointer* (HIP global memory) owned by the caller; the
 *    library never allocates or frees result buffers.  Scratch comes from caller-provided workspaces
 *    sized by the matching *_workspace_bytes query.
 *  - Kernels are enqueued asynchronously on the passed `stream` (a hipStream_t); no entry point
 *    synchronises the device and there is no global mutable state besides immutable plans.
 *  - Return value: NQA_OK (0) or a negative error code; nqa_last_error() returns a thread-local
 *    human-readable message.  The host side converts non-zero codes to RuntimeError, matching the
 *    reference's exception-only error convention.
 *  - Feature layout is e3nn "mul_ir" ([mul, 2l+1], m fastest) unless the plan was created with
 *    NQA_LAYOUT_IR_MUL for that operand.  Edge attributes have mul == 1 per irrep.
 *  - dtype selects the arithmetic/storage type of feature tensors: NQA_F32 or NQA_F64 (the reference's
 *    `model_dtype`, nequip/nn/_tp_scatter_base.py:33).  Edge vectors are always float64
 *    (nequip/utils/global_dtype.py:5).
 */
#ifndef NEQUIP_AMD_H
#define NEQUIP_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NQA_ABI_VERSION 1

enum nqa_status {
  NQA_OK = 0,
  NQA_ERR_INVALID = -1,     /* bad argument / inconsistent irreps or instruction            */
  NQA_ERR_UNSUPPORTED = -2, /* l > NQA_LMAX, unsupported dtype, ...                          */
  NQA_ERR_LAUNCH = -3,      /* HIP launch / runtime failure                                  */
  NQA_ERR_WORKSPACE = -4    /* workspace missing or too small                                */
};

enum nqa_dtype { NQA_F32 = 0, NQA_F64 = 1 };
enum nqa_layout { NQA_LAYOUT_MUL_IR = 0, NQA_LAYOUT_IR_MUL = 1 };

enum nqa_plan_field {
  NQA_PLAN_DIM_IN1 = 0,      /* feature_irreps_in.dim                                        */
  NQA_PLAN_DIM_IN2 = 1,      /* irreps_edge_attr.dim                                         */
  NQA_PLAN_DIM_OUT = 2,      /* irreps_mid.dim                                               */
  NQA_PLAN_WEIGHT_NUMEL = 3, /* e3nn TensorProduct.weight_numel                              */
  NQA_PLAN_NUM_INSTR = 4,
  NQA_PLAN_OUT_NEEDS_ZERO = 5, /* 1 if output slots are shared/uncovered (caller must zero `out`) */
  NQA_PLAN_YPART_WIDTH = 6,  /* columns of the per-edge dY partial buffer (bwd_edge workspace) */
  NQA_PLAN_HAS_SPECIALIZED = 7, /* 1 if structure-specialised (edge-outer) kernels are prebuilt for this plan */
  NQA_PLAN_FUSED_ROWS_OK = 8  /* 1 if nqa_tp_scatter_bwd_fused keeps its per-channel operands (grad_out row, two feature
                                 rows, the weights and their gradient) in registers; 0: it spills (l_max = 4 middle
                                 layer: 364 values) and nqa_tp_scatter_bwd_x + _bwd_edge are the faster route */
};

typedef struct nqa_plan nqa_plan;
typedef void* nqa_stream; /* hipStream_t */

int nqa_abi_version(void);
const char* nqa_last_error(void);
/* largest supported l for features / edge attributes / outputs, and for spherical harmonics */
int nqa_lmax(void);
int nqa_sh_lmax(void);

/* ---------------------------------------------------------------------------------------------
 * Plan: replaces the constructor of nequip.nn.TensorProductScatter
 *   __init__(feature_irreps_in, irreps_edge_attr, irreps_mid, instructions)
 *   (nequip/nn/_tp_scatter_base.py:10-33), i.e. e3nn TensorProduct(..., 'uvu' instructions,
 *   shared_weights=False, internal_weights=False, irrep_normalization="component",
 *   path_normalization="element").  Built once from exactly those four arguments; immutable and
 *   thread-safe afterwards.  Each irreps operand is given as parallel arrays (mul, l, p) with
 *   p = +1 (even) / -1 (odd).  Instructions are (i_in1, i_in2, i_out) index triples, mode "uvu";
 *   path_weight may be NULL (all 1.0).  The weight tensor is consumed in instruction-list order,
 *   mul_in1 values per instruction.
 * ------------------------------------------------------------------------------------------- */
int nqa_plan_create(int32_t n_in1, const int32_t* in1_mul, const int32_t* in1_l, const int32_t* in1_p,
                    int32_t n_in2, const int32_t* in2_mul, const int32_t* in2_l, const int32_t* in2_p,
                    int32_t n_out, const int32_t* out_mul, const int32_t* out_l, const int32_t* out_p,
                    int32_t n_instr, const int32_t* instr_i1, const int32_t* instr_i2,
                    const int32_t* instr_io, const double* instr_path_weight,
                    int32_t layout_in1, int32_t layout_out, nqa_plan** plan);
void nqa_plan_destroy(nqa_plan* plan);
int64_t nqa_plan_query(const nqa_plan* plan, int32_t field);
/* The kernels read the plan's path tables from device memory.  The library does not allocate device
 * memory: the caller obtains the (position independent) table image, copies it into a device buffer it
 * owns (the host side keeps it as a non-persistent module buffer so it follows `.to(device)`) and
 * passes that buffer as `plan_image` to the nqa_tp_* calls. */
int64_t nqa_plan_image_bytes(const nqa_plan* plan);
int nqa_plan_image_write(const nqa_plan* plan, void* host_dst, int64_t host_dst_bytes);

/* ---------------------------------------------------------------------------------------------
 * Edge topology (CSR): replaces the implicit index handling of
 *   x[edge_src] (row gather, nequip/nn/_tp_scatter_base.py:36) and
 *   scatter(edge_features, edge_dst, dim=0, dim_size=N) (nequip/nn/utils.py:24-53),
 * for arbitrary (unsorted, repeated) int64 indices as in
 *   tests/unit/nn/test_tp_scatter_kernel.py:144-149.  Groups the E edges by `key` with a stable
 * radix sort:  rowptr[n]..rowptr[n+1] indexes the edges whose key == n (ascending original edge
 * id), edge_id[] holds their original ids and other_sorted[] the matching `other` index.
 * Call once with (key=edge_dst, other=edge_src) for forward / edge gradients and once with
 * (key=edge_src, other=edge_dst) for the feature gradient (the transposed graph, cf.
 * nequip/data/transforms/neighborlist.py:150-155 `edge_transpose_perm`).
 * Returns NQA_ERR_INVALID (reported asynchronously as out-of-range being clamped is NOT done):
 * indices must satisfy 0 <= idx < num_nodes; this is checked on the device and reported through
 * `status_flag` (int32 device word, set non-zero on violation) when it is non-NULL.
 * ------------------------------------------------------------------------------------------- */
int64_t nqa_csr_workspace_bytes(int64_t num_nodes, int64_t num_edges);
int nqa_csr_build(const int64_t* key, const int64_t* other, int64_t num_nodes, int64_t num_edges,
                  int32_t* rowptr, int32_t* edge_id, int32_t* other_sorted, int32_t* status_flag,
                  void* workspace, int64_t workspace_bytes, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Fused gather -> Clebsch-Gordan tensor product ('uvu', per-edge weights) -> scatter-add.
 * Replaces TensorProductScatter.forward(x, edge_attr, edge_weight, edge_dst, edge_src)
 *   (nequip/nn/_tp_scatter_base.py:35-38):
 *   out[n, slot_p, u, k] = sum_{e: dst(e)=n} c_p * w[e, p, u] * sum_ij C^p_ijk x[src(e), u, i] y[e, j]
 * x [N, dim_in1], y [E, dim_in2], w [E, weight_numel], out [N, dim_out]; (rowptr, edge_id,
 * src_sorted) from nqa_csr_build(key=dst, other=src).  Rows of `out` without incoming edges are
 * written as zeros.  If NQA_PLAN_OUT_NEEDS_ZERO the caller must pre-zero `out`.
 * ------------------------------------------------------------------------------------------- */
int nqa_tp_scatter_fwd(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x, const void* y, const void* w,
                       const int32_t* rowptr_dst, const int32_t* edge_id_dst, const int32_t* src_sorted,
                       void* out, int64_t num_nodes, int64_t num_edges, nqa_stream stream);

/* Backward of the op above w.r.t. the per-edge operands (replaces the autograd of the e3nn einsum
 * chain exercised by tests/unit/nn/test_tp_scatter_kernel.py:160-177):
 *   gw[e,p,u] = c_p sum_ijk C^p_ijk x[src(e),u,i] y[e,j] g[dst(e),slot_p,u,k]
 *   gy[e,j]   = sum_p sum_u c_p w[e,p,u] sum_ik C^p_ijk x[src(e),u,i] g[dst(e),slot_p,u,k]
 * gw and/or gy may be NULL (gradient not needed).  `workspace` (>= nqa_tp_bwd_edge_workspace_bytes)
 * holds deterministic per-path partial sums of gy; required iff gy != NULL. */
int64_t nqa_tp_bwd_edge_workspace_bytes(const nqa_plan* plan, int32_t dtype, int64_t num_edges);
int nqa_tp_scatter_bwd_edge(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x, const void* y, const void* w,
                            const void* grad_out, const int32_t* rowptr_dst, const int32_t* edge_id_dst,
                            const int32_t* src_sorted, void* grad_w, void* grad_y, void* workspace,
                            int64_t workspace_bytes, int64_t num_nodes, int64_t num_edges, nqa_stream stream);

/* Backward w.r.t. the node features (a scatter over *src*: the transposed graph):
 *   gx[m, u, i] = sum_{e: src(e)=m} sum_p c_p w[e,p,u] sum_jk C^p_ijk y[e,j] g[dst(e),slot_p,u,k]
 * (rowptr, edge_id, dst_sorted) from nqa_csr_build(key=src, other=dst). */
int nqa_tp_scatter_bwd_x(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* y, const void* w, const void* grad_out,
                         const int32_t* rowptr_src, const int32_t* edge_id_src, const int32_t* dst_sorted,
                         void* grad_x, int64_t num_nodes, int64_t num_edges, nqa_stream stream);

/* All three gradients of the op in one pass over grad_out (same maths as the two calls above, i.e. the
 * autograd of nequip/nn/_tp_scatter_base.py:77-120 w.r.t. x, edge_attr and the weights): the edge kernel
 * (dst-CSR, grad_out[dst] resident in registers) additionally emits each edge's contribution to
 * grad_x[src(e)] as a row of `workspace`; a second kernel sums those rows per source node through the
 * src-CSR (rowptr_src, edge_id_src) -- deterministic, no atomics, and grad_out rows are never gathered
 * per edge.  grad_w, grad_y and grad_x are all required (callers needing fewer use the calls above).  Only plans with a structure-specialised
 * kernel (NQA_PLAN_HAS_SPECIALIZED) in float32 support it: nqa_tp_bwd_fused_workspace_bytes returns -1
 * otherwise and the caller uses nqa_tp_scatter_bwd_edge + nqa_tp_scatter_bwd_x. */
int64_t nqa_tp_bwd_fused_workspace_bytes(const nqa_plan* plan, int32_t dtype, int64_t num_edges);
int nqa_tp_scatter_bwd_fused(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x, const void* y,
                             const void* w, const void* grad_out, const int32_t* rowptr_dst,
                             const int32_t* edge_id_dst, const int32_t* src_sorted, const int32_t* rowptr_src,
                             const int32_t* edge_id_src, void* grad_w, void* grad_y, void* grad_x, void* workspace,
                             int64_t workspace_bytes, int64_t num_nodes, int64_t num_edges, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Edge vectors: replaces with_edge_vectors_ (nequip/nn/utils.py:68-118),
 *   edge_vec[e] = pos[edge_src[e]] - pos[edge_dst[e]] (+ edge_cell_shift[e] @ cell[batch[edge_dst[e]]]),
 * (edge_dst = edge_index[0] = centre atom, edge_src = edge_index[1] = neighbour), all float64.
 * cell [F,3,3] (rows = lattice vectors), edge_cell_shift [E,3] and batch [N] are optional (NULL: no
 * periodic images / single frame).  The adjoint nqa_edge_vectors_bwd replaces the autograd of those
 * index_select / baddbmm ops (the float64 atomic index_add kernels) by ordered per-atom sums over the
 * two CSRs of nqa_csr_build: g_pos [N,3], and -- when g_cell_per_node [N,9] is non-NULL -- the per-atom
 * contribution sum_{e: dst(e)=n} shift[e]^T g[e] to d/dcell (summed per frame by the caller).
 * ------------------------------------------------------------------------------------------- */
int nqa_edge_vectors_fwd(const double* pos, const int64_t* edge_dst, const int64_t* edge_src,
                         const double* edge_cell_shift, const double* cell, const int64_t* batch,
                         int64_t num_edges, double* edge_vec, nqa_stream stream);
int nqa_edge_vectors_bwd(const double* g_edge_vec, const double* edge_cell_shift, const int32_t* rowptr_dst,
                         const int32_t* edge_id_dst, const int32_t* rowptr_src, const int32_t* edge_id_src,
                         int64_t num_nodes, double sign, double* g_pos, double* g_cell_per_node, nqa_stream stream);
/* `sign` multiplies g_pos (-1: forces = -dE/dpos directly).  g_cell_per_node[n] = sum_{e: centre(e)=n} left[e] (x) g[e]
 * with left = edge_cell_shift -- or any other [E,3] per-edge factor: with left = edge_vec it is the per-atom virial
 * sum, which nqa_virial_finalize reduces per frame:
 *   virial[f] = -sym(sum_n per_atom[n]),  stress[f] = sym(...) / |det cell[f]|   (nequip/nn/grad_output.py:222-271;
 *   stress may be NULL (no cell); batch [N] int64 is required iff num_frames > 1). */
int nqa_virial_finalize(const double* per_atom, const int64_t* batch, const double* cell, int64_t num_nodes,
                        int64_t num_frames, double* virial, double* stress, nqa_stream stream);
/* nqa_frame_sum: out[f, :] = sum_{n: batch[n] = f} rows[n, :]  (float64, width <= 16, every frame written; batch may be
 * NULL for a single frame).  The per-frame reductions of the training path -- autograd's backward of
 * `symmetric_displacement[batch]` and the d/dcell sum of with_edge_vectors_ (nequip/nn/grad_output.py:230-247,
 * nequip/nn/utils.py:88-114), which ATen evaluates as float64 atomics -- as one ordered tree reduction per frame. */
int nqa_frame_sum(const double* rows, const int64_t* batch, int64_t num_nodes, int32_t width, int64_t num_frames,
                  double* out, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Edge embedding: real spherical harmonics + Bessel radial basis with polynomial cutoff.
 * Replaces, for precomputed float64 edge vectors (nequip/nn/utils.py:68-118),
 *   SphericalHarmonicEdgeAttrs.forward  (nequip/nn/embedding/_edge.py:193-198; e3nn
 *       SphericalHarmonics(irreps 0..lmax, normalize=True, normalization="component")),
 *   EdgeLengthNormalizer.forward        (nequip/nn/embedding/_edge.py:65-80),
 *   BesselEdgeLengthEncoding.forward    (nequip/nn/embedding/_edge.py:136-150),
 *   PolynomialCutoff.forward            (nequip/nn/embedding/cutoffs.py:17-27),
 *   ApplyFactor (2*pi/r_max^2)          (nequip/model/nequip_models.py:318-322).
 * All arithmetic is float64; results are rounded to `dtype` exactly where the reference casts
 * (.to(model_dtype)), then bessel*cutoff*factor is formed in `dtype`.
 *   sh  [E, (lmax+1)^2]   emb [E, num_bessels]   cutoff [E]   (any output may be NULL)
 * rmax_recip_edge (optional, [E] float64) overrides the scalar 1/r_max per edge (per-edge-type
 * cutoffs).  bessel_weights: [num_bessels] float64 DEVICE pointer (the reference's buffer /
 * trainable parameter, _edge.py:112-121).
 * ------------------------------------------------------------------------------------------- */
int nqa_edge_embed_fwd(int32_t dtype, int32_t lmax, const double* edge_vec, int64_t num_edges,
                       double rmax_recip, const double* rmax_recip_edge, int32_t num_bessels,
                       const double* bessel_weights, double cutoff_p, double factor, void* sh, void* emb,
                       void* cutoff, nqa_stream stream);
/* Vector-Jacobian product of the above: g_edge_vec[E,3] (float64) from g_sh / g_emb (either may be
 * NULL).  This is the edge -> position leg of the force backward (nequip/nn/grad_output.py:217-221). */
int nqa_edge_embed_bwd(int32_t dtype, int32_t lmax, const double* edge_vec, int64_t num_edges,
                       double rmax_recip, const double* rmax_recip_edge, int32_t num_bessels,
                       const double* bessel_weights, double cutoff_p, double factor, const void* g_sh,
                       const void* g_emb, double* g_edge_vec, nqa_stream stream);
/* The same two kernels for an edge list with a reverse-edge pairing (nqa_edge_pairs: pair_row[e] < num_pairs for the
 * representative edge of a pair, its row in the per-pair arrays; >= num_pairs for the reverse edge): the radial rows are
 * ALSO written per pair, emb_pairs [P, num_bessels] = emb[rep_edge[p]] (what the radial MLP consumes when it is evaluated
 * once per pair -- the gather nqa_pair_gather would do), and the backward takes the per-pair cotangent g_emb_pairs [P,
 * num_bessels] directly (the adjoint nqa_pair_expand would do) next to / instead of the per-edge one; emb, g_sh, g_emb,
 * g_emb_pairs may be NULL.  Plain r_max only (no per-edge cutoffs: those lists are not paired).  Replaces, for a paired
 * list, `edge_embedding[rep]` / its autograd adjoint of nequip_amd's own host (nn/_paired_radial.py); the reference
 * evaluates edge_mlp per directed edge (nequip/nn/interaction_block.py:190-199). */
int nqa_edge_embed_fwd_paired(int32_t dtype, int32_t lmax, const double* edge_vec, int64_t num_edges,
                              double rmax_recip, int32_t num_bessels, const double* bessel_weights, double cutoff_p,
                              double factor, const int32_t* pair_row, int64_t num_pairs, void* sh, void* emb,
                              void* emb_pairs, nqa_stream stream);
int nqa_edge_embed_bwd_paired(int32_t dtype, int32_t lmax, const double* edge_vec, int64_t num_edges,
                              double rmax_recip, int32_t num_bessels, const double* bessel_weights, double cutoff_p,
                              double factor, const int32_t* pair_row, int64_t num_pairs, const void* g_sh,
                              const void* g_emb, const void* g_emb_pairs, double* g_edge_vec, nqa_stream stream);
/* Second order (force-matching training, nequip/nn/grad_output.py:220 create_graph=True): for the cotangent
 * cot_g_edge_vec [E,3] of the VJP output above, gg_sh / gg_emb = J(v) c (gradients w.r.t. g_sh / g_emb) and
 * g_edge_vec2 = (sum_k g_k Hessian_k(v)) c (gradient w.r.t. the edge vector).  Evaluated with forward-mode dual
 * numbers through the same per-edge code as the first-order kernels.  Any output may be NULL. */
int nqa_edge_embed_bwd_bwd(int32_t dtype, int32_t lmax, const double* edge_vec, int64_t num_edges,
                           double rmax_recip, const double* rmax_recip_edge, int32_t num_bessels,
                           const double* bessel_weights, double cutoff_p, double factor, const void* g_sh,
                           const void* g_emb, const double* cot_g_edge_vec, void* gg_sh, void* gg_emb,
                           double* g_edge_vec2, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Radial network on MFMA: replaces ScalarMLPFunction.forward as InteractionBlock.edge_mlp
 *   (nequip/nn/interaction_block.py:119-127,196; nequip/nn/mlp.py:141-156,194-196,262-268) for the
 *   standard one-hidden-layer, bias-free, SiLU radial MLP:
 *     edge_weight[E, W] = silu(edge_embedding[E, nb] @ (w0[nb, H] * alpha0)) @ (w1[H, W] * alpha1)
 *   The hidden layer never leaves the chip.  `mode` selects how the big GEMM ([E,H] x [H,W]) runs on the matrix
 *   cores: NQA_MLP_FP32 = v_mfma_f32_32x32x2_f32 (bitwise an fp32 fma chain); NQA_MLP_BF16X6 = every fp32 operand
 *   split exactly into three bf16 terms and the six partial products >= 2^-16 accumulated in fp32 on
 *   v_mfma_f32_32x32x16_bf16 (dropped terms < 2^-24 relative: fp32 accuracy, 2.7x the fp32-MFMA ceiling).  The
 *   small first layer (K = nb) and all element-wise maths are fp32 in both modes.
 * nqa_radial_mlp_bwd is its vector-Jacobian product w.r.t. the edge embedding (inference forces:
 *   nequip/nn/grad_output.py:217-221); pre-activations are recomputed, not stored.  These two entry points give
 *   no parameter gradients: training runs the variants below (nqa_radial_mlp_bwd_train, nqa_radial_mlp_fwd_tangent),
 *   which hand out the on-chip pieces of dW0 and dW1.  num_basis 1..8: rows of edge_embedding and of
 *   grad_edge_embedding have stride num_basis.
 * nqa_radial_mlp_supported returns 1 when (dtype, nb, H, W) can run on the fused kernels
 *   (float32, nb <= 8, H in {64, 128}, W % 4 == 0).  `workspace` (>= nqa_radial_mlp_workspace_bytes(mode,
 *   backward, H, W); 0 for the fp32 forward) receives the re-laid-out / split second-layer weights (a function of
 *   w1, alpha1, mode and direction only): a caller whose weights are constant may keep it and pass
 *   workspace_ready != 0 on later calls to skip the prepass kernel.
 * ------------------------------------------------------------------------------------------- */
#define NQA_MLP_FP32 0
#define NQA_MLP_BF16X6 1
/* every entry point except nqa_radial_mlp_fwd_tangent (which rejects it): operands multiplied by exact powers of two and split into two fp16 terms, three partial products on
 * v_mfma_f32_32x32x16_f16 -- fp32-level accuracy (2^-22 per operand) at half the matrix instructions of BF16X6.  Forward:
 * weights scaled per 32-column tile, hidden activations per row.  Backward: weights per 32-row K chunk, the streamed
 * gradient rows by a running per-row exponent that is lowered, together with the row's accumulators, when a chunk
 * outgrows it.  The workspace of this mode differs from BF16X6's (nqa_radial_mlp_workspace_bytes). */
#define NQA_MLP_F16X3 2
/* OR-ed into `mode` of nqa_radial_mlp_bwd (ignored elsewhere): a scheduling hint, no effect on results beyond the order of
 * fp32 roundings -- "nothing else will run on the device next to this launch".  The inference backward of a NARROW output
 * (W <= 256) may then take the persistent form with all weight fragments resident in LDS (radial_mlp_pipe.h; enabled by
 * NQA_MLP_BWD_SMALL=1, see radial_mlp.hip for the measurements); without the hint it keeps the many-short-workgroups form, which shares the chip better with concurrent streams (nequip_amd's host runs
 * the radial backward of all layers but the first next to the main chain). */
#define NQA_MLP_HINT_DEVICE_IS_IDLE 0x100
int nqa_radial_mlp_supported(int32_t dtype, int32_t num_basis, int32_t hidden, int32_t out_features);
int64_t nqa_radial_mlp_workspace_bytes(int32_t mode, int32_t backward, int32_t hidden, int32_t out_features);
int nqa_radial_mlp_fwd(int32_t dtype, int32_t mode, const void* edge_embedding, const void* w0, double alpha0,
                       const void* w1, double alpha1, int32_t num_basis, int32_t hidden, int32_t out_features,
                       int64_t num_edges, void* edge_weight, void* workspace, int64_t workspace_bytes,
                       int32_t workspace_ready, nqa_stream stream);
int nqa_radial_mlp_bwd(int32_t dtype, int32_t mode, const void* edge_embedding, const void* w0, double alpha0,
                       const void* w1, double alpha1, const void* grad_edge_weight, int32_t num_basis,
                       int32_t hidden, int32_t out_features, int64_t num_edges, void* grad_edge_embedding,
                       void* workspace, int64_t workspace_bytes, int32_t workspace_ready, nqa_stream stream);

/* Training variants of the fused radial MLP (force-matching training differentiates the force pass once more,
 *   nequip/nn/grad_output.py:216-221 `create_graph=self.training`; in the reference all of this is autograd through
 *   ScalarMLPFunction.forward, nequip/nn/mlp.py:194-196).  nqa_radial_mlp_bwd_train: NQA_MLP_BF16X6 or
 *   NQA_MLP_F16X3 (the host's default, nn/mlp.py::backward_mode); nqa_radial_mlp_fwd_tangent: NQA_MLP_BF16X6 only.
 *   NQA_MLP_FP32 has no training form and no second gradient stream: NQA_ERR_UNSUPPORTED, outputs untouched.  Every
 *   output below is tested element by element against float64 (tests/test_radial_mlp_launches.py).  With
 *   W_i = w_i alpha_i, P = emb W0, G_h = grad_edge_weight W1^T:
 * nqa_radial_mlp_bwd_train, cotangent == NULL (first order, with the pieces of the parameter gradients):
 *     grad_edge_embedding = (G_h silu'(P)) W0^T                       [E, num_basis]
 *     hidden_out          = silu(P)                                   [E, hidden]   (dW1 = alpha1 hidden_out^T grad_edge_weight)
 *     w0_partials[tile]   = emb_tile^T (G_h silu'(P))_tile            [tiles][num_basis][hidden], dW0 = alpha0 sum_tiles
 *                           (tile t = rows 128 t .. 128 t + 127; every element of every tile is written)
 *   cotangent != NULL ([E, num_basis], a cotangent c of grad_edge_embedding; second order), Q = c W0:
 *     grad_edge_embedding = (Q G_h silu''(P)) W0^T                    = d<c, g_emb>/d emb
 *     hidden_out          = Q silu'(P)                                (d<c,g_emb>/dW1 = alpha1 hidden_out^T grad_edge_weight)
 *     w0_partials[tile]   = emb^T (Q G_h silu''(P)) + c^T (G_h silu'(P))   (d<c,g_emb>/dW0 = alpha0 sum_tiles)
 *   tiles = nqa_radial_mlp_train_tiles(num_edges) (128-edge workgroup tiles).
 * nqa_radial_mlp_fwd_tangent: out = (Q silu'(P)) W1 = d<c, g_emb>/d grad_edge_weight, the directional derivative of
 *   the MLP along `cotangent`; same workspace as nqa_radial_mlp_fwd. */
/* nqa_radial_mlp_bwd_paired: nqa_radial_mlp_bwd for an incoming gradient given as two row streams that are added on
 *   the fly (grad_edge_weight[row] + grad_edge_weight2[row]): the halves written by the two directed edges of a pair in
 *   nqa_tp_scatter_bwd_*_paired.  num_edges counts rows (pairs).  NQA_MLP_BF16X6 or NQA_MLP_F16X3. */
int nqa_radial_mlp_bwd_paired(int32_t dtype, int32_t mode, const void* edge_embedding, const void* w0, double alpha0,
                              const void* w1, double alpha1, const void* grad_edge_weight,
                              const void* grad_edge_weight2, int32_t num_basis, int32_t hidden, int32_t out_features,
                              int64_t num_edges, void* grad_edge_embedding, void* workspace, int64_t workspace_bytes,
                              int32_t workspace_ready, nqa_stream stream);
int64_t nqa_radial_mlp_train_tiles(int64_t num_edges);
int nqa_radial_mlp_bwd_train(int32_t dtype, int32_t mode, const void* edge_embedding, const void* cotangent,
                             const void* w0, double alpha0, const void* w1, double alpha1,
                             const void* grad_edge_weight, int32_t num_basis, int32_t hidden, int32_t out_features,
                             int64_t num_edges, void* grad_edge_embedding, void* hidden_out, void* w0_partials,
                             void* workspace, int64_t workspace_bytes, int32_t workspace_ready, nqa_stream stream);
int nqa_radial_mlp_fwd_tangent(int32_t dtype, int32_t mode, const void* edge_embedding, const void* cotangent,
                               const void* w0, double alpha0, const void* w1, double alpha1, int32_t num_basis,
                               int32_t hidden, int32_t out_features, int64_t num_edges, void* out, void* workspace,
                               int64_t workspace_bytes, int32_t workspace_ready, nqa_stream stream);

/* The last layer of a DEEPER radial MLP (ScalarMLPFunction with hidden_layers_depth >= 2, nequip/nn/mlp.py:81-196; the
 *   reference's tutorial model uses depth 2 / width 64, configs/tutorial.yaml:222-223) on the same GEMM cores:
 *     nqa_radial_mlp_last_fwd:  out [E, out_features] = silu(pre) @ (w alpha)
 *     nqa_radial_mlp_last_bwd:  grad_pre [E, hidden]  = ((grad_out (+ grad_out2)) @ (w alpha)^T) * silu'(pre)
 *   `pre` [E, hidden] are the PRE-activations of the layer's input -- for depth 2 the output of nqa_radial_mlp_fwd on the
 *   first two weight matrices (out_features = hidden width), whose gradient nqa_radial_mlp_bwd then takes on to the edge
 *   embedding; deeper stacks chain nqa_radial_mlp_last_fwd.  hidden 64 or 128, out_features % 4 == 0, float32, mode
 *   NQA_MLP_F16X3 (fp32-accurate two-plane fp16 split; workspaces as for nqa_radial_mlp_fwd / _bwd in that mode).
 *   Any other mode, or another hidden width: NQA_ERR_UNSUPPORTED.  `pre` is taken as exact data: silu and silu' are
 *   evaluated to fp32 accuracy for |pre| up to 30 and beyond (compensated exponent, radial_mlp.hip).
 *   Inference (first order) only: training-mode deep MLPs stay on the ATen formulation. */
int nqa_radial_mlp_last_fwd(int32_t dtype, int32_t mode, const void* pre, const void* w, double alpha, int32_t hidden,
                            int32_t out_features, int64_t num_edges, void* out, void* workspace, int64_t workspace_bytes,
                            int32_t workspace_ready, nqa_stream stream);
int nqa_radial_mlp_last_bwd(int32_t dtype, int32_t mode, const void* pre, const void* w, double alpha,
                            const void* grad_out, const void* grad_out2, int32_t hidden, int32_t out_features,
                            int64_t num_edges, void* grad_pre, void* workspace, int64_t workspace_bytes,
                            int32_t workspace_ready, nqa_stream stream);


/* ---------------------------------------------------------------------------------------------
 * Node-side channel mixing in one launch: replaces e3nn o3.Linear (linear_1 / linear_2,
 *   nequip/nn/interaction_block.py:82-87,129-138,177,201), the self-connection
 *   FullyConnectedTensorProduct with scalar node attributes (interaction_block.py:142-146,175; weights
 *   pre-contracted per atom type by the caller) and the residual add `x + sc` (:203-204):
 *     out[z, ob, w, m] = scale * sum_{(ib->ob)} sum_u x[z, ib, u, m] * W[type(z)][ib->ob][u, w]  (+ addend[z,...])
 *   mul_ir layout.  chunk_table: int32 records {o_off, d, mul_out, c0, instr_begin, instr_end, width, 0} (one per
 *   64-channel chunk of an output irrep block, every output element covered exactly once); instr_table: int32
 *   records {x_off, mul_in, w_off, 0} ([mul_in, mul_out] row-major matrix at weights + type*weight_stride + w_off).
 *   chunk_width = 64: float32 runs on fp32 MFMA with LDS-staged operands, float64 on the VALU kernel;
 *   chunk_width = -64 forces the VALU kernel for float32 as well.
 *   atom_types (int64 [N]) is required iff n_types > 1.  The backward w.r.t. x is the same call with transposed
 *   tables/weights.  chunk_table / instr_table are HOST pointers (<= 64 instructions; more than 40 chunks are
 *   processed in several launches): they are copied into the kernel arguments at call time.  x, weights, addend, out, atom_types are device pointers.
 * nqa_gate: e3nn Gate (nequip/nn/convnetlayer.py:104-112,162-164): in = scalars (+) gates (+) gated ->
 *   out = act(scalars) (+) act(gates)[u] * gated[u, :] (act 0 = identity, 1 = silu, 2 = tanh, each times its e3nn
 *   normalize2mom constant `cst`).  col_table: one 32-byte record {int32 a, b, c, d; double cst; int32 e, f} per
 *   column -- forward (backward == 0), per OUTPUT column: {src, gate (-1 for scalars), act, 0, cst, 0, 0}:
 *   out[z,c] = gate < 0 ? act(in[z,src]) : act(in[z,gate]) * in[z,src]; backward, per INPUT column:
 *   {kind, act, o, i, cst, len, gate}: kind 0 (scalar) gin = g[z,o] act'(in[z,c]); kind 1 (gate) gin = act'(in[z,c])
 *   sum_{m<len} g[z,o+m] in[z,i+m]; kind 2 (gated) gin = act(in[z,gate]) g[z,o]; kind 3: zero.
 *   Second order (training, nequip/nn/grad_output.py:220 create_graph): with a cotangent c [N, dim_in] of gin,
 *   backward = 2 writes d<c,gin>/d grad_out [N, dim_out] (forward table), backward = 3 writes d<c,gin>/d input
 *   [N, dim_in] (backward table).
 * ------------------------------------------------------------------------------------------- */
int nqa_node_linear(int32_t dtype, const void* x, const void* weights, const void* addend, void* out,
                    const int64_t* atom_types, const void* chunk_table, int32_t n_chunks, const void* instr_table,
                    int32_t n_instr, int32_t n_types, int64_t weight_stride, int32_t dim_in, int32_t dim_out,
                    int64_t num_nodes, double scale, int32_t chunk_width, nqa_stream stream);
/* ... _ordered: the same launch with an atom order (int32 [N] device pointer, may be NULL; float32 MFMA kernels only): the
 *   work units walk the atoms in that order and skip the typed stages of atom types none of their atoms has.  ANY permutation
 *   gives the same results; one that groups the atoms by type makes a typed map (the self-connection: one weight set per
 *   atom type) one pass per atom instead of one per type. */
int nqa_node_linear_ordered(int32_t dtype, const void* x, const void* weights, const void* addend, void* out,
                            const int64_t* atom_types, const int32_t* atom_order, const void* chunk_table, int32_t n_chunks,
                            const void* instr_table, int32_t n_instr, int32_t n_types, int64_t weight_stride,
                            int32_t dim_in, int32_t dim_out, int64_t num_nodes, double scale, int32_t chunk_width,
                            nqa_stream stream);
int nqa_gate(int32_t dtype, int32_t backward, const void* input, const void* grad_out, const void* cotangent,
             void* out, const void* col_table, int32_t dim_in, int32_t dim_out, int64_t num_nodes, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Split 16-bit form of nqa_node_linear (float32 tensors, default for constant weights): the same maps -- e3nn `o3.Linear`
 *   / the type-contracted `FullyConnectedTensorProduct` of nequip/nn/interaction_block.py:82-87,129-146,175-177,201 --
 *   with fp32-level accuracy on the 16-bit matrix pipe.  Default: every operand multiplied by an exact power of two and
 *   written as the sum of two fp16 numbers, three partial products on v_mfma_f32_32x32x16_f16 (weights scaled per atom
 *   type, instruction and 16-row K block; every output column carries a running exponent).  NQA_NODE_F16=0 (environment,
 *   read at every call): three bf16 numbers per operand, six partial products on v_mfma_f32_32x32x16_bf16.
 * nqa_node_weights_pack: weights [n_types][weight_stride] (the layout nqa_node_linear reads) -> `packed`
 *   (nqa_node_weights_pack_bytes bytes): [type][instruction][16-row K block][32-column tile][plane][lane] of 16 bytes = 8
 *   16-bit values W[16 kb + 8 (lane >> 5) + e][32 tile + (lane & 31)], zero beyond the matrix; fp16 mode: 2 planes, then
 *   int32 exponents [type][instruction][K block]; bf16 mode: 3 planes.  Once per weight version, and the buffer must be
 *   consumed in the mode it was packed in.
 * nqa_node_linear_packed: out = scale * sum_instr x_block @ W (+ addend), tables as for nqa_node_linear (chunks must
 *   start at multiples of 64 channels); one 64-lane workgroup per (64-channel chunk, floor(32 / d) atoms) unit.
 * ------------------------------------------------------------------------------------------- */
int64_t nqa_node_weights_pack_bytes(const void* chunk_table, int32_t n_chunks, const void* instr_table, int32_t n_instr,
                                    int32_t n_types);
int nqa_node_weights_pack(const void* weights, const void* chunk_table, int32_t n_chunks, const void* instr_table,
                          int32_t n_instr, int32_t n_types, int64_t weight_stride, void* packed, nqa_stream stream);
int nqa_node_linear_packed(const void* x, const void* packed, const void* addend, void* out, const int64_t* atom_types,
                           const void* chunk_table, int32_t n_chunks, const void* instr_table, int32_t n_instr,
                           int32_t n_types, int32_t dim_in, int32_t dim_out, int64_t num_nodes, double scale,
                           nqa_stream stream);
int nqa_node_linear_packed_ordered(const void* x, const void* packed, const void* addend, void* out,
                                   const int64_t* atom_types, const int32_t* atom_order, const void* chunk_table,
                                   int32_t n_chunks, const void* instr_table, int32_t n_instr, int32_t n_types,
                                   int32_t dim_in, int32_t dim_out, int64_t num_nodes, double scale, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * The node side of a layer boundary in one launch per direction.  Between two tensor products the reference runs
 *   h = linear_2(y) + sc;  x = Gate(h)                                   (nequip/nn/convnetlayer.py:156-170)
 *   sc' = sc(x, node_attrs);  x1 = linear_1(x) / sqrt(avg_num_neighbors)   (nequip/nn/interaction_block.py:175-181)
 * -- Gate, linear_1 and the self-connection as three passes over [N, D] rows (and four more in the backward).
 * nqa_node_fused runs up to two `parts` (each what nqa_node_linear_packed takes: rows, packed fp16-split weights and the
 *   tables they were packed with, a destination) in ONE launch:
 *     - parts[k].in_gate != NULL: the part's rows x are PRE-gate rows h; the instruction x_off of its tables are offsets
 *       into Gate(h) and the gate is applied while the operand slab is staged (forward: both consumers of a gate in
 *       one launch, two destinations, Gate(h) never written);
 *     - parts[1].accumulate != 0: parts[1] has the same output chunks as parts[0] and is ADDED into the same tiles
 *       (linear_1^T(g_x1) + sc^T(g_sc); one scale, out / addend / dim_out of parts[0]);
 *     - out_gate != NULL: the tiles are gradients w.r.t. Gate(h) and leave through the gate's backward,
 *       out[N, gate_dim] = d/dh, with gate_h the pre-gate rows (chunk o_off are offsets into Gate(h)).
 *   nqa_gate_block: one block of a gate's OUTPUT: `mul` channels of dimension `d` at out_off <- values at val_off of the
 *   input row, gate scalars at gate_off (one per channel; -1: a scalar block, act applied to the values; act / cst as
 *   for nqa_gate).  Gated blocks need d >= 3; gated / activated blocks need offsets, multiplicities and row widths that
 *   are multiples of 4 (NQA_ERR_INVALID otherwise: the caller keeps the separate launches).  Float32, fp16-split packing
 *   (NQA_ERR_UNSUPPORTED under NQA_NODE_F16=0); at most 48 merged instructions; tables are HOST pointers.
 *   atom_order (optional, int32 [N], device): the order in which the work units walk the atoms -- ANY permutation gives the
 *   same results; a unit skips the typed stages of atom types none of its atoms has, so an order that groups the atoms by
 *   type makes the typed self-connection (at most 16 types) one pass per atom instead of one per type.
 * nqa_node_fused_plan: the merged tables of such a launch, for host-side tests -- chunk records of 12 int32 {o_off, d,
 *   mul_out, c0, instr_begin, instr_end, dst, epilogue (0 plain, 1 scalar block, 2 gated block of the output gate), ev_off,
 *   eg_off, act, cst (float bits)}, instruction records of 8 int32 {x_off, mul_in, frag_off, exp_off, gate_off (>= 0 gate
 *   scalars, -1 activate the values, -2 plain), act, cst (float bits), operand set}; returns (n_chunks << 16) | n_instr.
 * ------------------------------------------------------------------------------------------- */
typedef struct nqa_gate_block {
  int32_t out_off, d, mul, val_off, gate_off, act;
  double cst;
} nqa_gate_block;

typedef struct nqa_node_part {
  const void* x;           /* [N, dim_in] float32 rows */
  const void* packed;      /* nqa_node_weights_pack of (chunk_table, instr_table, n_types), fp16 split */
  const void* chunk_table; /* as for nqa_node_linear_packed (host) */
  const void* instr_table;
  int32_t n_chunks, n_instr, n_types, dim_in;
  void* out;               /* [N, dim_out]; ignored when accumulate != 0 */
  const void* addend;      /* optional [N, dim_out] */
  int32_t dim_out, accumulate;
  double scale;
  const nqa_gate_block* in_gate; /* optional (host) */
  int32_t n_in_gate, pad;
} nqa_node_part;

int nqa_node_fused(const nqa_node_part* parts, int32_t n_parts, const int64_t* atom_types, const int32_t* atom_order,
                   int64_t num_nodes, const nqa_gate_block* out_gate, int32_t n_out_gate, const void* gate_h,
                   int32_t gate_dim, nqa_stream stream);
int nqa_node_fused_plan(const nqa_node_part* parts, int32_t n_parts, const nqa_gate_block* out_gate, int32_t n_out_gate,
                        int32_t* chunks_out, int32_t chunks_cap, int32_t* instr_out, int32_t instr_cap);

/* ---------------------------------------------------------------------------------------------
 * Per-atom energy head in one launch per direction.  After the last convolution the reference runs Gate (scalars only) ->
 *   ScalarMLP readout of depth 0 (x @ W alpha, nequip/nn/mlp.py:262-268; built at nequip/model/nequip_models.py:371-381)
 *   -> PerTypeScaleShift (float64 addcmul, nequip/nn/atomwise.py:116-284), and autograd the same chain backwards.
 *   backward == 0:  out[z] (float64) = shift[type z] + scale[type z] * double( sum_c W[c] cst act(h[z, c]) )
 *   backward != 0:  out[z, c] (float32) = float(grad_e[z] * scale[type z]) * W[c] * cst act'(h[z, c])
 *   h [N, dim] float32 (dim a multiple of 4), readout_weight [dim] float32 with alpha folded in, scales / shifts float64 of
 *   length 0 (absent), 1 (shared) or one per type (atom_types required), act as for nqa_gate (0 identity, 1 silu, 2 tanh).
 *   The dot product is accumulated in float32 and scaled / shifted in float64, as the reference does.
 * ------------------------------------------------------------------------------------------- */
int nqa_energy_head(int32_t backward, const void* h, const void* readout_weight, const void* scales, int32_t n_scales,
                    const void* shifts, int32_t n_shifts, const int64_t* atom_types, const void* grad_e, void* out,
                    int32_t dim, int32_t act, double cst, int64_t num_nodes, nqa_stream stream);

/* Training form of the energy head: trainable PerTypeScaleShift tables (nequip/nn/atomwise.py:190-234).  The forward is
 *   nqa_energy_head(0, ...).  With a(x) = cst act(x), s_n = sum_c W[c] a(h[n, c]) (float32), t = type n,
 *   gf_n = float(grad_e[n] * scale[t]):
 *   nqa_energy_head_train_bwd:      grad_h[n, c] = gf_n W[c] a'(h[n, c])                       (may be NULL)
 *                                   grad_w[c] = sum_n gf_n a(h[n, c])                          (may be NULL)
 *                                   grad_scales[t] = sum_{n in t} grad_e[n] double(s_n)        (may be NULL; [n_scales])
 *                                   grad_shifts[t] = sum_{n in t} grad_e[n]                    (may be NULL; [n_shifts])
 *   nqa_energy_head_train_bwd_bwd:  the backward of (grad_e, h, W, scale) -> grad_h for a cotangent cot_grad_h [N, dim],
 *                                   u_n = sum_c cot[n, c] W[c] a'(h[n, c]) (float32):
 *                                   grad_grad_e[n] = scale[t] double(u_n)                      (may be NULL)
 *                                   grad_h[n, c] = gf_n W[c] a''(h[n, c]) cot[n, c]            (may be NULL)
 *                                   grad_w[c] = sum_n gf_n a'(h[n, c]) cot[n, c]               (may be NULL)
 *                                   grad_scales[t] = sum_{n in t} grad_e[n] double(u_n)        (may be NULL)
 *   Tables of one entry collect every atom.  The sums over atoms are taken in two launches: one row of partial sums per
 *   workgroup into `workspace` (device memory of nqa_energy_head_train_workspace_bytes(num_nodes, dim or 0, n_scales or 0,
 *   n_shifts or 0) bytes, 0 for a gradient that is not requested; 8-byte aligned, owned by the caller), then the rows added
 *   in a fixed order.  No atomics: the results are bit-reproducible.  No allocation, no host synchronisation.  dim a multiple
 *   of 4 up to 512; a table whose gradient is requested has at most 128 entries. */
int64_t nqa_energy_head_train_workspace_bytes(int64_t num_nodes, int32_t dim, int32_t n_scales, int32_t n_shifts);
int nqa_energy_head_train_bwd(const void* h, const void* readout_weight, const void* scales, int32_t n_scales,
                              int32_t n_shifts, const int64_t* atom_types, const void* grad_e, void* grad_h, void* grad_w,
                              void* grad_scales, void* grad_shifts, void* workspace, int64_t workspace_bytes, int32_t dim,
                              int32_t act, double cst, int64_t num_nodes, nqa_stream stream);
int nqa_energy_head_train_bwd_bwd(const void* h, const void* readout_weight, const void* scales, int32_t n_scales,
                                  const int64_t* atom_types, const void* grad_e, const void* cot_grad_h, void* grad_grad_e,
                                  void* grad_h, void* grad_w, void* grad_scales, void* workspace, int64_t workspace_bytes,
                                  int32_t dim, int32_t act, double cst, int64_t num_nodes, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * ZBL core-repulsion pair term (nequip/nn/pair_potential.py:230-389, _ZBL / ZBL; LAMMPS pair_style zbl).  Per edge
 *   e = (i <- j), r = |edge_vec_e|, u = r * rmax_recip(e):
 *     E_e = qqr2e_half Z_i Z_j / r * psi((Z_i^0.23 + Z_j^0.23) r / 0.46850) * cutoff_p(u),  psi = the four-exponential
 *     screening function, cutoff_p = the PolynomialCutoff polynomial masked by u < 1 (E_e and all its derivatives are an
 *     exact zero for u >= 1).
 *   nqa_zbl_fwd:     pe_out[n] = pe_in[n] (NULL: 0) + sum_{e: centre(e) = n} E_e
 *   nqa_zbl_bwd:     g_edge_vec[e] = g_pe[centre(e)] * E'(r) v_e / r          (every row of [E, 3] written)
 *   nqa_zbl_bwd_bwd: given a cotangent c [E, 3] of g_edge_vec, h = v / r:
 *                      gg_pe[n] = sum_{e: centre(e) = n} E'(r) (h . c_e)                      (may be NULL)
 *                      g_edge_vec2[e] = g_pe[centre] (E'' h (h . c) + E'/r (c - h (h . c)))   (may be NULL)
 *   edge_vec float64 [E, 3]; (rowptr_dst, edge_id_dst, src_sorted) the centre-atom CSR of nqa_csr_build(key = edge_dst);
 *   atom_types int64 [num_nodes]; z_table float64 [T, 2] = (Z, Z^0.23) holding model-dtype values; rmax_recip_edge
 *   float64 [E] or NULL (then the scalar rmax_recip); p >= 2; round_f32 != 0: the float32 model's roundings (the sum
 *   Z_i^0.23 + Z_j^0.23, the cutoff value and, in nqa_zbl_bwd, its cotangent are rounded to float32, as the reference
 *   and its autograd do); qqr2e_half: ONE float64 in device memory, 0.5 qqr2e (the module's `_qqr2exesquare` buffer:
 *   no host read, capturable).
 *   Rows n >= num_out (num_out <= num_nodes: a local-ghost list) have no per-atom energy: their edges contribute nothing.
 *   16 lanes per centre atom, fixed-order sums: no atomics, bit-identical repeated evaluations.  No allocation.
 * ------------------------------------------------------------------------------------------- */
int nqa_zbl_fwd(const double* edge_vec, const int32_t* rowptr_dst, const int32_t* edge_id_dst, const int32_t* src_sorted,
                const int64_t* atom_types, const double* z_table, const double* rmax_recip_edge, double rmax_recip, double p,
                int32_t round_f32, const double* qqr2e_half, int64_t num_nodes, int64_t num_out, const double* pe_in,
                double* pe_out, nqa_stream stream);
int nqa_zbl_bwd(const double* edge_vec, const int32_t* rowptr_dst, const int32_t* edge_id_dst, const int32_t* src_sorted,
                const int64_t* atom_types, const double* z_table, const double* rmax_recip_edge, double rmax_recip, double p,
                int32_t round_f32, const double* qqr2e_half, int64_t num_nodes, int64_t num_out, const double* g_pe,
                double* g_edge_vec, nqa_stream stream);
int nqa_zbl_bwd_bwd(const double* edge_vec, const int32_t* rowptr_dst, const int32_t* edge_id_dst,
                    const int32_t* src_sorted, const int64_t* atom_types, const double* z_table,
                    const double* rmax_recip_edge, double rmax_recip, double p, int32_t round_f32, const double* qqr2e_half,
                    int64_t num_nodes, int64_t num_out, const double* g_pe, const double* cot_edge_vec, double* gg_pe,
                    double* g_edge_vec2, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Paired radial weights.  InteractionBlock.edge_mlp (nequip/nn/interaction_block.py:119-127,190-192) is a function of
 *   the edge length alone, and a neighbour list holds every interaction as (i <- j, S) and (j <- i, -S): the reference
 *   evaluates the MLP twice per pair.  nqa_edge_pairs finds the pairs of a list:
 *     weight_rows[e] = p (representative edge of pair p: dst < src, or a self image with a "positive" shift) or
 *                      p + P (its reverse), P = num_edges / 2;  rep_edge[p] = the representative edge;
 *     partner_edge[e] = the reverse edge of e;
 *     *ok (device int32) = 1 iff every edge has exactly one reverse partner (else the arrays are not to be used).
 *   edge_cell_shift: [E, 3] float32 / float64 (shift_dtype) integer-valued, or NULL.  (rowptr_dst, edge_id_dst, src_sorted):
 *   the dst-CSR of the same list (nqa_csr_build) -- the reverse of (i <- j, S) is looked up in row j, eight lanes per edge,
 *   no sort; pairs are numbered in the edge order of their representative.  For nqa_edge_pairs edge_id_dst may be NULL: the
 *   dst-CSR then lists the edges in edge order (edge_id[k] == k: a list grouped by centre atom, as the device neighbour list
 *   emits it), one dependent load less per look-up.
 * nqa_csr_from_pairs: the by-SOURCE CSR of a paired list without sorting -- row j holds the partners of the edges of row j
 *   of the dst-CSR: rowptr_src = rowptr_dst, edge_id_src[k] = partner_edge[edge_id_dst[k]], dst_sorted = src_sorted.
 * nqa_tp_scatter_{fwd,bwd_edge,bwd_x,bwd_fused}_paired: the tensor-product entry points above with
 *   w = [num_pairs, weight_numel] (one row per pair) and, for the edge backward, grad_w = [2 * num_pairs, weight_numel]
 *   (row weight_rows[e] receives edge e's gradient; the caller -- or nqa_radial_mlp_bwd's second stream -- adds the two
 *   halves).  weight_rows is given in CSR slot order of the respective topology (weight_rows[edge_id[slot]]).
 *   Structure-specialised float32 plans only (NQA_ERR_UNSUPPORTED otherwise).
 * ------------------------------------------------------------------------------------------- */
int64_t nqa_edge_pairs_workspace_bytes(int64_t num_edges);
int nqa_edge_pairs(const int64_t* edge_dst, const int64_t* edge_src, const void* edge_cell_shift, int32_t shift_dtype,
                   const int32_t* rowptr_dst, const int32_t* edge_id_dst, const int32_t* src_sorted, int64_t num_edges,
                   int64_t num_nodes, void* workspace, int64_t workspace_bytes, int32_t* weight_rows, int64_t* rep_edge,
                   int32_t* partner_edge, int32_t* ok, nqa_stream stream);
int nqa_csr_from_pairs(const int32_t* edge_id_dst, const int32_t* partner_edge, int64_t num_edges, int32_t* edge_id_src,
                       nqa_stream stream);
/* nqa_pair_gather: rows_out[p, :] = rows_in[rep_edge[p], :] (the per-pair rows of a per-edge float32 array, e.g. the
 *   edge embedding fed to the radial MLP); nqa_pair_expand is its adjoint: edge_rows[e, :] = pair_rows[weight_rows[e], :]
 *   for representative edges and 0 for the reverse ones (every row written).  width = 32-bit words per row. */
int nqa_pair_gather(const void* rows_in, const int64_t* rep_edge, int64_t num_pairs, int32_t width, void* rows_out,
                    nqa_stream stream);
/* nqa_pair_owner_lists: the pair lists of nqa_tp_scatter_bwd_pairs (below) from a pairing (weight_rows, rep_edge of
 *   nqa_edge_pairs with *ok == 1) and the dst-CSR of the same edge list (nqa_csr_build: rowptr, edge_id, src_sorted).  Every
 *   directed edge is the owner-side or the other-side edge of its pair -- owner of {i <- j, j <- i}: i when (i < j) xor
 *   (i + j odd), a self-image pair through its representative edge -- so both lists of a node are subsequences of its CSR
 *   row: two counting passes, two prefix sums, two fill passes, no sort, no synchronisation.  Slots keep the CSR order.
 *   Outputs (int32, device): owner_rowptr [N + 1], pair_other / pair_row / pair_edge_in / pair_edge_out [P] by slot,
 *   other_rowptr [N + 1], other_slot [P] (the slots grouped by their other node). */
int64_t nqa_pair_owner_workspace_bytes(int64_t num_edges, int64_t num_nodes);
int nqa_pair_owner_lists(const int32_t* weight_rows, const int64_t* rep_edge, const int32_t* rowptr_dst,
                         const int32_t* edge_id_dst, const int32_t* src_sorted, int64_t num_edges, int64_t num_nodes,
                         void* workspace, int64_t workspace_bytes, int32_t* owner_rowptr, int32_t* pair_other,
                         int32_t* pair_row, int32_t* pair_edge_in, int32_t* pair_edge_out, int32_t* other_rowptr,
                         int32_t* other_slot, nqa_stream stream);
/* nqa_pair_owner_lists_guard: for callers that cannot wait for nqa_edge_pairs' verdict (a hipGraph capture): when *ok == 0 on
 *   the device, both row pointers are zeroed -- the pair-centric kernels then walk empty lists instead of unwritten slots.
 *   The evaluation is void in that case; the caller reads `ok` afterwards. */
int nqa_pair_owner_lists_guard(const int32_t* ok, int64_t num_nodes, int32_t* owner_rowptr, int32_t* other_rowptr,
                               nqa_stream stream);
int nqa_pair_expand(const void* pair_rows, const int32_t* weight_rows, int64_t num_edges, int64_t num_pairs,
                    int32_t width, void* edge_rows, nqa_stream stream);
int nqa_tp_scatter_fwd_paired(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x, const void* y,
                              const void* w, const int32_t* rowptr_dst, const int32_t* edge_id_dst,
                              const int32_t* src_sorted, void* out, int64_t num_nodes, int64_t num_edges,
                              const int32_t* weight_rows, int64_t num_pairs, nqa_stream stream);
int nqa_tp_scatter_bwd_edge_paired(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x,
                                   const void* y, const void* w, const void* grad_out, const int32_t* rowptr_dst,
                                   const int32_t* edge_id_dst, const int32_t* src_sorted, void* grad_w, void* grad_y,
                                   void* workspace, int64_t workspace_bytes, int64_t num_nodes, int64_t num_edges,
                                   const int32_t* weight_rows, int64_t num_pairs, nqa_stream stream);
int nqa_tp_scatter_bwd_fused_paired(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x,
                                    const void* y, const void* w, const void* grad_out, const int32_t* rowptr_dst,
                                    const int32_t* edge_id_dst, const int32_t* src_sorted, const int32_t* rowptr_src,
                                    const int32_t* edge_id_src, void* grad_w, void* grad_y, void* grad_x,
                                    void* workspace, int64_t workspace_bytes, int64_t num_nodes, int64_t num_edges,
                                    const int32_t* weight_rows, int64_t num_pairs, nqa_stream stream);
int nqa_tp_scatter_bwd_x_paired(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* y,
                                const void* w, const void* grad_out, const int32_t* rowptr_src,
                                const int32_t* edge_id_src, const int32_t* dst_sorted, void* grad_x, int64_t num_nodes,
                                int64_t num_edges, const int32_t* weight_rows, int64_t num_pairs, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Pair-centric backward of the tensor-product scatter with paired radial weights (all three gradients in one pass;
 *   replaces, like nqa_tp_scatter_bwd_fused_paired, autograd's backward of `out = scatter(tp(x[src], y, w), dst)`,
 *   nequip/nn/_tp_scatter_base.py:33-38, for the case where `w` holds one row per reverse-edge pair).
 *   Every pair p = {other -> owner, owner -> other} has an owner node; the owner's wavefront evaluates both directed
 *   edges, so the weight row is read once, grad_w = [num_pairs, weight_numel] leaves ALREADY SUMMED over the two
 *   directed edges (no halves), and one per-pair row of grad_x contributions (instead of one per edge) goes through the
 *   workspace.  The pair lists (int32, device), P = num_edges / 2 slots grouped by owner:
 *     owner_rowptr [N+1]; per slot: pair_other (the other node), pair_row (row of w / grad_w), pair_edge_in (the edge
 *     other -> owner, i.e. dst = owner), pair_edge_out (owner -> other);  other_rowptr [N+1] / other_slot [P]: the slots
 *     grouped by their `other` node.  Any assignment of owners is valid; a balanced one halves every node's list.
 *   grad_y [E, dim_in2] per directed edge, grad_x [N, dim_in1] or NULL (grad_w and grad_y only: other_rowptr /
 *   other_slot are then not read).  float32 structure-specialised plans whose register
 *   budget allows it: nqa_tp_bwd_pairs_workspace_bytes returns -1 otherwise (use the per-edge entry points).
 *   Round 6: for multiples of 64 channels (and at least as many pairs as nodes) the other node's grad_x contributions are
 *   summed by floating-point atomics into a zeroed [N, dim_in1] accumulator inside the same workspace instead of one row per
 *   pair + a row sum (other_rowptr / other_slot are then not read): grad_x is equal within fp32 rounding but NOT bit-identical
 *   from call to call (sums in arrival order).  NQA_PAIR_GX_ATOMIC=0 in the environment keeps the fixed-order rows,
 *   NQA_PAIR_RING=0 the register / plain-loop kernels of rounds 3-5 (both read at every call).
 * ------------------------------------------------------------------------------------------- */
int64_t nqa_tp_bwd_pairs_workspace_bytes(const nqa_plan* plan, int32_t dtype, int64_t num_edges);
int nqa_tp_scatter_bwd_pairs(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x, const void* y,
                             const void* w, const void* grad_out, const int32_t* owner_rowptr,
                             const int32_t* pair_other, const int32_t* pair_row, const int32_t* pair_edge_in,
                             const int32_t* pair_edge_out, const int32_t* other_rowptr, const int32_t* other_slot,
                             void* grad_w, void* grad_y, void* grad_x, void* workspace, int64_t workspace_bytes,
                             int64_t num_nodes, int64_t num_edges, nqa_stream stream);

/* Second-order companion (force-matching training differentiates the backward once more, nequip/nn/grad_output.py:217-221):
 *   with cotangents x_cot [N, dim_in1] of grad_x and y_cot [E, dim_in2] of grad_y,
 *     grad_w = Bw(x_cot, y, grad_out) + Bw(x, y_cot, grad_out)   [num_pairs, weight_numel], summed over each pair,
 *     grad_y = By(x_cot, w, grad_out) (+ By(x, w_cot, grad_out) when w_cot [num_pairs, weight_numel] is given)  [E, dim_in2]
 *   in ONE pair-centric pass (the intermediate sum_k C_ijk grad_out_k serves both products) instead of two calls of
 *   nqa_tp_scatter_bwd_pairs and an addition.  Plans with a single-wavefront pair kernel only
 *   (nqa_tp_bwd_pairs_dual_supported); workspace as nqa_tp_bwd_pairs_workspace_bytes. */
int32_t nqa_tp_bwd_pairs_dual_supported(const nqa_plan* plan, int32_t dtype);
int nqa_tp_scatter_bwd_pairs_dual(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x,
                                  const void* x_cot, const void* y, const void* y_cot, const void* w, const void* w_cot,
                                  const void* grad_out, const int32_t* owner_rowptr, const int32_t* pair_other,
                                  const int32_t* pair_row, const int32_t* pair_edge_in, const int32_t* pair_edge_out,
                                  void* grad_w, void* grad_y, void* workspace, int64_t workspace_bytes,
                                  int64_t num_nodes, int64_t num_edges, nqa_stream stream);

/* Forward-mode companion of the same second-order backward: the gradient w.r.t. grad_out of <cotangents, backward outputs>,
 *   out = F(x_cot, y, w) + F(x, y_cot, w) + F(x, y, w_cot)      (F = nqa_tp_scatter_fwd; the op is trilinear)
 *   in one pass over the edges instead of three forward launches and two additions.  A NULL cotangent drops its term (at
 *   least one is required when there are edges: the operands of an edge-free graph are empty, so their pointers may
 *   all be NULL, and out is zeros); w / w_cot hold one row per edge, or per pair when weight_rows (dst-CSR slot order, as
 *   nqa_tp_scatter_fwd_paired) is given.  Structure-specialised float32 plans (nqa_tp_fwd_jvp_supported). */
int32_t nqa_tp_fwd_jvp_supported(const nqa_plan* plan, int32_t dtype);
int nqa_tp_scatter_fwd_jvp(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* x, const void* y,
                           const void* w, const void* x_cot, const void* y_cot, const void* w_cot,
                           const int32_t* rowptr_dst, const int32_t* edge_id_dst, const int32_t* src_sorted, void* out,
                           int64_t num_nodes, int64_t num_edges, const int32_t* weight_rows, int64_t num_pairs,
                           nqa_stream stream);
/* ... and the gradient w.r.t. x:  grad_x = Bx(y_cot, w, grad_out) + Bx(y, w_cot, grad_out)  in one pass over the source
 *   CSR (operands as nqa_tp_scatter_bwd_x / _paired; plans for which nqa_tp_fwd_jvp_supported holds). */
int nqa_tp_scatter_bwd_x_dual(const nqa_plan* plan, const void* plan_image, int32_t dtype, const void* y, const void* w,
                              const void* y_cot, const void* w_cot, const void* grad_out, const int32_t* rowptr_src,
                              const int32_t* edge_id_src, const int32_t* dst_sorted, void* grad_x, int64_t num_nodes,
                              int64_t num_edges, const int32_t* weight_rows, int64_t num_pairs, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Parameter gradients of the dense maps of the path (training; in the reference these come out of autograd as the
 *   weight-side `mm` / `einsum` backward of ScalarLinearLayer.forward (nequip/nn/mlp.py:262-268), e3nn o3.Linear
 *   (nequip/nn/interaction_block.py:82-87,129-138) and the self-connection FullyConnectedTensorProduct (:142-146)):
 *     dW[t][out_off + i*N + j] = sum_{z < num_rows, type(z) == t} sum_{m < d} A[z*lda + a_off + i*d + m] *
 *                                                                              B[z*ldb + b_off + j*d + m]
 *   for every record {int32 a_off, b_off, M, N, d, out_off} of instr_table (HOST pointer, <= 64 records; i < M,
 *   j < N).  ScalarMLP layer: one record {0, 0, in, out, 1, 0} over the E edge rows; o3.Linear / FCTP: one record per
 *   (input block -> output block) matrix with d = 2l+1 over the N atom rows (mul_ir layout), row_types / n_types > 1
 *   for the per-atom-type pre-contracted self-connection weights.
 *   The reduction over rows is split into `splits` ranges (nqa_wgrad_splits suggests a count that fills the device;
 *   each range is covered by the four wavefronts of one workgroup, which add their tiles in a fixed order on chip);
 *   partials is [splits][n_types][out_stride] floats, every element covered by a record is written (the rest is
 *   left untouched), and the caller sums over the first axis -- deterministic, no atomics.  float32 only (fp32 MFMA;
 *   outputs wider than 64 rows run as fp32-accurate split-bf16 products, NQA_WGRAD_EXACT_FP32=1 keeps them on fp32 MFMA).
 * ------------------------------------------------------------------------------------------- */
int32_t nqa_wgrad_splits(const void* instr_table, int32_t n_instr, int32_t n_types, int64_t num_rows);
int nqa_wgrad(int32_t dtype, const void* a_rows, const void* b_rows, const int64_t* row_types,
              const void* instr_table, int32_t n_instr, int64_t lda, int64_t ldb, int64_t num_rows, int32_t n_types,
              int64_t out_stride, int32_t splits, void* partials, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Neighbour list on the device: replaces _compute_neighborlist_single_frame
 *   (nequip/data/_nl.py:63-165), i.e. the CPU library call `neighbour_list("ijS", pbc, cell, positions, cutoff)`:
 *   all ordered pairs (i, j, S) with |pos[j] - pos[i] + S @ cell| < r_max except i == j with S == 0;
 *   edge_index[0] = i (convolution centre), edge_index[1] = j, S = integer lattice shifts (0 along non-periodic
 *   directions).  pos [N,3] float64 (anywhere in space), cell [3,3] float64 rows = lattice vectors (NULL or all-zero:
 *   no cell, only valid without periodicity), pbc int32[3] (device; NULL = none).  Triclinic cells, cells thinner than
 *   the cutoff (several images of one atom) and mixed periodicity are supported.
 * Two calls because the number of edges is data dependent:
 *   nqa_neighbor_list_count builds the cell grid in `workspace` (>= nqa_neighbor_list_workspace_bytes(N)) and writes
 *     rowptr [N+1] int32 (device): rowptr[i]..rowptr[i+1] = the edge range of centre atom i, rowptr[N] = E;
 *   the caller reads rowptr[N], allocates edge_index [2,E] int64 and edge_cell_shift [E,3] float64, and calls
 *   nqa_neighbor_list_fill with the same workspace.  Edges come out grouped by centre atom in ascending order
 *   (dst-sorted: rowptr IS the dst-CSR row pointer of the tensor-product kernels) and in a deterministic order
 *   within each atom.
 * ------------------------------------------------------------------------------------------- */
int64_t nqa_neighbor_list_workspace_bytes(int64_t num_atoms);
int nqa_neighbor_list_count(const double* pos, const double* cell, const int32_t* pbc, double r_max, int64_t num_atoms,
                            void* workspace, int64_t workspace_bytes, int32_t* rowptr, nqa_stream stream);
int nqa_neighbor_list_fill(const void* workspace, const int32_t* rowptr, int64_t num_atoms, int64_t num_edges,
                           int64_t* edge_index, double* edge_cell_shift, nqa_stream stream);
/* Capacity-padded variant: no read-back of the edge count, so neighbour list -> pairing -> model can be captured in ONE
 *   hipGraph and replayed with new positions (molecular dynamics; the reference rebuilds its list on the host every step,
 *   nequip/integrations/ase.py:125-160 -> data/_nl.py:63-165).  After nqa_neighbor_list_count, writes exactly `edge_capacity`
 *   (even) edges: the E_real = rowptr[N] real ones, and behind the real edges of each atom its share of the E_cap - E_real
 *   padding edges -- self-image pairs (i <- i, +S), (i <- i, -S) with S = k >= k0 cells along the shortest periodic lattice
 *   vector, k0 |a| > r_max.  Padding edges lie outside the polynomial cutoff (nequip/nn/embedding/cutoffs.py:23-27: exactly
 *   zero there, with zero slope), so their radial embedding, their bias-free radial-MLP weights
 *   (nequip/nn/interaction_block.py:119-127) and every derivative w.r.t. their length vanish: energies and forces are those
 *   of the unpadded list.  A cell is required (edge vectors of self images come from the shift alone).
 *   rowptr_padded [N+1] int32 = the dst-CSR row pointer of the padded list (rowptr_padded[N] = edge_capacity);
 *   src_sorted int32 [edge_capacity] (may be NULL) = edge_index[1] as the int32 neighbour array of that CSR (whose edge ids
 *   are 0 .. edge_capacity - 1 in order).
 *   status int32[2] (device, may be NULL): status[0] = 1 when the list did not fit (E_real > capacity, or capacity - E_real
 *   odd) -- the output then holds padding edges ONLY (all indices valid, results void) and the caller repeats the step with a
 *   larger capacity; status[1] = E_real. */
int nqa_neighbor_list_fill_padded(const void* workspace, const int32_t* rowptr, int64_t num_atoms, int64_t edge_capacity,
                                  int32_t* rowptr_padded, int64_t* edge_index, double* edge_cell_shift, int32_t* src_sorted,
                                  int32_t* status, nqa_stream stream);
/* Batched variant: F frames (systems) in one set of launches, with one host read per batch instead of one per frame.
 *   Frame f owns the atoms [frame_ptr[f], frame_ptr[f+1]) of pos [N,3] float64; frame_ptr int64 [F+1] (device) starts at 0
 *   and ends at N.  cell [F,3,3] float64 (NULL = no frame has a cell), pbc int32 [F,3] (device; NULL = none): every frame has
 *   its own cell and periodicity, and frames without a cell (all-zero) may sit next to periodic triclinic ones.  Zero lattice
 *   vectors along non-periodic directions are completed on the device as the host path's _complete_cell does.
 *   nqa_neighbor_list_batched_count plans every frame on the device (one header per frame: cell inverse, fractional origin,
 *     bins per direction; frame f gets the n_f + 8 bins the single-frame plan gives it, so workspace bytes depend on (N, F)
 *     alone) and writes rowptr [N+1] int32 (device, global atom numbering; rowptr[N] = E) and status int32[1] (device,
 *     zeroed first): bit 0 more than 2^31 - 1 edges, bit 1 a zero lattice vector along a periodic direction, bit 2 linearly
 *     dependent lattice vectors, bit 3 frame_ptr not a partition of [0, N), bit 4 periodicity without a cell.  The caller
 *     reads rowptr[N] and status together (place them next to each other: one copy), rejects a non-zero status, and calls
 *   nqa_neighbor_list_batched_fill with the same workspace.  edge_index / edge_cell_shift are bitwise the concatenation of
 *     the single-frame lists of the frames with atom indices offset by frame_ptr[f]: grouped by centre atom in ascending
 *     order (rowptr is the dst-CSR row pointer of the whole batch), the single-frame order within an atom, no edge between
 *     two frames.  Needs N + 8F < 2^31. */
int64_t nqa_neighbor_list_batched_workspace_bytes(int64_t num_atoms, int64_t num_frames);
int nqa_neighbor_list_batched_count(const double* pos, const double* cell, const int32_t* pbc, const int64_t* frame_ptr,
                                    double r_max, int64_t num_atoms, int64_t num_frames, void* workspace,
                                    int64_t workspace_bytes, int32_t* rowptr, int32_t* status, nqa_stream stream);
int nqa_neighbor_list_batched_fill(const void* workspace, const int32_t* rowptr, int64_t num_atoms, int64_t num_frames,
                                   int64_t num_edges, int64_t* edge_index, double* edge_cell_shift, nqa_stream stream);
/* Typed variants: per-edge-type cutoffs (nequip/data/transforms/neighborlist.py:9-117 prunes a finished list on the host; here
 *   the pruning is part of the search).  atom_types int64 [N] (device), cutoff_table float64 [T,T] (device, row-major
 *   (centre type, neighbour type): the table EdgeLengthNormalizer indexes with type[edge_index[0]] * T + type[edge_index[1]]),
 *   1 <= T <= 32768.  The edge (i <- j, S) is kept iff  r2 < r_max^2  and  r2 <= cutoff_table[type_i][type_j]^2  (`<=` as the
 *   reference's norm_length <= 1; the squares are formed once per call, on the device).  Everything else is the contract of the
 *   untyped entry point of the same name: the grid is the r_max grid, so the result is bitwise the untyped list with the
 *   dropped edges removed -- same grouping by centre atom, same order within an atom, rowptr = the dst-CSR row pointer of the
 *   PRUNED list, batched = concatenation of the typed single-frame lists.  A symmetric table keeps the list symmetric (both
 *   directions of a pair see the same r2); an asymmetric table legitimately does not.
 *   The caller checks the table on the host (entries positive and <= r_max); the kernels do not.
 *   Workspace: nqa_neighbor_list_typed_workspace_bytes(N, T) / nqa_neighbor_list_batched_typed_workspace_bytes(N, F, T) -- the
 *   untyped workspace followed by the neighbour types in bin order (int32 [N], read coalesced by the walk) and the squared
 *   table; the untyped queries return what they always did.
 *   An atom type outside [0, T) never indexes outside the table (it is replaced by 0) and is reported as bit 5 (value 32) of
 *   `status`: int32[1] (device, zeroed first) for the single-frame count, where bit 0 also reports more than 2^31 - 1 edges;
 *   the sixth bit of the batched status word next to the five above.  Place it behind rowptr[N] and read both in one copy.
 *   symmetrise != 0 (single-frame count): prune by max(rc[a][b], rc[b][a]) instead.  The capacity-padded form needs an even
 *   number of free slots, i.e. a symmetric list, so nqa_neighbor_list_fill_padded_typed must follow a count with symmetrise
 *   = 1; the few extra edges of an asymmetric table lie beyond their own type cutoff and are zeroed by the model like every
 *   edge outside its cutoff.  Padding edges are longer than r_max, hence beyond every type cutoff: unchanged.
 *   The fill calls take the same atom_types and num_types as the count. */
int64_t nqa_neighbor_list_typed_workspace_bytes(int64_t num_atoms, int64_t num_types);
int nqa_neighbor_list_count_typed(const double* pos, const double* cell, const int32_t* pbc, double r_max,
                                  const int64_t* atom_types, const double* cutoff_table, int64_t num_types, int32_t symmetrise,
                                  int64_t num_atoms, void* workspace, int64_t workspace_bytes, int32_t* rowptr, int32_t* status,
                                  nqa_stream stream);
int nqa_neighbor_list_fill_typed(const void* workspace, const int32_t* rowptr, const int64_t* atom_types, int64_t num_atoms,
                                 int64_t num_types, int64_t num_edges, int64_t* edge_index, double* edge_cell_shift,
                                 nqa_stream stream);
int nqa_neighbor_list_fill_padded_typed(const void* workspace, const int32_t* rowptr, const int64_t* atom_types,
                                        int64_t num_atoms, int64_t num_types, int64_t edge_capacity, int32_t* rowptr_padded,
                                        int64_t* edge_index, double* edge_cell_shift, int32_t* src_sorted, int32_t* status,
                                        nqa_stream stream);
int64_t nqa_neighbor_list_batched_typed_workspace_bytes(int64_t num_atoms, int64_t num_frames, int64_t num_types);
int nqa_neighbor_list_batched_count_typed(const double* pos, const double* cell, const int32_t* pbc, const int64_t* frame_ptr,
                                          double r_max, const int64_t* atom_types, const double* cutoff_table,
                                          int64_t num_types, int64_t num_atoms, int64_t num_frames, void* workspace,
                                          int64_t workspace_bytes, int32_t* rowptr, int32_t* status, nqa_stream stream);
int nqa_neighbor_list_batched_fill_typed(const void* workspace, const int32_t* rowptr, const int64_t* atom_types,
                                         int64_t num_atoms, int64_t num_frames, int64_t num_types, int64_t num_edges,
                                         int64_t* edge_index, double* edge_cell_shift, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * STREAM / TERM / SLOT reductions: the form nqa_metrics_* and nqa_stats_* below share.
 *   A STREAM is one [rows, cols] row-major tensor (or pair of tensors) that is read once; a TERM is one quantity reduced over a
 *   stream; a term owns n_groups SLOTS, slot g collecting the elements of group g.  The term table is ordered by stream
 *   ("terms must be ordered by stream") and slot0 counts the slots of the terms before it ("slots must be contiguous in term
 *   order"); every stream carries at least one term ("a stream without terms").  A table that breaks one of these is refused
 *   with NQA_ERR_INVALID and that text under the entry point's name, before anything is launched.
 *   Two stages.  A fixed number of workgroups (NQA_*_GROUPS) walk every stream once and leave ONE row of per-slot partial
 *   accumulators each in `workspace`: [groups, slots] per 8-byte plane, nqa_*_workspace_bytes(total slots), 8-byte aligned.
 *   Inside a workgroup the elements of a slot are folded in element order by a fixed number of owner threads, whose parts are
 *   merged in part order.  The second stage merges the rows in row order, and where lanes of a wavefront hold partial results
 *   lane l takes lane l + off behind itself, off = 32 .. 1.  No floating-point atomics and a fixed merge order everywhere: the
 *   same inputs give the same bits.
 * ------------------------------------------------------------------------------------------- */

/* ---------------------------------------------------------------------------------------------
 * Losses and error metrics on one fused reduction: what nequip.train.MetricsManager.forward evaluates entry by entry
 *   (nequip/train/metrics_manager.py:283-373; the metric classes of nequip/train/metrics.py on nequip/data/stats.py::_MeanX;
 *   nequip/data/modifier.py::PerAtomModifier), without boolean indexing, masked_select or a host read.
 *   A STREAM is one distinct (prediction, target) pair: [rows, cols] row-major, float32 or float64 each (either
 *   combination); optional row_scale [rows] float64 applied to BOTH sides (PerAtomModifier: factor / num_atoms); optional
 *   group [rows] int64 (the atom types, for per-type terms).  With p, t promoted to float64 FIRST (the reference subtracts in
 *   the tensors' own dtype and promotes afterwards): d = p scale - t scale.
 *   A TERM is one metric on a stream; it owns n_groups slots (1, or T: slot g collects the rows with group == g).  Per slot:
 *   sum of m(d) (float64), count of contributing elements (int64), max |d| (float64), where m is d^2 (MSE, RMSE), |d|
 *   (MAE), Huber (|d| < delta ? d^2 / 2 : delta (|d| - delta / 2), strict <) or stratified Huber (the delta of the stratum
 *   i with |t row| >= bound[i] and not |t row| >= bound[i + 1]; strata in the given order, the last match wins, a row in no
 *   stratum adds 0).  ignore_nan: an element whose TARGET is NaN contributes to nothing of that term.
 *   Slot value: sum / count (MSE, MAE, Huber kinds with reduce_sum == 0), sqrt(sum / count) (RMSE), sum (reduce_sum != 0),
 *   max (-inf without elements); no element: 0 / 0 = NaN.  Term value: the slot value, or over the groups whose value is not
 *   NaN the equal mean / sum(c_g v_g) / sum(c_g) with has_group_coeffs.  weighted_sum = sum over the terms with has_coeff of
 *   coeff * term value, in term order.
 *   The term table (ordered as described above): out0 is the index of the term's first returned value
 *   (n_groups > 1: out0 + g per group, out0 + n_groups the aggregate).  It is read on the device (terms_device: a device
 *   copy of the host table `terms`, which the entry points use for checking and sizing); streams are passed by value.
 * nqa_metrics_fwd: two launches, the two stages described above.  NQA_METRICS_GROUPS workgroups (nqa_metrics_groups) leave
 *   their rows of partials (sum, count, max) in `workspace` (nqa_metrics_workspace_bytes(total slots)); one workgroup
 *   adds the rows in row order and writes values [n_values] (float64),
 *   saved [2, slots] (batch sums float64, counts int64: for the backward) and, if state != NULL, adds the batch to the running
 *   state [3, slots] (sum float64, count int64, max float64; the caller initialises 0, 0, -inf).  rows == 0 is valid.
 *   The first launch keeps 256 float64 values per term of one stream in LDS: from about 30 terms on ONE stream it asks the
 *   device for more than 64 KiB (at most 102 KiB at the limits) and returns NQA_ERR_LAUNCH if that is not granted.
 * nqa_metrics_bwd: one launch.  grad_values [n_values] is the upstream gradient over ALL returned values; every stream with
 *   grad_pred != NULL gets [rows, cols] in the prediction's dtype, every element written, the contributions of all its terms
 *   summed, with m'(d), the row scale, 1 / count, 1 / (2 rmse) and the group weights folded in; masked elements exactly 0.
 *   Max-abs terms are metrics, computed detached: no gradient.  Targets get no gradient.  Once differentiable.
 *   No allocation, no host synchronisation: forward, state update and backward capture into a hipGraph.
 * ------------------------------------------------------------------------------------------- */
#define NQA_METRICS_MAX_STREAMS 8
#define NQA_METRICS_MAX_TERMS 32
#define NQA_METRICS_MAX_TYPES 16
#define NQA_METRICS_MAX_STRATA 8
#define NQA_METRICS_GROUPS 64

enum nqa_metric_kind {
  NQA_METRIC_MSE = 0,
  NQA_METRIC_MAE = 1,
  NQA_METRIC_RMSE = 2,
  NQA_METRIC_MAXABS = 3,
  NQA_METRIC_HUBER = 4,
  NQA_METRIC_STRATIFIED_HUBER = 5
};

typedef struct nqa_metric_stream {
  const void* pred;        /* [rows, cols] */
  const void* target;      /* [rows, cols] */
  const double* row_scale; /* optional [rows] */
  const int64_t* group;    /* optional [rows] */
  void* grad_pred;         /* backward: optional [rows, cols], dtype of pred */
  int64_t rows;
  int32_t cols, pred_dtype, target_dtype, pad;
} nqa_metric_stream;

typedef struct nqa_metric_term {
  int32_t stream, kind, n_groups, ignore_nan, reduce_sum, n_strata, has_coeff, has_group_coeffs, slot0, out0;
  double coeff, delta;
  double bound[NQA_METRICS_MAX_STRATA], stratum_delta[NQA_METRICS_MAX_STRATA];
  double group_coeff[NQA_METRICS_MAX_TYPES];
} nqa_metric_term;

int32_t nqa_metrics_groups(void);
int64_t nqa_metrics_workspace_bytes(int32_t n_slots);
int nqa_metrics_fwd(const nqa_metric_stream* streams, int32_t n_streams, const nqa_metric_term* terms,
                    const nqa_metric_term* terms_device, int32_t n_terms, int32_t n_values, int32_t weighted_sum_index,
                    void* workspace, int64_t workspace_bytes, void* state, void* saved, double* values, nqa_stream stream);
int nqa_metrics_bwd(const nqa_metric_stream* streams, int32_t n_streams, const nqa_metric_term* terms,
                    const nqa_metric_term* terms_device, int32_t n_terms, int32_t n_values, int32_t weighted_sum_index,
                    const void* saved, const double* grad_values, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * The multi-tensor chunk layout of the five sections that follow (weight averaging, schedule-free AdamW, Adam, ConFIG,
 *   per-tensor statistics): launches over device-resident tables.  `tensors` [n] is the tensor table, one record per tensor (or per set of
 *   tensors of one shape that are walked together), float32 or float64, dense.  `chunks` [chunk_capacity] is the chunk map: the
 *   tensor a chunk belongs to and the element offset at which it starts.  A chunk is NQA_EMA_CHUNK elements (nqa_ema_chunk_elems;
 *   NQA_TSTATS_CHUNK, nqa_tstats_chunk_elems, for the statistics), the last one of a tensor shorter; a tensor without elements
 *   has an entry and no chunk.  One workgroup takes one chunk.  The grid is chunk_capacity; *n_chunks (device memory, int64) says
 *   how many entries of the map are in use and the workgroups past it return, so the tables can be rewritten in place under a
 *   captured launch.  An entry that does not lie inside its tensor is skipped, nothing is read or written through it.  Pointers
 *   need only be element-aligned: accesses are 16 bytes per lane where all pointers of a chunk are 16-byte aligned, element by
 *   element otherwise.
 * ------------------------------------------------------------------------------------------- */
typedef struct nqa_mt_chunk {
  int64_t offset; /* first element of the chunk within its tensor */
  int32_t tensor, pad;
} nqa_mt_chunk;

/* ---------------------------------------------------------------------------------------------
 * Exponential moving average of the model weights (nequip/train/ema.py::EMAWeights) as multi-tensor launches over the chunk
 *   layout above: one table entry per EMA buffer / parameter pair.
 * nqa_ema_update: with n = *counter (device memory, int64): n == 0 copies param into ema (ema may hold anything); otherwise
 *   w = 1 - min(decay, (1 + n) / (10 + n)) in double, rounded to float for float32 tensors, and
 *   ema = w < 0.5 ? ema + w (param - ema) : param - (param - ema) (1 - w)  (ATen's lerp).  Then *counter += 1, by a second
 *   one-thread launch on the same stream (no workgroup of the first sees the advanced value).  chunk_capacity == 0: only
 *   the counter moves.
 * nqa_ema_swap: exchanges ema and param element by element in registers: bit-exact, no temporary, one launch.
 *   No allocation, no host synchronisation: both capture into a hipGraph, and each replay of an update advances the warm-up.
 * ------------------------------------------------------------------------------------------- */
#define NQA_EMA_CHUNK 1024

typedef struct nqa_ema_tensor {
  void* ema;
  void* param;
  int64_t numel;
  int32_t dtype, pad; /* nqa_dtype */
} nqa_ema_tensor;

int32_t nqa_ema_chunk_elems(void);
int nqa_ema_update(const nqa_ema_tensor* tensors, const nqa_mt_chunk* chunks, int64_t chunk_capacity, const int64_t* n_chunks,
                   double decay, int64_t* counter, nqa_stream stream);
int nqa_ema_swap(const nqa_ema_tensor* tensors, const nqa_mt_chunk* chunks, int64_t chunk_capacity, const int64_t* n_chunks,
                 nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Schedule-free AdamW (the optimizer nequip/train/schedulefree.py::ScheduleFreeLightningModule is driven with) as multi-tensor
 *   launches over the chunk layout above: a table entry is (parameter, .grad, z, exp_avg_sq), the four of one dtype, and `group`
 *   indexes `groups` [n_groups]: the hyper-parameters AND the state of every parameter group, in device memory, so that a
 *   captured step advances.  A chunk whose `group` is outside [0, n_groups) is skipped.
 * nqa_sfree_step: per group, from the OLD state, in double (each rounded once to float for float32 tensors):
 *       sched = k < warmup_steps ? (k + 1) / warmup_steps : 1,  bc2 = 1 - beta2^(k+1),  lr_k = lr sched,
 *       lr_max' = max(lr_k, lr_max),  weight = (k + 1)^r lr_max'^weight_lr_power,  weight_sum' = weight_sum + weight,
 *       c = weight_sum' == 0 ? 0 : weight / weight_sum'
 *   and per element of every tensor whose `grad` is not null (the others are skipped, their state untouched)
 *       v = beta2 v + (1 - beta2) g g,  gn = g / (sqrt(v / bc2) + eps) + weight_decay y,
 *       y = lerp(y, z, c) + lr_k (beta1 (1 - c) - 1) gn,  z = z - lr_k gn
 *   with ATen's lerp (nqa_ema_update) and y the parameter; for k == 0, z is read as y (z may hold anything).  `grad` is only
 *   read.  Then k += 1, weight_sum = weight_sum', lr_max = lr_max', scheduled_lr = lr_k, by a second launch with one thread per
 *   group on the same stream (no workgroup of the first sees the advanced state).  chunk_capacity == 0: only the state moves.
 * nqa_sfree_swap: param = lerp(param, z, w) for every tensor of the table, w = 1 - 1 / beta1 with `to_eval` (the parameter
 *   then holds the averaged weights x), w = 1 - beta1 without (it holds y again).  beta1 == 0 has no way to x.
 *   No allocation, no host synchronisation: both capture into a hipGraph.
 * ------------------------------------------------------------------------------------------- */
typedef struct nqa_sfree_tensor {
  void* param;
  void* grad; /* null: skipped by nqa_sfree_step */
  void* z;
  void* exp_avg_sq;
  int64_t numel;
  int32_t dtype, group; /* nqa_dtype, index into the group records */
} nqa_sfree_tensor;

typedef struct nqa_sfree_group {
  double lr, beta1, beta2, eps, weight_decay, r, weight_lr_power;
  int64_t warmup_steps;
  int64_t k; /* steps done */
  double weight_sum, lr_max, scheduled_lr;
} nqa_sfree_group;

int nqa_sfree_step(const nqa_sfree_tensor* tensors, const nqa_mt_chunk* chunks, int64_t chunk_capacity, const int64_t* n_chunks,
                   nqa_sfree_group* groups, int32_t n_groups, nqa_stream stream);
int nqa_sfree_swap(const nqa_sfree_tensor* tensors, const nqa_mt_chunk* chunks, int64_t chunk_capacity, const int64_t* n_chunks,
                   const nqa_sfree_group* groups, int32_t n_groups, int32_t to_eval, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Adam / AdamW (torch.optim.Adam, torch.optim.AdamW) with gradient clipping, and ReduceLROnPlateau
 *   (torch.optim.lr_scheduler.ReduceLROnPlateau): the optimizer and scheduler of the reference's default training recipe, as
 *   multi-tensor launches over the chunk layout above.  A table entry is (parameter, .grad, exp_avg, exp_avg_sq, max_exp_avg_sq,
 *   step), the tensors of one dtype and `step` a 0-d float32 in device memory, the count of steps THIS parameter has taken (as
 *   torch's capturable and fused Adam keep it); `group` indexes `groups` [n_groups]: the hyper-parameters of every parameter
 *   group, in device memory, so that a captured launch sees a rewritten lr.  A chunk whose `group` is outside [0, n_groups) is
 *   skipped.  `counts` [2] (device memory, int64) = {chunks in use, tensors in use}; `tensor_capacity` is the length of `tensors`.
 * nqa_adam_step: per tensor whose `grad` is not null (the others are skipped, their state and step untouched), from the OLD
 *   *step, in double (each scalar rounded once to float for float32 tensors):
 *       s = *step + 1,  bc1 = 1 - beta1^s,  bc2 = 1 - beta2^s,  step_size = lr / bc1,  bc2_sqrt = sqrt(bc2)
 *   and per element, torch's _single_tensor_adam with p the parameter, m = exp_avg, v = exp_avg_sq:
 *       g = grad;  factor != 1: g = g factor;  g = clamp(g, -clip_value, clip_value) (a NaN passes);  maximize: g = -g
 *       weight_decay != 0:  decoupled: p = p (1 - lr weight_decay),  otherwise: g = g + weight_decay p
 *       m = lerp(m, g, 1 - beta1)  (ATen's lerp, nqa_ema_update),  v = beta2 v + (1 - beta2) g g
 *       amsgrad: max_exp_avg_sq = max(max_exp_avg_sq, v) (a NaN of either stays) and v' = max_exp_avg_sq, otherwise v' = v
 *       p = p - step_size m / (sqrt(v') / bc2_sqrt + eps)
 *   `grad` is only read.  `clip` is the clipping record: factor is exactly 1 and clip_value +inf without clipping.  Then
 *   *step += 1 for every entry with a `grad`, by a second launch with one thread per table entry on the same stream (no
 *   workgroup of the first sees the advanced count).  chunk_capacity == 0: only the counts move.
 * nqa_adam_grad_norm: two launches.  (1) One wavefront per chunk sums the squares of the chunk's `grad` elements in double (a
 *   lane its elements in ascending order, the lanes by a fixed tree) into partials [chunk_capacity]; a chunk without `grad` gives
 *   0.  (2) One wavefront adds the partials in use (lane l a contiguous run in index order, then the 64 lane sums in lane order)
 *   and writes clip->norm = sqrt(sum) and clip->factor = min(1, max_norm / (norm + 1e-6)) (clip_grad_norm_'s; a NaN stays, as
 *   with error_if_nonfinite=False).  No floating-point atomics: the same inputs give the same bits.
 * nqa_adam_plateau: one launch of one thread, torch's ReduceLROnPlateau.step(metric) with the metric (float32 or float64) read
 *   through a device pointer: last_epoch += 1; the metric is better than `best` when (min, rel) metric < best (1 - threshold),
 *   (min, abs) metric < best - threshold, (max, rel) metric > best (threshold + 1), (max, abs) metric > best + threshold; then
 *   best = metric, num_bad_epochs = 0, otherwise num_bad_epochs += 1; cooldown_counter > 0: cooldown_counter -= 1,
 *   num_bad_epochs = 0; num_bad_epochs > patience: for every group new_lr = max(lr factor, min_lr) and lr = new_lr where
 *   lr - new_lr > eps, cooldown_counter = cooldown, num_bad_epochs = 0.  Double arithmetic without contraction: every
 *   comparison is the IEEE operation of torch's Python.
 *   No allocation, no host synchronisation: all three capture into a hipGraph.
 * ------------------------------------------------------------------------------------------- */
typedef struct nqa_adam_tensor {
  void* param;
  const void* grad; /* null: skipped */
  void* exp_avg;
  void* exp_avg_sq;
  void* max_exp_avg_sq; /* null without amsgrad */
  float* step;          /* 0-d float32: the steps this parameter has taken */
  int64_t numel;
  int32_t dtype, group; /* nqa_dtype, index into the group records */
} nqa_adam_tensor;

typedef struct nqa_adam_group {
  double lr, beta1, beta2, eps, weight_decay;
  int32_t amsgrad, maximize, decoupled, pad;
  double min_lr; /* of the scheduler */
} nqa_adam_group;

typedef struct nqa_adam_clip {
  double norm;       /* written by nqa_adam_grad_norm: the norm of all gradients before clipping */
  double factor;     /* written by nqa_adam_grad_norm; exactly 1 when clipping by norm is off */
  double max_norm;   /* the bound of clipping by norm */
  double clip_value; /* the bound of clipping by value; +inf when off */
} nqa_adam_clip;

typedef struct nqa_adam_plateau_state {
  double best;
  int64_t num_bad_epochs, cooldown_counter, last_epoch;
  double factor, threshold, eps;
  int64_t patience, cooldown;
  int32_t mode_max, threshold_abs; /* 0: "min" / "rel" */
} nqa_adam_plateau_state;

int nqa_adam_step(const nqa_adam_tensor* tensors, int64_t tensor_capacity, const nqa_mt_chunk* chunks, int64_t chunk_capacity,
                  const int64_t* counts, const nqa_adam_group* groups, int32_t n_groups, const nqa_adam_clip* clip,
                  nqa_stream stream);
int nqa_adam_grad_norm(const nqa_adam_tensor* tensors, const nqa_mt_chunk* chunks, int64_t chunk_capacity, const int64_t* counts,
                       double* partials, nqa_adam_clip* clip, nqa_stream stream);
int nqa_adam_plateau(const void* metric, int32_t metric_dtype, nqa_adam_plateau_state* state, nqa_adam_group* groups,
                     int32_t n_groups, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Conflict-free inverse gradients, ConFIG (nequip/train/config.py::ConFIGLightningModule._ConFIG_backwards) as multi-tensor
 *   launches over the chunk layout above, with the records of the weight averaging: in an nqa_ema_tensor `ema` is the .grad of a
 *   parameter, `param` its slice of ROW 0 of the buffer of collected gradients [n_terms, row_stride] (`buf_dtype`: float64 if any
 *   .grad is, else float32; row_stride a multiple of 4 elements, the elements past the last slice zero).
 *   The tables live in device memory and are not validated by these calls: an entry with a float64 .grad under a float32
 *   buffer is outside the contract (the buffer dtype rule above excludes it) and such a chunk is skipped, neither read nor written.
 * nqa_config_collect: row `row` of the buffer = .grad (widened exactly), then .grad = 0, in one pass.  row < 0: only the zeros.
 * nqa_config_gram: two launches.  (1) One workgroup per NQA_CONFIG_GRAM_CHUNK elements of the rows (grid gram_capacity, the row
 *   length *numel read from device memory) forms the n_terms (n_terms + 1) / 2 products g_k . g_l in double and writes them to
 *   partials[chunk][pair] (gram_capacity * 36 doubles at most).  (2) One workgroup adds the partials in a fixed order and solves
 *       n_k = max(sqrt(G_kk), eps), Gh_kl = G_kl / (n_k n_l), bh = b / max(|b|, eps), c = pinv(Gh) bh (cyclic Jacobi, eigenvalues
 *       <= 1e-12 lambda_max dropped), xi = sqrt(max(c' Gh c, 0)), d = max(xi, eps), s = (sum_kl G_kl c_l / n_l) / d,
 *       w_l = s c_l / (n_l d), |new_grad| = |s| xi / d
 *   and writes out[NQA_CONFIG_OUT] = [w_0 .. w_7 (0 past n_terms), |new_grad|, factor]; with NQA_CONFIG_CLIP_NORM factor =
 *   min(1, clip / (|new_grad| + 1e-6)) and w is multiplied by it, otherwise factor = 1.  `b`: n_terms doubles on the device.
 *   No floating-point atomics: the same rows give the same bits.
 * nqa_config_apply: .grad[i] = (dtype of the .grad) clamp(sum_l weights[l] row_l[i]), the sum in double; the clamp to +-clip
 *   only with NQA_CONFIG_CLIP_VALUE (NaN passes).  `weights`: n_terms doubles on the device (the head of `out`).
 *   No allocation, no host synchronisation: all capture into a hipGraph.
 * nqa_config_solve_host: the solve of launch (2) on the host, all pointers host memory, `gram` the upper triangle row by row
 *   (for tests without a GPU; it runs the very function the kernel runs).
 * ------------------------------------------------------------------------------------------- */
#define NQA_CONFIG_GRAM_CHUNK 2048
#define NQA_CONFIG_MAX_TERMS 8
#define NQA_CONFIG_OUT 10

enum nqa_config_clip { NQA_CONFIG_CLIP_NONE = 0, NQA_CONFIG_CLIP_NORM = 1, NQA_CONFIG_CLIP_VALUE = 2 };

int32_t nqa_config_gram_chunk_elems(void);
int nqa_config_collect(const nqa_ema_tensor* tensors, const nqa_mt_chunk* chunks, int64_t chunk_capacity, const int64_t* n_chunks,
                       int32_t row, int64_t row_stride, int32_t buf_dtype, nqa_stream stream);
int nqa_config_gram(const void* buf, int32_t buf_dtype, int32_t n_terms, int64_t row_stride, const int64_t* numel,
                    int64_t gram_capacity, double* partials, const double* b, double norm_eps, int32_t clip_mode, double clip,
                    double* out, nqa_stream stream);
int nqa_config_apply(const nqa_ema_tensor* tensors, const nqa_mt_chunk* chunks, int64_t chunk_capacity, const int64_t* n_chunks,
                     int32_t n_terms, int64_t row_stride, int32_t buf_dtype, const double* weights, int32_t clip_mode, double clip,
                     nqa_stream stream);
int nqa_config_solve_host(const double* gram, int32_t n_terms, const double* b, double norm_eps, int32_t clip_mode, double clip,
                          double* out);

/* ---------------------------------------------------------------------------------------------
 * Dataset statistics on one fused reduction: what nequip.data.DataStatisticsManager.forward accumulates entry by entry
 *   (nequip/data/stats_manager.py:121-165 on the metric classes of nequip/data/stats.py; nequip/data/modifier.py::NumNeighbors),
 *   without boolean indexing, masked_select, unique or a host read.
 *   A STREAM is one distinct field tensor: [rows, cols] row-major, float32, float64, int32 or int64, promoted to float64;
 *   optional row_scale [rows] float64 (PerAtomModifier: factor / num_atoms).  Its group index, formed in the kernel:
 *   NQA_STATS_GROUP_NODE  atom_types[row];  NQA_STATS_GROUP_EDGE  atom_types[edge_index[0, row]] * T + atom_types[edge_index[1,
 *   row]] with edge_index [2, rows] int64, T = num_types; a type or an atom index out of range belongs to no group (the element
 *   still enters the terms with one slot).
 *   A TERM is one entry on a stream; it owns 1 slot, or T (node stream) / T * T (edge stream) slots: slot g collects the
 *   elements of group g.  ignore_nan: a NaN element contributes to nothing of that term; otherwise NaN propagates (through min
 *   and max as well).  The table is ordered as described above; both tables are HOST pointers, passed to the kernels by value.
 *   Running state [6, slots], 8 bytes each: count (int64), mean, mean_lo, M2 = sum (y - mean)^2, min, max (float64) of y = m(x)
 *   with m the term's modifier; the caller initialises 0, 0, 0, 0, +inf, -inf.  The mean is mean + mean_lo: mean the rounded
 *   value, mean_lo what the rounding lost, so that the difference of two means in Chan's merge keeps its digits when the data
 *   are large against their spread.  Every metric kind follows from the state: mean, sqrt(mean of squares), M2 / (count - 1),
 *   min, max, count.
 * nqa_stats_update: two launches for any number of terms and types, the two stages described above.  NQA_STATS_GROUPS
 *   workgroups (nqa_stats_groups) leave their rows of partial states in `workspace` (nqa_stats_workspace_bytes(total slots)):
 *   Welford updates in element order, Chan merges in the fixed order.  One wavefront per slot then merges the rows and the batch
 *   into the running state; a slot that received no element stays bit for bit.  No sum of squares is differenced.  All
 *   rows == 0: nothing is launched.
 * nqa_stats_neighbor_counts: counts [num_atoms] int32 = number of edges with edge_center[e] == atom (zeroed here, then integer
 *   atomics: exact, any edge order); an index outside [0, num_atoms) is skipped.  num_atoms == 0: nothing is launched.
 *   No allocation, no host synchronisation: both capture into a hipGraph.
 * ------------------------------------------------------------------------------------------- */
#define NQA_STATS_MAX_STREAMS 8
#define NQA_STATS_MAX_TERMS 32
#define NQA_STATS_MAX_NODE_TYPES 128
#define NQA_STATS_MAX_EDGE_TYPES 16
#define NQA_STATS_MAX_SLOTS 1024
#define NQA_STATS_GROUPS 256

enum nqa_stats_dtype { NQA_STATS_F32 = 0, NQA_STATS_F64 = 1, NQA_STATS_I32 = 2, NQA_STATS_I64 = 3 }; /* 0, 1: nqa_dtype */
enum nqa_stats_mod { NQA_STATS_MOD_IDENTITY = 0, NQA_STATS_MOD_ABS = 1, NQA_STATS_MOD_SQUARE = 2 };
enum nqa_stats_group { NQA_STATS_GROUP_NONE = 0, NQA_STATS_GROUP_NODE = 1, NQA_STATS_GROUP_EDGE = 2 };

typedef struct nqa_stats_stream {
  const void* data;          /* [rows, cols] */
  const double* row_scale;   /* optional [rows] */
  const int64_t* atom_types; /* grouped streams: [rows] (node) / [num_atoms] (edge) */
  const int64_t* edge_index; /* edge streams: [2, rows] */
  int64_t rows, num_atoms;
  int32_t cols, dtype, group_kind, num_types;
} nqa_stats_stream;

typedef struct nqa_stats_term {
  int32_t stream, mod, n_groups, ignore_nan, slot0, pad[3];
} nqa_stats_term;

int32_t nqa_stats_groups(void);
int64_t nqa_stats_workspace_bytes(int32_t n_slots);
int nqa_stats_update(const nqa_stats_stream* streams, int32_t n_streams, const nqa_stats_term* terms, int32_t n_terms,
                     void* workspace, int64_t workspace_bytes, void* state, nqa_stream stream);
int nqa_stats_neighbor_counts(const int64_t* edge_center, int64_t num_edges, int64_t num_atoms, int32_t* counts,
                              nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Per-tensor statistics of weights, gradients and Adam moments (nequip/train/callbacks/training_stats.py::
 *   TrainingStatsMonitor) as one multi-tensor reduction over the chunk layout above, with NQA_TSTATS_CHUNK elements per chunk:
 *   `tensors` [tensor_capacity] (transform f = identity or sqrt, applied element by element after the promotion to double;
 *   chunk0 the index of the tensor's first chunk in the map, its chunks are contiguous and ascending).  counts = [chunks in use,
 *   tensors in use] (device memory, int64): the grids are the two capacities and the workgroups past the counts return.
 * nqa_tstats_reduce: two launches.  With n = *counter (device memory, int64), every workgroup returns without touching a
 *   tensor, the workspace or the table unless n % log_freq == 0.  (1) One workgroup per chunk forms count, mean, M2, sum of
 *   squares, min, max, absmin, absmax of f(x) in double (Welford per lane, Chan merges in a fixed lane and wavefront order)
 *   and writes workspace[chunk] (chunk_capacity * 8 doubles).  (2) One wavefront per tensor merges its chunk rows in ascending
 *   order and writes table[tensor] = [min, max, mean, std (unbiased, NaN for one element), absmin, absmax, rms, count]
 *   (tensor_capacity * 8 doubles); *stamp = n.  One NaN makes all seven statistics NaN; with +-inf and no NaN, min, max,
 *   absmin, absmax and rms are exact and mean and std non-finite (Welford forms inf - inf).  No floating-point atomics: the same
 *   inputs give the same bits.  A capacity of 0: nothing is launched.
 * nqa_tstats_advance: *counter += 1 by a one-thread launch (a launch of its own, after every reduce launch of the step on the
 *   same stream: no workgroup of a reduce sees the advanced value).
 *   No allocation, no host synchronisation: both capture into a hipGraph; every replay advances the count and every
 *   log_freq-th replay rewrites the table.
 * ------------------------------------------------------------------------------------------- */
#define NQA_TSTATS_CHUNK 4096

enum nqa_tstats_transform { NQA_TSTATS_IDENTITY = 0, NQA_TSTATS_SQRT = 1 };

typedef struct nqa_tstats_tensor {
  const void* data;
  int64_t numel;
  int32_t dtype, transform; /* nqa_dtype, nqa_tstats_transform */
  int32_t chunk0, pad;
} nqa_tstats_tensor;

int32_t nqa_tstats_chunk_elems(void);
int nqa_tstats_reduce(const nqa_tstats_tensor* tensors, int64_t tensor_capacity, const nqa_mt_chunk* chunks,
                      int64_t chunk_capacity, const int64_t* counts, const int64_t* counter, int64_t log_freq, double* workspace,
                      double* table, int64_t* stamp, nqa_stream stream);
int nqa_tstats_advance(int64_t* counter, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Nose-Hoover / velocity-Verlet molecular dynamics (the scheme of nequip/ase/nosehoover.py) with the state in device memory:
 *   positions, velocities, masses (float64, [N, 3] / [N]) and the record below.  One MD step is nqa_md_step followed by
 *   nqa_md_bath on the same stream, then one force evaluation at the new positions by the caller.
 *   With F the force at the current positions (float32 or float64, promoted on load), m the masses, hdt = dt / 2:
 * nqa_md_step: flat over the 3N components (component i belongs to atom i / 3), one launch.
 *   (1) unless state->fresh: v = (v + hdt F/m) / (1 + hdt xi), which completes the PREVIOUS step (its last line needs this
 *       step's force; between two steps `velocities` holds the half-step velocities);
 *   (2) a = F/m - xi v;  x += dt v + dt^2/2 a;  v_half = v + hdt a, written to `velocities`.
 *   Workgroup b (NQA_MD_THREADS components) writes partials[2b] = sum m v^2 over the completed velocities of (1) and
 *   partials[2b + 1] = sum m v_half^2, both summed in a fixed order; `partials` holds 2 * nqa_md_num_partials(N) doubles.
 *   NQA_MD_FINISH_ONLY: only (1), written to `vel_out` ([N, 3], required in this mode); positions, velocities and the record are
 *   not written, partials[2b + 1] = 0.  Give this mode a partials table of its own if the sums of the last step are still needed.
 * nqa_md_bath: one wavefront; adds the rows of `partials` in a fixed order to S = sum m v^2 and S_half = sum m v_half^2, then
 *   with NQA_MD_THERMOSTAT: xi_half = xi + hdt (S - g) / (2 Q);  xi = xi_half + hdt (S_half - g) / (2 Q)   (without: xi untouched)
 *   kinetic_energy = S / 2 (of the completed velocities, i.e. at the START of this step);  nsteps += 1;  fresh = 0.
 *   NQA_MD_FINISH_ONLY: observed_kinetic_energy = S / 2 and nothing else.
 *   The record is rewritten by this second launch so that no workgroup of nqa_md_step sees the new xi (launches of one stream
 *   run in order).  g = (3N + 1) kB T, as in the reference.  The host may rewrite dt, g and q in place between steps.
 *   No floating-point atomics, no fused multiply-adds: the same inputs give the same bits, and (1) gives the same bits in both
 *   modes.  No allocation, no host synchronisation: both capture into a hipGraph.
 * ------------------------------------------------------------------------------------------- */
#define NQA_MD_THREADS 256

enum nqa_md_mode { NQA_MD_FINISH_ONLY = 1, NQA_MD_THERMOSTAT = 2 };

typedef struct nqa_md_state {
  double dt, g, q, xi, kinetic_energy;
  int64_t nsteps, fresh; /* fresh != 0: `velocities` holds completed velocities, (1) is skipped */
  double observed_kinetic_energy;
} nqa_md_state;

int64_t nqa_md_num_partials(int64_t num_atoms);
int nqa_md_step(int32_t force_dtype, const void* forces, const double* masses, double* positions, double* velocities,
                double* vel_out, int64_t num_atoms, const nqa_md_state* state, double* partials, int32_t mode, nqa_stream stream);
int nqa_md_bath(const double* partials, int64_t num_partials, nqa_md_state* state, int32_t mode, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Langevin dynamics, BAOAB splitting (Leimkuhler-Matthews), on the same state: positions, velocities, masses, the nqa_md_state
 *   record (its dt, nsteps, fresh and the two kinetic energies; g, q and xi are unused) and the parameter record below.  One MD
 *   step is nqa_md_langevin_step followed by nqa_md_bath WITHOUT NQA_MD_THERMOSTAT on the same stream, then one force evaluation
 *   at the new positions by the caller.  With F the force at the current positions, hdt = dt / 2:
 * nqa_md_langevin_step: flat over the 3N components as nqa_md_step, one launch.
 *   (1) unless state->fresh: v = v + hdt F/m, which completes the PREVIOUS step (between two steps `velocities` holds v2);
 *   (2) B  v1 = v + hdt F/m;   A  x += hdt v1;   O  v2 = c1 v1 + (c2 sqrt(kT/m)) z;   A  x += hdt v2;   v2 written to `velocities`.
 *   c1 = exp(-friction dt) and c2 = sqrt(1 - c1^2) are the host's, in float64 (friction = 0: c1 = 1, c2 = 0, velocity Verlet).
 *   The noise z of component i at step s = state->nsteps (before nqa_md_bath increments it) with the 64-bit seed:
 *     (w0, w1, w2, w3) = Philox4x32-10(counter = (i & 0xffffffff, i >> 32, s & 0xffffffff, s >> 32), key = (seed & 0xffffffff, seed >> 32))
 *       multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85; ten rounds, the key bumped between rounds
 *     u1 = ((w0 >> 5) * 67108864.0 + (w1 >> 6) + 1.0) * 2^-53   in (0, 1]
 *     u2 = ((w2 >> 5) * 67108864.0 + (w3 >> 6)) * 2^-53         in [0, 1)
 *     z  = sqrt(-2 log(u1)) * cos(6.283185307179586 * u2)       (the second Box-Muller value is dropped)
 *   and of nothing else: not the grid, not the number of atoms, not what was read in between.
 *   Workgroup b writes partials[2b] = sum m v^2 over the completed velocities of (1) and partials[2b + 1] = sum m v2^2, summed in
 *   the order of nqa_md_step.
 *   NQA_MD_FINISH_ONLY: only (1), written to `vel_out` ([N, 3], required in this mode); positions, velocities and the records are
 *   not written, partials[2b + 1] = 0.  NQA_MD_THERMOSTAT is not a mode of this entry.
 * nqa_md_bath (without the thermostat bit): kinetic_energy = S / 2, nsteps += 1, fresh = 0; finish-only: observed_kinetic_energy.
 *   The record is rewritten by that second launch, so no workgroup of the step sees the incremented nsteps.  The host may rewrite
 *   dt, c1, c2, kT and seed in place between steps; a captured pair of launches draws fresh noise at every replay.
 * nqa_md_noise: the generator alone, through the same device function: for components 0 .. count - 1 of (seed, step) the four
 *   Philox words (`words`, [count, 4]) and / or z (`normals`, [count]); either may be NULL, not both.
 *   No atomics, no FMA contraction, no allocation, no host synchronisation: captures into a hipGraph.
 * ------------------------------------------------------------------------------------------- */
typedef struct nqa_md_langevin_params {
  double c1, c2, kT; /* exp(-friction dt), sqrt(1 - c1^2), kB T */
  uint64_t seed;
} nqa_md_langevin_params;

int nqa_md_langevin_step(int32_t force_dtype, const void* forces, const double* masses, double* positions, double* velocities,
                         double* vel_out, int64_t num_atoms, const nqa_md_state* state, const nqa_md_langevin_params* params,
                         double* partials, int32_t mode, nqa_stream stream);
int nqa_md_noise(uint64_t seed, uint64_t step, int64_t count, uint32_t* words, double* normals, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Isotropic NPT: the Langevin step above followed by a stochastic cell rescaling barostat (Bernetti and Bussi 2020, first order
 *   in the volume), for ONE system whose cell (`cell`, [3, 3] float64, rows are the lattice vectors) lives on the device.  One
 *   step is nqa_md_langevin_step (unchanged), nqa_md_npt_bath IN PLACE OF nqa_md_bath, nqa_md_npt_scale, on the same stream,
 *   then one force evaluation at the new positions and cell by the caller.  `stress` ([3, 3], float32 or float64, promoted on
 *   load) is the potential stress at the positions and cell of the start of the step, (1/V) dE/d(strain).
 * nqa_md_npt_bath: one wavefront; adds the rows of `partials` in the order of nqa_md_bath to S = sum m v^2, then lane 0:
 *   K = S / 2;  V = |det cell| (cofactors along the first row);  P = (2 K) / (3 V) - (stress_00 + stress_11 + stress_22) / 3
 *   xi = the normal of nqa_md_langevin_step's generator for component `noise_index` (the host writes 3N: one past the atoms'
 *        components) at step s = state->nsteps with params->seed
 *   d_eps = -a (p0 - P) + sqrt((2 kT a) / V) xi;  mu = exp(d_eps / 3)
 *   mu not finite or not V > 0: mu = 1 and `failed` = 1, which stays set until the host clears it.
 *   cell = mu cell;  mu, pressure = P, kinetic_energy = K, volume = V (BEFORE the scaling) into the record; and, as nqa_md_bath,
 *   state->kinetic_energy = K, state->nsteps += 1, state->fresh = 0.
 *   a = compressibility dt / taup (the host's float64) and p0 (eV/A^3) may be rewritten in place between steps.  a = 0 gives
 *   mu = 1 exactly: the trajectory of nqa_md_langevin_step + nqa_md_bath bit for bit.
 * nqa_md_npt_scale: flat over the 3N components as nqa_md_step: x = mu x;  v2 = v2 / mu (a division), with the mu of the record.
 *   mu is written by the second launch and read by the third, nsteps by the second and read by the first of the next step: no
 *   launch sees a word that a launch of the same step rewrites after it started.  The finish-only readers are those of the
 *   Langevin step.  No atomics, no FMA contraction, no allocation, no host synchronisation: the three capture into a hipGraph.
 * ------------------------------------------------------------------------------------------- */
typedef struct nqa_md_npt_state {
  double a, p0;        /* compressibility dt / taup, target pressure: the host's */
  int64_t noise_index; /* 3N: the host's */
  double mu, pressure, kinetic_energy, volume;
  int64_t failed;
} nqa_md_npt_state;

int nqa_md_npt_bath(const double* partials, int64_t num_partials, nqa_md_state* state, const nqa_md_langevin_params* params,
                    nqa_md_npt_state* npt, int32_t stress_dtype, const void* stress, double* cell, nqa_stream stream);
int nqa_md_npt_scale(double* positions, double* velocities, int64_t num_atoms, const nqa_md_npt_state* npt, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Batched Langevin NVT and NPT: S independent systems concatenated along the atom axis (system s has n_s atoms, contiguous),
 *   each with its own records, as arrays: nqa_md_state[S], nqa_md_langevin_params[S], nqa_md_npt_state[S] (noise_index = 3 n_s),
 *   cells and stresses [S, 3, 3].  One step of the whole batch is nqa_md_batched_langevin_step + nqa_md_batched_bath (NVT), or
 *   nqa_md_batched_langevin_step + nqa_md_batched_npt_bath + nqa_md_batched_npt_scale (NPT), on the same stream, then one force
 *   evaluation by the caller.  System s takes, BIT FOR BIT, the steps that nqa_md_langevin_step + nqa_md_bath (or the NPT
 *   three) take for it alone with the same records, forces and stress: the arithmetic is the same device functions, and
 *   - the noise of a component is drawn for (seed of its system, nsteps of its system, j) with j the component's index INSIDE
 *     its system, 0 .. 3 n_s - 1, never the global index;
 *   - the components are cut into chunks (nqa_md_chunk): chunk k of system s covers its local components
 *     [NQA_MD_THREADS k, min(NQA_MD_THREADS (k + 1), 3 n_s)): the workgroups of nqa_md_langevin_step for n_s atoms.  A chunk may
 *     straddle two atoms, never two systems.  chunk_begin[s] .. chunk_begin[s + 1] are the chunks of system s, in order;
 *     there are nqa_md_num_partials(n_s) of them.  The host builds both tables once.
 * nqa_md_batched_langevin_step: one workgroup per chunk, one component per lane; (1) and (2) of nqa_md_langevin_step with dt,
 *   fresh, nsteps, c1, c2, kT and seed of the chunk's system.  Row c of `partials` (2 doubles per chunk) = the sums of chunk c.
 *   NQA_MD_FINISH_ONLY: only (1), into `vel_out`, as there.
 * nqa_md_batched_bath: one wavefront per system; lane b adds the contiguous run of ceil(P_s / 64) rows of its system in
 *   ascending order, the lanes are merged by the tree of nqa_md_bath; then kinetic_energy = S / 2, nsteps += 1, fresh = 0 (or, in
 *   the finish-only mode, observed_kinetic_energy) in the record of that system.  There is no thermostat bit.
 * nqa_md_batched_npt_bath: one wavefront per system; the sum as above, then lane 0 as in nqa_md_npt_bath with the records,
 *   stress and cell of that system.  A mu that is not finite or a cell without volume sets `failed` of that system alone.
 * nqa_md_batched_npt_scale: one workgroup per chunk: x = mu x;  v2 = v2 / mu with the mu of the chunk's system.
 *   The records are rewritten only by the second launch; mu is written by the second and read by the third: no launch sees a
 *   word that a launch of the same step rewrites after it started.  No atomics, no FMA contraction, no allocation, no host
 *   synchronisation: the launches capture into a hipGraph.  Every entry refuses null pointers, num_systems <= 0,
 *   num_chunks <= 0, unknown dtypes and unknown mode bits before anything is launched.
 * ------------------------------------------------------------------------------------------- */
typedef struct nqa_md_chunk {
  int64_t component0;    /* the flat (global) component of the chunk's first lane */
  int64_t local0;        /* the same component counted from the first of its system: NQA_MD_THREADS k */
  int32_t count, system; /* components component0 .. component0 + count - 1 (count <= NQA_MD_THREADS) of system `system` */
} nqa_md_chunk;

int nqa_md_batched_langevin_step(int32_t force_dtype, const void* forces, const double* masses, double* positions,
                                 double* velocities, double* vel_out, const nqa_md_chunk* chunks, int64_t num_chunks,
                                 const nqa_md_state* states, const nqa_md_langevin_params* params,
                                 double* partials /* 2 doubles per chunk */, int32_t mode, nqa_stream stream);
int nqa_md_batched_bath(const double* partials, const int64_t* chunk_begin /* [num_systems + 1] */, nqa_md_state* states,
                        int64_t num_systems, int32_t mode, nqa_stream stream);
int nqa_md_batched_npt_bath(const double* partials, const int64_t* chunk_begin, nqa_md_state* states,
                            const nqa_md_langevin_params* params, nqa_md_npt_state* npt, int32_t stress_dtype,
                            const void* stress /* [S, 3, 3] */, double* cell /* [S, 3, 3] */, int64_t num_systems,
                            nqa_stream stream);
int nqa_md_batched_npt_scale(double* positions, double* velocities, const nqa_md_chunk* chunks, int64_t num_chunks,
                             const nqa_md_npt_state* npt, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * FIRE structural relaxation (Bitzek et al. 2006; ASE's defaults and step cap; massless dynamics, fixed cell) with the state in
 *   device memory: positions and velocities (float64, [N, 3]) and one nqa_fire_system record per system.  A batch of independent
 *   systems is concatenated along the atom axis; the atoms are cut into chunks of at most NQA_FIRE_CHUNK atoms, none of which
 *   straddles two systems (nqa_fire_chunk; chunk_begin[s] .. chunk_begin[s + 1] are the chunks of system s, in atom order).
 *   One step is nqa_fire_reduce, nqa_fire_decide, nqa_fire_move on the same stream, then one force evaluation at the new
 *   positions by the caller.  F is the force at the current positions (float32 or float64, promoted on load); the components
 *   of atoms with fixed[i] != 0 count as zero everywhere (`fixed` may be NULL: no atom is fixed).
 * nqa_fire_reduce: one workgroup per chunk, one atom per lane.  Row b of `partials` (4 doubles per chunk) = over the atoms of
 *   chunk b:  sum F.v,  sum F.F,  sum v.v,  max (Fx^2 + Fy^2 + Fz^2)   (a NaN is kept by the max).
 * nqa_fire_decide: one wavefront per system; merges the rows of its chunks in a fixed order to P, FF, VV, M.  Then lane 0:
 *     fmax = sqrt(M);  converged = M < fmax_target^2            (both always written)
 *     if converged: nothing else changes (nsteps included)
 *     else if nsteps == 0:  cv = 0, cf = 0                      (the velocities are zero by construction: no branch is taken)
 *     else if P > 0:        cv = 1 - a;  cf = a sqrt(VV) / sqrt(FF)   (the old a)
 *                           if npos > nmin: dt = min(dt finc, dtmax), a = a fa
 *                           npos += 1
 *     else (NaN included):  cv = 0, cf = 0, a = astart, dt = dt fdec, npos = 0
 *     then, with the new dt:  c = cf + dt;  VVn = cv cv VV + 2 cv c P + c c FF;  normdr = dt sqrt(VVn)
 *                           scale = normdr > maxstep ? maxstep / normdr : 1;   nsteps += 1
 *   VVn is the squared norm of the velocities the move is about to form, from the sums of the old ones (every term is
 *   non-negative in both branches): it differs from a direct norm by rounding only and spares a third reduction.
 * nqa_fire_move: one workgroup per chunk, flat over its components; for systems that are not converged and atoms that are not
 *   fixed:  v = cv v + cf F;  v = v + dt F;  x = x + scale (dt v).
 *   The record is rewritten by the second launch and read by the third, so that no workgroup sees a half-written record
 *   (launches of one stream run in order).  The host may rewrite the parameter words in place between steps.
 *   No floating-point atomics, no fused multiply-adds, a fixed order of every sum: the same inputs give the same bits, and a
 *   system takes the same steps alone and inside a batch.  No allocation, no host synchronisation: the three capture into a
 *   hipGraph.
 * The record, sixteen 8-byte words:
 *   0 dt  1 a  2 npos  3 nsteps                                         state (decide advances it)
 *   4 dtmax  5 maxstep  6 finc  7 fdec  8 astart  9 fa  10 fmax_target   parameters (the host's)
 *   11 nmin (low 32 bits, the host's) and converged (high 32 bits, written by decide)
 *   12 cv  13 cf  14 scale  15 fmax                                      written by decide
 * ------------------------------------------------------------------------------------------- */
#define NQA_FIRE_CHUNK 256

typedef struct nqa_fire_system {
  double dt, a;
  int64_t npos, nsteps;
  double dtmax, maxstep, finc, fdec, astart, fa, fmax_target;
  int32_t nmin, converged;
  double cv, cf, scale, fmax;
} nqa_fire_system;

typedef struct nqa_fire_chunk {
  int64_t atom0;
  int32_t count, system; /* atoms atom0 .. atom0 + count - 1 (count <= NQA_FIRE_CHUNK) of system `system` */
} nqa_fire_chunk;

int32_t nqa_fire_chunk_atoms(void);
int nqa_fire_reduce(int32_t force_dtype, const void* forces, const double* velocities, const uint8_t* fixed /* [N] or NULL */,
                    const nqa_fire_chunk* chunks, int64_t n_chunks, double* partials /* 4 doubles per chunk */,
                    nqa_stream stream);
int nqa_fire_decide(const double* partials, const int64_t* chunk_begin /* [n_systems + 1] */, nqa_fire_system* systems,
                    int64_t n_systems, nqa_stream stream);
int nqa_fire_move(int32_t force_dtype, const void* forces, double* positions, double* velocities, const uint8_t* fixed,
                  const nqa_fire_chunk* chunks, int64_t n_chunks, const nqa_fire_system* systems, nqa_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Variable-cell FIRE: the FIRE above over the atoms and the cell together, as ASE's UnitCellFilter under opt.fire.FIRE, with the
 *   state in device memory.  Per system: n atoms, the reference cell C0 (rows = lattice vectors, taken at construction), the
 *   current cell C, the deformation gradient D = (C0^-1 C)^T, i.e. C = C0 D^T (D = I at the start), cell_factor (ASE: n).
 *   Generalised coordinates, n + 3 rows of 3:  q_i = x_i D^-T for the atoms (carried as state, never re-solved),
 *   Q = cell_factor D for the cell.  Generalised forces, with F the force and sigma the stress ([S, 3, 3], float32 or float64,
 *   sigma = (1/V) dE/d(strain), V = |det C|) at (x, C):
 *     atoms  g_i = F_i D  (row vector times matrix; the rows of atoms with fixed[i] != 0 count as zero; a fixed atom keeps its
 *            q_i, so its x_i = q_i D^T follows the cell)
 *     cell   W = -V (sigma + pressure I);  G = W D^-T;  then, in this order:
 *            hydrostatic:      G = (tr G / 3) I
 *            mask:             G = G * mask elementwise (nine doubles, 0 or 1)
 *            constant_volume:  tr G / 3 is subtracted from the diagonal
 *            finally           G = G / cell_factor
 * One step is nqa_cellfire_reduce, nqa_cellfire_decide, nqa_cellfire_move on the same stream, then one force evaluation at
 *   (x, C) by the caller.  Chunks, chunk_begin and `partials` are those of the fixed-cell kernels.
 * nqa_cellfire_reduce: one workgroup per chunk, one atom per lane; g is formed with the D of the record (d_new: the D at which F
 *   was evaluated).  Row b of `partials` = over the atoms of chunk b:  sum g.v,  sum g.g,  sum v.v,  max |g_i|^2.
 * nqa_cellfire_decide: one wavefront per system; merges the rows of its chunks in the fixed order.  Then lane 0, in plain C++:
 *     forms G (det and D^-T by cofactors), adds its nine components to P, FF, VV (against the cell velocity vd, row-major order)
 *     and its three row norms to M;  fmax = sqrt(M);  converged = M < fmax_target^2  (both always written; a NaN in a force or
 *     in the stress reaches fmax);  if converged nothing else changes;  else the FIRE branch of nqa_fire_decide, word for word,
 *     which gives cv, cf, dt, a, npos, scale, nsteps += 1;  then the cell move:
 *       d_old = d_new;  vd = cv vd + cf G;  vd = vd + dt G;  Q = cell_factor d_old;  Q = Q + scale (dt vd)
 *       d_new = Q / cell_factor;  C = C0 d_new^T, written to row s of `cell` ([S, 3, 3] float64: the buffer the force step reads)
 * nqa_cellfire_move: one workgroup per chunk, one atom per lane; for systems that are not converged:
 *       g = F d_old;  v = cv v + cf g;  v = v + dt g;  q = q + scale (dt v)    (skipped for fixed atoms)
 *       x = q d_new^T                                                          (fixed atoms included)
 *   The record hazards are those of the fixed-cell kernels: three launches of one stream.  No floating-point atomics, no fused
 *   multiply-adds, a fixed order of every sum, no allocation, no host synchronisation.
 * The record, sixty-four 8-byte words: 0 .. 15 are the words of nqa_fire_system, then
 *   16 cell_factor  17 pressure  18 hydrostatic (low 32 bits) and constant_volume (high 32 bits)      parameters (the host's)
 *   19 .. 27 mask  28 .. 36 c0                                                      parameters, 3 x 3 row-major
 *   37 .. 45 d_old  46 .. 54 d_new  55 .. 63 vd                                     state (decide advances it), 3 x 3 row-major
 * ------------------------------------------------------------------------------------------- */
typedef struct nqa_cellfire_system {
  double dt, a;
  int64_t npos, nsteps;
  double dtmax, maxstep, finc, fdec, astart, fa, fmax_target;
  int32_t nmin, converged;
  double cv, cf, scale, fmax;
  double cell_factor, pressure;
  int32_t hydrostatic, constant_volume;
  double mask[9], c0[9], d_old[9], d_new[9], vd[9];
} nqa_cellfire_system;

int nqa_cellfire_reduce(int32_t force_dtype, const void* forces, const double* velocities, const uint8_t* fixed /* [N] or NULL */,
                        const nqa_fire_chunk* chunks, int64_t n_chunks, const nqa_cellfire_system* systems,
                        double* partials /* 4 doubles per chunk */, nqa_stream stream);
int nqa_cellfire_decide(const double* partials, const int64_t* chunk_begin /* [n_systems + 1] */, int32_t stress_dtype,
                        const void* stress /* [n_systems, 3, 3] */, nqa_cellfire_system* systems, double* cell /* [n_systems, 3, 3] */,
                        int64_t n_systems, nqa_stream stream);
int nqa_cellfire_move(int32_t force_dtype, const void* forces, double* positions, double* coords /* q, [N, 3] */,
                      double* velocities, const uint8_t* fixed, const nqa_fire_chunk* chunks, int64_t n_chunks,
                      const nqa_cellfire_system* systems, nqa_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* NEQUIP_AMD_H */
