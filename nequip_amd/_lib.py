"""ctypes binding of ``libnequip_amd.so`` -- the C ABI declared in ``include/nequip_amd.h``.

There is deliberately no fallback: if the HIP library has not been built (``python -m
nequip_amd.csrc.build`` / ``__graft_entry__.build()``) every kernel-backed op raises.  Nothing in this
package computes the hot path on the CPU.
"""

from __future__ import annotations

import ctypes
import os
import threading
from ctypes import POINTER, c_char_p, c_double, c_int32, c_int64, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libnequip_amd.so")

NQA_OK = 0
NQA_F32 = 0
NQA_F64 = 1
NQA_MLP_FP32 = 0  # radial MLP GEMM on exact-fp32 MFMA
NQA_MLP_BF16X6 = 1  # ... on bf16 MFMA with 3-way split operands (fp32-accurate)
NQA_MLP_F16X3 = 2  # forward: scaled operands split into two fp16 terms, three products (fp32-accurate)
NQA_MLP_HINT_DEVICE_IS_IDLE = 0x100  # OR-ed into `mode` of nqa_radial_mlp_bwd: nothing runs next to this launch
NQA_LAYOUT_MUL_IR = 0
NQA_LAYOUT_IR_MUL = 1

NQA_PLAN_DIM_IN1 = 0
NQA_PLAN_DIM_IN2 = 1
NQA_PLAN_DIM_OUT = 2
NQA_PLAN_WEIGHT_NUMEL = 3
NQA_PLAN_NUM_INSTR = 4
NQA_PLAN_OUT_NEEDS_ZERO = 5
NQA_PLAN_YPART_WIDTH = 6
NQA_PLAN_HAS_SPECIALIZED = 7
NQA_PLAN_FUSED_ROWS_OK = 8

_P32 = POINTER(c_int32)


class GateBlock(ctypes.Structure):
    """``nqa_gate_block`` (include/nequip_amd.h): one block of a gate's output."""

    _fields_ = [("out_off", c_int32), ("d", c_int32), ("mul", c_int32), ("val_off", c_int32), ("gate_off", c_int32),
                ("act", c_int32), ("cst", c_double)]


class NodePart(ctypes.Structure):
    """``nqa_node_part`` (include/nequip_amd.h): one operand set + destination of ``nqa_node_fused``."""

    _fields_ = [("x", c_void_p), ("packed", c_void_p), ("chunk_table", c_void_p), ("instr_table", c_void_p),
                ("n_chunks", c_int32), ("n_instr", c_int32), ("n_types", c_int32), ("dim_in", c_int32),
                ("out", c_void_p), ("addend", c_void_p), ("dim_out", c_int32), ("accumulate", c_int32),
                ("scale", c_double), ("in_gate", c_void_p), ("n_in_gate", c_int32), ("pad", c_int32)]


NQA_METRICS_MAX_STREAMS = 8
NQA_METRICS_MAX_TERMS = 32
NQA_METRICS_MAX_TYPES = 16
NQA_METRICS_MAX_STRATA = 8
NQA_METRICS_GROUPS = 64  # workgroups (= rows of partials) of the first forward launch; nqa_metrics_groups()
NQA_METRIC_MSE, NQA_METRIC_MAE, NQA_METRIC_RMSE, NQA_METRIC_MAXABS, NQA_METRIC_HUBER, NQA_METRIC_STRATIFIED_HUBER = range(6)


class MetricStream(ctypes.Structure):
    """``nqa_metric_stream`` (include/nequip_amd.h): one distinct (prediction, target) pair of ``nqa_metrics_*``."""

    _fields_ = [("pred", c_void_p), ("target", c_void_p), ("row_scale", c_void_p), ("group", c_void_p),
                ("grad_pred", c_void_p), ("rows", c_int64), ("cols", c_int32), ("pred_dtype", c_int32),
                ("target_dtype", c_int32), ("pad", c_int32)]


class MetricTerm(ctypes.Structure):
    """``nqa_metric_term`` (include/nequip_amd.h): one metric attached to a stream."""

    _fields_ = [("stream", c_int32), ("kind", c_int32), ("n_groups", c_int32), ("ignore_nan", c_int32),
                ("reduce_sum", c_int32), ("n_strata", c_int32), ("has_coeff", c_int32), ("has_group_coeffs", c_int32),
                ("slot0", c_int32), ("out0", c_int32), ("coeff", c_double), ("delta", c_double),
                ("bound", c_double * NQA_METRICS_MAX_STRATA), ("stratum_delta", c_double * NQA_METRICS_MAX_STRATA),
                ("group_coeff", c_double * NQA_METRICS_MAX_TYPES)]


NQA_STATS_MAX_STREAMS = 8
NQA_STATS_MAX_TERMS = 32
NQA_STATS_MAX_NODE_TYPES = 128
NQA_STATS_MAX_EDGE_TYPES = 16
NQA_STATS_MAX_SLOTS = 1024  # all slots of one manager
NQA_STATS_GROUPS = 256  # workgroups (= rows of partial states) of the first launch; nqa_stats_groups()
NQA_STATS_F32, NQA_STATS_F64, NQA_STATS_I32, NQA_STATS_I64 = range(4)
NQA_STATS_MOD_IDENTITY, NQA_STATS_MOD_ABS, NQA_STATS_MOD_SQUARE = range(3)
NQA_STATS_GROUP_NONE, NQA_STATS_GROUP_NODE, NQA_STATS_GROUP_EDGE = range(3)


class StatsStream(ctypes.Structure):
    """``nqa_stats_stream`` (include/nequip_amd.h): one distinct field tensor of ``nqa_stats_update``."""

    _fields_ = [("data", c_void_p), ("row_scale", c_void_p), ("atom_types", c_void_p), ("edge_index", c_void_p),
                ("rows", c_int64), ("num_atoms", c_int64), ("cols", c_int32), ("dtype", c_int32), ("group_kind", c_int32),
                ("num_types", c_int32)]


class StatsTerm(ctypes.Structure):
    """``nqa_stats_term`` (include/nequip_amd.h): one statistics entry attached to a stream."""

    _fields_ = [("stream", c_int32), ("mod", c_int32), ("n_groups", c_int32), ("ignore_nan", c_int32), ("slot0", c_int32),
                ("pad", c_int32 * 3)]


# name -> (restype, argtypes); must list every symbol include/nequip_amd.h declares
SIGNATURES = {
    "nqa_abi_version": (c_int32, []),
    "nqa_last_error": (c_char_p, []),
    "nqa_lmax": (c_int32, []),
    "nqa_sh_lmax": (c_int32, []),
    "nqa_plan_create": (
        c_int32,
        [c_int32, _P32, _P32, _P32, c_int32, _P32, _P32, _P32, c_int32, _P32, _P32, _P32]
        + [c_int32, _P32, _P32, _P32, POINTER(c_double), c_int32, c_int32, POINTER(c_void_p)],
    ),
    "nqa_plan_destroy": (None, [c_void_p]),
    "nqa_plan_query": (c_int64, [c_void_p, c_int32]),
    "nqa_plan_image_bytes": (c_int64, [c_void_p]),
    "nqa_plan_image_write": (c_int32, [c_void_p, c_void_p, c_int64]),
    "nqa_csr_workspace_bytes": (c_int64, [c_int64, c_int64]),
    "nqa_csr_build": (
        c_int32,
        [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p],
    ),
    "nqa_tp_scatter_fwd": (
        c_int32,
        [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
        + [c_int64, c_int64, c_void_p],
    ),
    "nqa_tp_bwd_edge_workspace_bytes": (c_int64, [c_void_p, c_int32, c_int64]),
    "nqa_tp_scatter_bwd_edge": (
        c_int32,
        [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
        + [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p],
    ),
    "nqa_tp_bwd_fused_workspace_bytes": (c_int64, [c_void_p, c_int32, c_int64]),
    "nqa_tp_scatter_bwd_fused": (
        c_int32,
        [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]  # plan, image, dtype, x, y, w, grad_out
        + [c_void_p] * 5  # rowptr_dst, edge_id_dst, src_sorted, rowptr_src, edge_id_src
        + [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p],
    ),
    "nqa_tp_scatter_bwd_x": (
        c_int32,
        [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
        + [c_int64, c_int64, c_void_p],
    ),
    "nqa_frame_sum": (c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_int64, c_void_p, c_void_p]),
    "nqa_edge_pairs_workspace_bytes": (c_int64, [c_int64]),
    "nqa_edge_pairs": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p,
         c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "nqa_csr_from_pairs": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "nqa_pair_owner_workspace_bytes": (c_int64, [c_int64, c_int64]),
    "nqa_pair_owner_lists": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "nqa_pair_owner_lists_guard": (c_int32, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "nqa_pair_gather": (c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    "nqa_pair_expand": (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_int32, c_void_p, c_void_p]),
    "nqa_tp_bwd_pairs_workspace_bytes": (c_int64, [c_void_p, c_int32, c_int64]),
    "nqa_tp_scatter_bwd_pairs": (
        c_int32,
        [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]  # plan, image, dtype, x, y, w, grad_out
        + [c_void_p] * 7  # owner_rowptr, pair_other, pair_row, pair_edge_in, pair_edge_out, other_rowptr, other_slot
        + [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p],
    ),
    "nqa_tp_fwd_jvp_supported": (c_int32, [c_void_p, c_int32]),
    "nqa_tp_scatter_fwd_jvp": (
        c_int32,
        [c_void_p, c_void_p, c_int32] + [c_void_p] * 6  # plan, image, dtype, x, y, w, x_cot, y_cot, w_cot
        + [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p],
    ),
    "nqa_tp_scatter_bwd_x_dual": (
        c_int32,
        [c_void_p, c_void_p, c_int32] + [c_void_p] * 5  # plan, image, dtype, y, w, y_cot, w_cot, grad_out
        + [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p],
    ),
    "nqa_tp_bwd_pairs_dual_supported": (c_int32, [c_void_p, c_int32]),
    "nqa_tp_scatter_bwd_pairs_dual": (
        c_int32,
        [c_void_p, c_void_p, c_int32] + [c_void_p] * 7  # plan, image, dtype, x, x_cot, y, y_cot, w, w_cot, grad_out
        + [c_void_p] * 5  # owner_rowptr, pair_other, pair_row, pair_edge_in, pair_edge_out
        + [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p],
    ),
    "nqa_edge_vectors_fwd": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p],
    ),
    "nqa_edge_vectors_bwd": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_double, c_void_p, c_void_p, c_void_p],
    ),
    "nqa_virial_finalize": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "nqa_edge_embed_fwd": (
        c_int32,
        [c_int32, c_int32, c_void_p, c_int64, c_double, c_void_p, c_int32, c_void_p, c_double, c_double]
        + [c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "nqa_edge_embed_bwd": (
        c_int32,
        [c_int32, c_int32, c_void_p, c_int64, c_double, c_void_p, c_int32, c_void_p, c_double, c_double]
        + [c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "nqa_edge_embed_fwd_paired": (
        c_int32,
        [c_int32, c_int32, c_void_p, c_int64, c_double, c_int32, c_void_p, c_double, c_double, c_void_p, c_int64]
        + [c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "nqa_edge_embed_bwd_paired": (
        c_int32,
        [c_int32, c_int32, c_void_p, c_int64, c_double, c_int32, c_void_p, c_double, c_double, c_void_p, c_int64]
        + [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "nqa_edge_embed_bwd_bwd": (
        c_int32,
        [c_int32, c_int32, c_void_p, c_int64, c_double, c_void_p, c_int32, c_void_p, c_double, c_double]
        + [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "nqa_radial_mlp_supported": (c_int32, [c_int32, c_int32, c_int32, c_int32]),
    "nqa_radial_mlp_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32, c_int32]),
    "nqa_radial_mlp_fwd": (
        c_int32,
        [c_int32, c_int32, c_void_p, c_void_p, c_double, c_void_p, c_double, c_int32, c_int32, c_int32, c_int64]
        + [c_void_p, c_void_p, c_int64, c_int32, c_void_p],
    ),
    "nqa_radial_mlp_bwd": (
        c_int32,
        [c_int32, c_int32, c_void_p, c_void_p, c_double, c_void_p, c_double, c_void_p, c_int32, c_int32, c_int32]
        + [c_int64, c_void_p, c_void_p, c_int64, c_int32, c_void_p],
    ),
    "nqa_node_linear": (
        c_int32,
        [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32]
        + [c_int64, c_int32, c_int32, c_int64, c_double, c_int32, c_void_p],
    ),
    "nqa_node_weights_pack_bytes": (c_int64, [c_void_p, c_int32, c_void_p, c_int32, c_int32]),
    "nqa_node_weights_pack": (
        c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int64, c_void_p, c_void_p],
    ),
    "nqa_node_linear_packed": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32]
        + [c_int64, c_double, c_void_p],
    ),
    "nqa_node_linear_ordered": (
        c_int32,
        [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32,
         c_int64, c_int32, c_int32, c_int64, c_double, c_int32, c_void_p],
    ),
    "nqa_node_linear_packed_ordered": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32]
        + [c_int32, c_int64, c_double, c_void_p],
    ),
    "nqa_node_fused": (
        c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_int32, c_void_p],
    ),
    "nqa_node_fused_plan": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, _P32, c_int32, _P32, c_int32]),
    "nqa_radial_mlp_last_fwd": (
        c_int32,
        [c_int32, c_int32, c_void_p, c_void_p, c_double, c_int32, c_int32, c_int64, c_void_p, c_void_p, c_int64, c_int32,
         c_void_p],
    ),
    "nqa_radial_mlp_last_bwd": (
        c_int32,
        [c_int32, c_int32, c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_int32, c_int32, c_int64, c_void_p, c_void_p,
         c_int64, c_int32, c_void_p],
    ),
    "nqa_energy_head": (
        c_int32,
        [c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
         c_double, c_int64, c_void_p],
    ),
    "nqa_energy_head_train_workspace_bytes": (c_int64, [c_int64, c_int32, c_int32, c_int32]),
    "nqa_energy_head_train_bwd": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
         c_int64, c_int32, c_int32, c_double, c_int64, c_void_p],
    ),
    "nqa_energy_head_train_bwd_bwd": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
         c_int64, c_int32, c_int32, c_double, c_int64, c_void_p],
    ),
    "nqa_zbl_fwd": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double, c_int32, c_void_p, c_int64,
         c_int64, c_void_p, c_void_p, c_void_p],
    ),
    "nqa_zbl_bwd": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double, c_int32, c_void_p, c_int64,
         c_int64, c_void_p, c_void_p, c_void_p],
    ),
    "nqa_zbl_bwd_bwd": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double, c_int32, c_void_p, c_int64,
         c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "nqa_neighbor_list_workspace_bytes": (c_int64, [c_int64]),
    "nqa_neighbor_list_count": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_double, c_int64, c_void_p, c_int64, c_void_p, c_void_p],
    ),
    "nqa_neighbor_list_fill": (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "nqa_neighbor_list_fill_padded": (
        c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nqa_neighbor_list_batched_workspace_bytes": (c_int64, [c_int64, c_int64]),
    "nqa_neighbor_list_batched_count": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p],
    ),
    "nqa_neighbor_list_batched_fill": (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "nqa_neighbor_list_typed_workspace_bytes": (c_int64, [c_int64, c_int64]),
    "nqa_neighbor_list_count_typed": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_int64, c_int32, c_int64, c_void_p, c_int64, c_void_p,
         c_void_p, c_void_p],
    ),
    "nqa_neighbor_list_fill_typed": (
        c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "nqa_neighbor_list_fill_padded_typed": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nqa_neighbor_list_batched_typed_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64]),
    "nqa_neighbor_list_batched_count_typed": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64,
         c_void_p, c_void_p, c_void_p],
    ),
    "nqa_neighbor_list_batched_fill_typed": (
        c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "nqa_gate": (
        c_int32,
        [c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int64, c_void_p],
    ),
    "nqa_radial_mlp_bwd_paired": (
        c_int32,
        [c_int32, c_int32, c_void_p, c_void_p, c_double, c_void_p, c_double, c_void_p, c_void_p, c_int32, c_int32,
         c_int32, c_int64, c_void_p, c_void_p, c_int64, c_int32, c_void_p],
    ),
    "nqa_radial_mlp_train_tiles": (c_int64, [c_int64]),
    "nqa_radial_mlp_bwd_train": (
        c_int32,
        [c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_double, c_void_p, c_int32, c_int32,
         c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p],
    ),
    "nqa_radial_mlp_fwd_tangent": (
        c_int32,
        [c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_double, c_int32, c_int32, c_int32,
         c_int64, c_void_p, c_void_p, c_int64, c_int32, c_void_p],
    ),
    "nqa_wgrad_splits": (c_int32, [c_void_p, c_int32, c_int32, c_int64]),
    "nqa_wgrad": (
        c_int32,
        [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int64, c_int64, c_int32, c_int64, c_int32,
         c_void_p, c_void_p],
    ),
    "nqa_metrics_groups": (c_int32, []),
    "nqa_metrics_workspace_bytes": (c_int64, [c_int32]),
    "nqa_metrics_fwd": (
        c_int32,
        [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
         c_void_p],
    ),
    "nqa_metrics_bwd": (
        c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "nqa_ema_chunk_elems": (c_int32, []),
    "nqa_ema_update": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_double, c_void_p, c_void_p]),
    "nqa_ema_swap": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "nqa_sfree_step": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_void_p]),
    "nqa_sfree_swap": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    "nqa_adam_step": (c_int32, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "nqa_adam_grad_norm": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nqa_adam_plateau": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p]),
    "nqa_config_gram_chunk_elems": (c_int32, []),
    "nqa_config_collect": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int64, c_int32, c_void_p]),
    "nqa_config_gram": (
        c_int32, [c_void_p, c_int32, c_int32, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_double, c_int32, c_double,
                  c_void_p, c_void_p]),
    "nqa_config_apply": (
        c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int64, c_int32, c_void_p, c_int32, c_double, c_void_p]),
    "nqa_config_solve_host": (c_int32, [c_void_p, c_int32, c_void_p, c_double, c_int32, c_double, c_void_p]),
    "nqa_stats_groups": (c_int32, []),
    "nqa_stats_workspace_bytes": (c_int64, [c_int32]),
    "nqa_stats_update": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int64, c_void_p, c_void_p]),
    "nqa_stats_neighbor_counts": (c_int32, [c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "nqa_tstats_chunk_elems": (c_int32, []),
    "nqa_tstats_reduce": (
        c_int32, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nqa_tstats_advance": (c_int32, [c_void_p, c_void_p]),
    "nqa_md_num_partials": (c_int64, [c_int64]),
    "nqa_md_step": (
        c_int32, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_void_p]),
    "nqa_md_bath": (c_int32, [c_void_p, c_int64, c_void_p, c_int32, c_void_p]),
    "nqa_md_langevin_step": (
        c_int32, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int32,
                  c_void_p]),
    "nqa_md_noise": (c_int32, [c_uint64, c_uint64, c_int64, c_void_p, c_void_p, c_void_p]),
    "nqa_md_npt_bath": (
        c_int32, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "nqa_md_npt_scale": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "nqa_md_batched_langevin_step": (
        c_int32, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                  c_int32, c_void_p]),
    "nqa_md_batched_bath": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    "nqa_md_batched_npt_bath": (
        c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_void_p]),
    "nqa_md_batched_npt_scale": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "nqa_fire_chunk_atoms": (c_int32, []),
    "nqa_fire_reduce": (c_int32, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "nqa_fire_decide": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "nqa_fire_move": (c_int32, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "nqa_cellfire_reduce": (c_int32, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "nqa_cellfire_decide": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "nqa_cellfire_move": (c_int32, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                    c_void_p]),
}

# nqa_tp_scatter_<family>_paired: the family's arguments with (weight_rows, num_pairs) before the stream
for _family in ("fwd", "bwd_edge", "bwd_fused", "bwd_x"):
    _res, _args = SIGNATURES[f"nqa_tp_scatter_{_family}"]
    SIGNATURES[f"nqa_tp_scatter_{_family}_paired"] = (_res, _args[:-1] + [c_void_p, c_int64, c_void_p])

_lock = threading.Lock()
_lib = None


class NequipAmdLibraryError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load (once) and return the shared library; raise loudly if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise NequipAmdLibraryError(
                f"{LIB_PATH} not found: the HIP kernels have not been built. Run "
                "`python -m nequip_amd.csrc.build` (or `__graft_entry__.build()`); there is no CPU fallback."
            )
        lib = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as exc:  # pragma: no cover
                raise NequipAmdLibraryError(f"{LIB_PATH} does not export `{name}`") from exc
            fn.restype = restype
            fn.argtypes = argtypes
        if lib.nqa_abi_version() != 1:
            raise NequipAmdLibraryError("libnequip_amd.so ABI version mismatch; rebuild the library")
        _lib = lib
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != NQA_OK:
        msg = load().nqa_last_error()
        raise RuntimeError(f"libnequip_amd {what} failed (code {rc}): {msg.decode() if msg else ''}")


def ptr(t):
    """Device address of a tensor as a ``void*`` argument; null for ``None``."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p()


def stream_ptr(device):
    """The current stream of ``device`` as an ``nqa_stream`` argument."""
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def int32_array(values):
    arr = (c_int32 * max(len(values), 1))()
    for i, v in enumerate(values):
        arr[i] = int(v)
    return arr
