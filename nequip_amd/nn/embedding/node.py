"""Node type embedding with optional categorical graph-field embeddings (mirror of ``nequip/nn/embedding/node.py:16-175``).

Each categorical graph field (total charge, spin, dataset index, ...: one integer per frame) has its own
``torch.nn.Embedding``; its rows are concatenated onto the type embedding, ``node_attrs[z] = cat(type_row, field_rows...)``.
The self-connections downstream contract their weights per row of a small table instead of per atom
(``o3.modules.FullyConnectedTensorProduct``), so besides ``node_attrs`` this module publishes what those tables are:

* one frame (every field holds one value): every atom shares the field rows, so ``node_attrs == table_eff[atom_types]``
  with ``table_eff[t] = cat(type_table[t], field rows)`` -- published as ``_nqa_node_attrs_table``, and the typed / fused
  node kernels run exactly as for a model without fields;
* a batch of frames: ``_nqa_node_attrs_table`` is the type table (the leading columns of ``node_attrs``) and
  ``_nqa_node_attrs_classes`` lists ``(per-atom row index, field table, first column)`` per field -- the self-connection is
  linear in ``node_attrs``, so it is the sum of one typed map per table (``forward_classes``).
"""

from dataclasses import dataclass
from math import sqrt
from typing import Any, Dict, List, Optional

import torch

from ...data import AtomicDataDict
from ...data._key_registry import _GRAPH_FIELDS
from ...o3.irreps import Irreps
from ...utils.wgrad import differentiable_parameters
from .._graph_mixin import GraphModuleMixin


def _tracing() -> bool:
    from ...utils.tracing import traceable

    return traceable()


def _capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


@dataclass(frozen=True)
class CategoricalGraphFieldEmbedSpec:
    field: str
    num_features: int
    min: int
    max: int
    init: Optional[str] = None

    @classmethod
    def from_dict(cls, field_embed: Dict[str, Any]) -> "CategoricalGraphFieldEmbedSpec":
        required_keys: List[str] = ["field", "num_features", "min", "max"]
        missing_keys = [key for key in required_keys if key not in field_embed]
        assert len(missing_keys) == 0, (
            f"missing keys {missing_keys} in `categorical_graph_field_embed` entry; required keys are {required_keys}."
        )
        return cls(field=str(field_embed["field"]), num_features=int(field_embed["num_features"]),
                   min=int(field_embed["min"]), max=int(field_embed["max"]), init=field_embed.get("init", None))


class NodeTypeEmbed(GraphModuleMixin, torch.nn.Module):
    # (class-level defaults: modules pickled before the field embeddings existed load as field-free)
    do_categorical_graph_field_embed: bool = False
    type_embed_init: Optional[str] = None

    def __init__(self, type_names: List[str], num_features: int, type_embed_init: Optional[str] = None,
                 set_features: bool = True, categorical_graph_field_embed: Optional[List[Dict[str, Any]]] = None,
                 irreps_in=None):
        super().__init__()
        irreps_in = {} if irreps_in is None else dict(irreps_in)
        self.num_types = len(type_names)
        self.set_features = set_features
        self.type_embed_init = type_embed_init
        self.embed_module = torch.nn.Embedding(num_embeddings=self.num_types, embedding_dim=num_features)
        self._init_embedding(self.embed_module, init=type_embed_init)

        # categorical graph fields: module / state-dict names and the order of construction (RNG draws) of the reference
        total_features = num_features
        self.categorical_graph_field_embed_modules = torch.nn.ModuleDict()
        self.categorical_graph_field_embed_shifts: Dict[str, int] = {}
        self.do_categorical_graph_field_embed = False
        if categorical_graph_field_embed is not None:
            self.do_categorical_graph_field_embed = True
            for field_embed_dict in categorical_graph_field_embed:
                field_embed = CategoricalGraphFieldEmbedSpec.from_dict(field_embed_dict)
                assert field_embed.field in _GRAPH_FIELDS, (
                    f"`{field_embed.field}` is not a graph field, only graph fields should be provided to "
                    f"`categorical_graph_field_embed`."
                )
                assert field_embed.max >= field_embed.min, f"`max` must be >= `min` for field `{field_embed.field}`."
                embed_module = torch.nn.Embedding(num_embeddings=field_embed.max - field_embed.min + 1,
                                                  embedding_dim=field_embed.num_features)
                self._init_embedding(embed_module, init=field_embed.init)
                self.categorical_graph_field_embed_modules.update({field_embed.field: embed_module})
                self.categorical_graph_field_embed_shifts.update({field_embed.field: field_embed.min})
                total_features += field_embed.num_features
                if field_embed.field not in irreps_in:
                    irreps_in[field_embed.field] = None  # (categorical: no irreps; makes GraphModel pass the field in)

        irreps_out = {AtomicDataDict.NODE_ATTRS_KEY: Irreps([(total_features, (0, 1))])}
        if set_features:
            irreps_out[AtomicDataDict.NODE_FEATURES_KEY] = irreps_out[AtomicDataDict.NODE_ATTRS_KEY]
        self._init_irreps(irreps_in=irreps_in, irreps_out=irreps_out)

    @staticmethod
    def _init_embedding(module: torch.nn.Embedding, init: Optional[str]) -> None:
        if init is None:
            return
        if init == "uniform":
            torch.nn.init.uniform_(module.weight, -sqrt(3.0), sqrt(3.0))
        elif init == "zero":
            torch.nn.init.zeros_(module.weight)
        elif init == "near_zero":
            torch.nn.init.normal_(module.weight, mean=0.0, std=1e-5)
        else:
            raise ValueError(f"unsupported embedding init mode `{init}`. supported modes: ('uniform', 'zero', 'near_zero') "
                             f"or None")

    def _lookup(self, idx: torch.Tensor, table: torch.Tensor, n: int) -> torch.Tensor:
        if table.requires_grad:
            # training: one-hot product instead of a row gather -- same values (each row is 1.0 x one table row plus exact
            # zeros); its backward is a [T, N] x [N, F] product instead of embedding_dense_backward's sort + segmented
            # reduction (127 -> ~15 us per step at 8192 atoms / 5 types), and it is differentiable again as is
            # (not F.one_hot: its range check of the indices synchronises with the device)
            kinds = torch.arange(n, device=idx.device).view(1, -1)
            return (idx.view(-1, 1) == kinds).to(table.dtype) @ table
        return torch.nn.functional.embedding(idx, table)

    def forward(self, data: AtomicDataDict.Type) -> AtomicDataDict.Type:
        atom_types = data[AtomicDataDict.ATOM_TYPE_KEY].view(-1)
        # Out-of-range types: `F.embedding` (eval path; the reference's only path) raises / faults on them, the one-hot
        # product of the training path below would silently give a zero row.  Host tensors are checked here (free);
        # device tensors are not (the check would synchronise every step) -- validate type maps where the data is built.
        if not atom_types.is_cuda and atom_types.numel() > 0 and not _tracing():
            lo, hi = int(atom_types.min()), int(atom_types.max())
            if lo < 0 or hi >= self.num_types:
                raise IndexError(f"atom type index out of range: [{lo}, {hi}] for {self.num_types} types")
        # eval mode: parameters are constants (same convention as o3.Linear) -- keeps autograd from carrying the
        # position-independent embedding through every backward kernel when only forces are requested
        w = self.embed_module.weight
        table = w if differentiable_parameters(self.training, w) else w.detach()
        classes = None
        if self.do_categorical_graph_field_embed:
            table, classes = self._field_tables(data, table, atom_types.shape[0])
        embedding = self._lookup(atom_types, table, table.shape[0])
        if classes is not None:
            embedding = torch.cat([embedding] + [self._lookup(idx, tb, tb.shape[0]) for idx, tb, _ in classes], dim=1)
            data["_nqa_node_attrs_classes"] = classes
        data[AtomicDataDict.NODE_ATTRS_KEY] = embedding
        # node_attrs == table[types] (+ the class rows of a batch): lets the self-connection contract its weights per
        # table row first
        data["_nqa_node_attrs_table"] = table
        if self.set_features:
            data[AtomicDataDict.NODE_FEATURES_KEY] = embedding
        return data

    # ---- categorical graph fields --------------------------------------------------------------------------------------
    def _field_values(self, data: AtomicDataDict.Type):
        """Per field its flat value tensor, after the checks of the reference (present, integer) and a range check that
        keeps any value outside ``[min, max]`` from ever reaching a kernel as a row index.  The check reads all fields in
        one small host copy (one number per frame).  While a tracer follows the model or a graph is captured there is no
        host read (``host`` is None): the row indices are then clamped on the device instead -- valid memory, never a
        fault -- so a graphed step must be fed validated labels."""
        vals = []
        for field in self.categorical_graph_field_embed_modules.keys():
            if field not in data:
                raise KeyError(f"categorical_graph_field_embed: field `{field}` is missing from the input data")
            v = data[field].reshape(-1)
            if v.is_floating_point() or v.is_complex() or v.dtype == torch.bool:
                raise TypeError(f"categorical_graph_field_embed: field `{field}` must hold integers, got {v.dtype}")
            vals.append(v)
        host = None
        if not _tracing() and (not _capturing() or not any(v.is_cuda for v in vals)):  # (host values: no device read)
            flat = [v.to(torch.int64) for v in vals]
            host = (torch.cat(flat) if len(flat) > 1 else flat[0]).cpu().tolist()
            off = 0
            for (field, module), v in zip(self.categorical_graph_field_embed_modules.items(), vals):
                lo = self.categorical_graph_field_embed_shifts[field]
                hi = lo + module.num_embeddings - 1
                bad = [k for k in host[off : off + v.numel()] if k < lo or k > hi]
                if bad:
                    raise IndexError(f"categorical_graph_field_embed: `{field}` value {bad[0]} outside [{lo}, {hi}]")
                off += v.numel()
        return vals, host

    def _field_tables(self, data: AtomicDataDict.Type, type_table: torch.Tensor, num_atoms: int):
        vals, host = self._field_values(data)
        tables = []
        for module in self.categorical_graph_field_embed_modules.values():
            w = module.weight
            tables.append(w if differentiable_parameters(self.training, w) else w.detach())
        nf = data.get(AtomicDataDict.NUM_NODES_KEY)
        if all(v.numel() == 1 for v in vals) and (nf is None or nf.numel() <= 1):
            return self._frame_table(type_table, tables, vals, host), None
        # a batch: per-atom row index of every field, through the frame index of each atom
        batch = data.get(AtomicDataDict.BATCH_KEY)
        if batch is None:
            raise ValueError("categorical_graph_field_embed: fields with one value per frame of a batch need "
                             f"`{AtomicDataDict.BATCH_KEY}`")
        batch = batch.view(-1)
        if host is not None:
            frames = nf.numel() if nf is not None else int(batch.max()) + 1
            for field, v in zip(self.categorical_graph_field_embed_modules.keys(), vals):
                if v.numel() != frames:
                    raise ValueError(f"categorical_graph_field_embed: `{field}` holds {v.numel()} values for {frames} "
                                     f"frames")
        classes = []
        col = type_table.shape[1]
        for (field, shift), v, tb in zip(self.categorical_graph_field_embed_shifts.items(), vals, tables):
            idx = torch.index_select(v.to(device=batch.device, dtype=torch.int64), 0, batch) - shift
            if host is None:
                idx = idx.clamp(0, tb.shape[0] - 1)
            classes.append((idx, tb, col))
            col += tb.shape[1]
        return type_table, classes

    def _frame_table(self, type_table, tables, vals, host):
        """``[T, F_total]``: every type row followed by the rows of this frame's field values (one gather + one cat on the
        device, from the validated host values; cached across calls while nothing it depends on changes)."""
        T = type_table.shape[0]
        if host is None:  # (tracing / capture: graph operations on the device values)
            rows = [tb.index_select(0, (v.to(device=tb.device, dtype=torch.int64) - s).clamp(0, tb.shape[0] - 1))
                    for tb, v, s in zip(tables, vals, self.categorical_graph_field_embed_shifts.values())]
            return torch.cat([type_table] + [r.expand(T, -1) for r in rows], dim=1)
        ks = [k - s for k, s in zip(host, self.categorical_graph_field_embed_shifts.values())]
        grad = type_table.requires_grad or any(tb.requires_grad for tb in tables)
        key = None
        if not grad:
            key = tuple(ks) + tuple((t.data_ptr(), t._version, t.dtype, str(t.device)) for t in [type_table] + tables)
            hit = self.__dict__.get("_frame_table_cache")
            if hit is not None and hit[0] == key:
                return hit[1]
        out = torch.cat([type_table] + [tb[k : k + 1].expand(T, -1) for tb, k in zip(tables, ks)], dim=1)
        if key is not None:
            self.__dict__["_frame_table_cache"] = (key, out)
        return out


def categorical_graph_fields(model: torch.nn.Module) -> List[str]:
    """The categorical graph fields (``categorical_graph_field_embed``) that any type embedding inside ``model`` reads."""
    out: List[str] = []
    for mod in model.modules():
        if getattr(mod, "do_categorical_graph_field_embed", False):
            out += [f for f in mod.categorical_graph_field_embed_modules.keys() if f not in out]
    return out


def refuse_categorical_graph_fields(model: torch.nn.Module, what: str) -> None:
    """Integrations that build the model's input themselves and have no way to carry a per-frame label refuse up front."""
    fields = categorical_graph_fields(model)
    if fields:
        raise NotImplementedError(f"{what} does not support models built with `categorical_graph_field_embed` (fields "
                                  f"{fields}): evaluate the model eagerly with the fields set in the input data")
