"""Which fields hold one value per frame (mirror of the graph-field part of ``nequip/data/_key_registry.py:24-36,75-145``).

``NodeTypeEmbed`` accepts only these as categorical graph fields, and ``AtomicDataDict.batched_from_list`` concatenates
them one row per frame.  ``register_fields(graph_fields=...)`` adds custom ones (the long / Cartesian-tensor
registries of the reference have no counterpart here).  The per-edge registry (``edge_fields``) names the fields that hold one
row per edge: what ``NeighborListPruneTransform`` masks together with ``edge_index``.  The per-node registry
(``node_fields``) names the fields with one row per atom: ``MetricsManager`` accepts ``per_type`` only for these
(``get_field_type``), and ``ABBREV`` gives the short names of its automatic metric names.
"""

from typing import Dict, Optional, Sequence, Set

from . import _keys

_DEFAULT_GRAPH_FIELDS: Set[str] = {
    _keys.TOTAL_ENERGY_KEY,
    "free_energy",
    _keys.STRESS_KEY,
    _keys.VIRIAL_KEY,
    _keys.PBC_KEY,
    _keys.CELL_KEY,
    _keys.NUM_NODES_KEY,
    _keys.DATASET_KEY,
    _keys.TOTAL_CHARGE_KEY,
    _keys.TOTAL_SPIN_KEY,
    "magmom",
    "polarization",
    "dielectric_tensor",
}
_GRAPH_FIELDS: Set[str] = set(_DEFAULT_GRAPH_FIELDS)

# one row per edge (``edge_index`` itself is [2, E] and handled on its own)
_DEFAULT_EDGE_FIELDS: Set[str] = {
    _keys.EDGE_CELL_SHIFT_KEY,
    _keys.EDGE_VECTORS_KEY,
    _keys.EDGE_LENGTH_KEY,
    _keys.NORM_LENGTH_KEY,
    _keys.EDGE_ATTRS_KEY,
    _keys.EDGE_EMBEDDING_KEY,
    "edge_features",
    _keys.EDGE_CUTOFF_KEY,
    "edge_energy",
    _keys.EDGE_FORCE_KEY,
}
_EDGE_FIELDS: Set[str] = set(_DEFAULT_EDGE_FIELDS)


# one row per atom (``nequip/data/_key_registry.py:39-54``)
_DEFAULT_NODE_FIELDS: Set[str] = {
    _keys.POSITIONS_KEY,
    _keys.NODE_FEATURES_KEY,
    _keys.NODE_ATTRS_KEY,
    "atomic_numbers",
    _keys.ATOM_TYPE_KEY,
    _keys.PER_ATOM_ENERGY_KEY,
    "charges",
    _keys.FORCE_KEY,
    "stresses",
    "magmoms",
    "dipole",
    "born_effective_charges",
    _keys.BATCH_KEY,
    _keys.FEATURE_NORM_FACTOR_KEY,
}
_NODE_FIELDS: Set[str] = set(_DEFAULT_NODE_FIELDS)

# short names for automatic metric names (``nequip/data/_key_registry.py:253-262``)
ABBREV: Dict[str, str] = {
    _keys.TOTAL_ENERGY_KEY: "E",
    _keys.PER_ATOM_ENERGY_KEY: "Ei",
    _keys.FORCE_KEY: "F",
    "magmom": "M",
    "charges": "Q",
    "polarization": "pol",
    "born_effective_charges": "Z*",
    "dielectric_tensor": "\u03b5",
}


def get_field_type(field: str, error_on_unregistered: bool = True) -> Optional[str]:
    """``"graph"``, ``"node"`` or ``"edge"``; an unregistered field raises ``KeyError`` (or gives ``None``)."""
    if field in _GRAPH_FIELDS:
        return "graph"
    if field in _NODE_FIELDS:
        return "node"
    if field in _EDGE_FIELDS:
        return "edge"
    if error_on_unregistered:
        raise KeyError(f"Unregistered field {field} found")
    return None


def register_fields(graph_fields: Optional[Sequence[str]] = None, edge_fields: Optional[Sequence[str]] = None,
                    node_fields: Optional[Sequence[str]] = None) -> None:
    """Register custom fields as per-frame (``graph_fields``), per-edge (``edge_fields``) or per-atom (``node_fields``)."""
    graph_fields = [] if graph_fields is None else graph_fields
    edge_fields = [] if edge_fields is None else edge_fields
    node_fields = [] if node_fields is None else node_fields
    assert not isinstance(node_fields, str), (
        "node_fields must be a sequence of strings, each representing a field name, rather than a single string")
    assert not set(node_fields) & (set(graph_fields) | set(edge_fields) | _GRAPH_FIELDS | _EDGE_FIELDS) and not (
        set(graph_fields) | set(edge_fields)) & _NODE_FIELDS, "a per-atom field cannot also be per-frame or per-edge"
    assert not isinstance(graph_fields, str), (
        "graph_fields must be a sequence of strings, each representing a field name, rather than a single string")
    assert not isinstance(edge_fields, str), (
        "edge_fields must be a sequence of strings, each representing a field name, rather than a single string")
    assert not set(graph_fields) & (set(edge_fields) | _EDGE_FIELDS) and not set(edge_fields) & _GRAPH_FIELDS, (
        "a field cannot be both per-frame and per-edge")
    _GRAPH_FIELDS.update(graph_fields)
    _EDGE_FIELDS.update(edge_fields)
    _NODE_FIELDS.update(node_fields)
