"""Which fields hold one value per frame (mirror of the graph-field part of ``nequip/data/_key_registry.py:24-36,75-145``).

``NodeTypeEmbed`` accepts only these as categorical graph fields, and ``AtomicDataDict.batched_from_list`` concatenates
them one row per frame.  ``register_fields(graph_fields=...)`` adds custom ones (the per-node / per-edge / long /
Cartesian-tensor registries of the reference have no counterpart here).
"""

from typing import Optional, Sequence, Set

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


def register_fields(graph_fields: Optional[Sequence[str]] = None) -> None:
    """Register custom fields as per-frame (``graph_fields``)."""
    graph_fields = [] if graph_fields is None else graph_fields
    assert not isinstance(graph_fields, str), (
        "graph_fields must be a sequence of strings, each representing a field name, rather than a single string")
    _GRAPH_FIELDS.update(graph_fields)
