from . import AtomicDataDict  # noqa: F401
from ._key_registry import register_fields  # noqa: F401
from .modifier import BaseModifier, MappedFieldModifier, PerAtomModifier  # noqa: F401
