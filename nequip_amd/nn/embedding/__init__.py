from ._edge import (EdgeLengthNormalizer, BesselEdgeLengthEncoding, SphericalHarmonicEdgeAttrs,  # noqa: F401
                    cutoff_partialdict_to_tensor, cutoff_str_to_fulldict, cutoff_tensor_to_str)
from .cutoffs import PolynomialCutoff  # noqa: F401
from .node import NodeTypeEmbed  # noqa: F401
