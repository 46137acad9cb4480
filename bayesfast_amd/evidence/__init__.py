from .bridge import bridge
from .importance import importance
from .harmonic import harmonic
from .gbs import GBS
from .gaussianized_q import GIS, GHM
from ..utils.psis import psis

__all__ = ['bridge', 'importance', 'harmonic', 'GBS', 'GIS', 'GHM', 'psis']
