from .poly import PolyConfig, PolyModel
from .fit_report import FitReport

__all__ = ['PolyConfig', 'PolyModel', 'FitReport']
