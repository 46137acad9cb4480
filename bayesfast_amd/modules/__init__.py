from .poly import PolyConfig, PolyModel
from .fit_report import FitReport, RidgeReport

__all__ = ['PolyConfig', 'PolyModel', 'FitReport', 'RidgeReport']
