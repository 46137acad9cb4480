from .acor import integrated_time, AutocorrError
from .resample import SystematicResampler

__all__ = ['SystematicResampler', 'integrated_time', 'AutocorrError']
