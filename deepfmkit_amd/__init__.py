"""deepfmkit_amd — MI355X-native DFMI per-segment NLS readout engine.

Drop-in for the hot path of mdovale/DeepFMKit: `DeepFitFramework.fit()` with the
'nls' and 'ekf' strategies, the fit.* module constants, and the workers entry
points. All arithmetic of the path runs in hand-written HIP kernels for gfx950
(libdfmi.so, C ABI in include/dfmi.h); there is no CPU fallback.
"""
from . import fit  # noqa: F401
from . import helpers  # noqa: F401
from .core import DeepFitFramework, vectorized_downsample  # noqa: F401
from .data import DeepFitObject, DeepRawObject  # noqa: F401
from .fitters import BaseFitter, EKFFitter, StandardNLSFitter  # noqa: F401
from .physics import (DFMIObject, InterferometerConfig, LaserConfig, SignalGenerator,  # noqa: F401
                      set_laser_df_for_effect)
from .helpers import (calculate_crlb_for_m, calculate_jacobian, calculate_m_precision,  # noqa: F401
                      snr_to_asd)

__version__ = "0.1.0"
