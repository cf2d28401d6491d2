"""livevisionkit_amd -- MI355X-native implementation of LiveVisionKit's video stabilization hot path.

The product is liblvk_hip.so (hand-written HIP kernels for gfx950 behind the C-ABI of include/lvk_hip.h) plus
the C++ facade in include/lvk/.  This Python package is the thin host-side mirror used by the tests and the
bench driver: it calls the C-ABI through ctypes and uses torch only for device memory and streams.
"""
from . import _native
from .context import Context, LvkHipError, REMAP_EXACT, REMAP_1LSB
from .stabilization import StabilizationFilter, StabilizationFilterSettings
from .deblocking import DeblockingFilter, DeblockingFilterSettings
from .cas import CASFilter
from .convert import ConversionFilter, reformat
from .fsr import FSRFilter, fsr_geometry, easu_const
from .draw import draw_points, draw_rect, draw_text, text_size
from .lens import LCFilter
from . import shard

__all__ = ["Context", "LvkHipError", "REMAP_EXACT", "REMAP_1LSB", "StabilizationFilter", "StabilizationFilterSettings", "DeblockingFilter", "DeblockingFilterSettings", "CASFilter",
           "ConversionFilter", "reformat", "FSRFilter", "fsr_geometry", "easu_const", "LCFilter", "draw_points", "draw_rect",
           "draw_text", "text_size", "_native"]
