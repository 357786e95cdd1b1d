"""MI355X-native Restormer / MoCE-IR transformer block (hand-written gfx950 HIP kernels behind a C-ABI).

Drop-in modules with the reference's class names, constructor arguments, parameter names and
``forward`` signatures live in :mod:`image_restoration_amd.restormer`; the kernels are reached
through ``libmi_restore.so`` (``include/mi_restore.h``).  There is no CPU fallback: calling a module
on a CPU tensor, or without the built library, raises.
"""
from . import _lib  # noqa: F401
from .darkir import DarkIR, DBlock, EBlock, FreMLP  # noqa: F401
from .ops import reload_env  # noqa: F401
from .restormer import (Attention, Downsample, FeedForward, LayerNorm, OverlapPatchEmbed, Restormer,  # noqa: F401
                        TransformerBlock, Upsample)
from .sfhformer import (FFN, BatchNorm2d, FourierUnit, Mixer, SFHformer_l, SFHformer_m, SFHformer_s, SFHformer_t,  # noqa: F401
                        TokenMixer_For_Gloal, TokenMixer_For_Local, scaled_residual)

__all__ = ["Attention", "BatchNorm2d", "DarkIR", "DBlock", "Downsample", "EBlock", "FFN", "FeedForward", "FourierUnit", "FreMLP", "LayerNorm", "Mixer", "OverlapPatchEmbed", "Restormer",
           "SFHformer_l", "SFHformer_m", "SFHformer_s", "SFHformer_t", "TokenMixer_For_Gloal", "TokenMixer_For_Local", "TransformerBlock",
           "Upsample", "reload_env", "scaled_residual"]
