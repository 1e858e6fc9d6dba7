"""Growing, shrinking and feathering the mask of a localized edit: the host side of ``ops.mask_shape``.

A mask from any source - drawn, ``mask="auto"``, ``mask_key=`` - serves two jobs that want different masks.  The latent hold wants a
generous HARD region, so that the model is free in the whole transition zone; the pixel composite wants a SOFT edge inside that region.
``shape_mask`` returns both: ``shaped`` (grown by ``grow`` pixels, then feathered over ``feather`` pixels OUTSIDE the grown edge) and
``support`` (1 wherever ``shaped`` > 0).  All defaults are starting values, untuned: the project has no checkpoint to tune them on.
"""
import math

from . import ops
from ._lib import MASK_PROFILES, MASK_SHAPE_MAX

MASK_SHAPE_KEYS = ("grow", "feather", "threshold", "profile")


def check_shape_args(grow=0.0, feather=0.0, threshold=0.5, profile="smooth"):
    """Host-side check of the shaping parameters (nothing is launched): ``grow`` in [-32, 32] pixels (negative shrinks), ``feather`` in
    [0, 32] pixels with ``grow + feather`` >= -32, a finite ``threshold`` (a pixel is inside where mask > threshold), ``profile``
    "linear" or "smooth"."""
    def real(v, name):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{name} {v!r} is not a finite number")
        return float(v)
    g, f = real(grow, "grow"), real(feather, "feather")
    real(threshold, "threshold")
    if not -MASK_SHAPE_MAX <= g <= MASK_SHAPE_MAX:
        raise ValueError(f"grow {grow!r} is outside [-{MASK_SHAPE_MAX}, {MASK_SHAPE_MAX}] pixels")
    if not 0 <= f <= MASK_SHAPE_MAX:
        raise ValueError(f"feather {feather!r} is outside [0, {MASK_SHAPE_MAX}] pixels")
    if g + f < -MASK_SHAPE_MAX:
        raise ValueError(f"grow + feather = {g + f!r} is below -{MASK_SHAPE_MAX} pixels")
    if profile not in MASK_PROFILES:
        raise ValueError(f"profile {profile!r} is neither 'linear' nor 'smooth'")


def check_mask_shape(mask_shape):
    """``mask_shape`` of ``edit_video``: a dict with keys among ``MASK_SHAPE_KEYS`` whose values pass ``check_shape_args``."""
    if not isinstance(mask_shape, dict) or set(mask_shape) - set(MASK_SHAPE_KEYS):
        raise ValueError(f"mask_shape (the shaping of an edit's mask) must be a dict with keys among {MASK_SHAPE_KEYS}, got {mask_shape!r}")
    try:
        check_shape_args(**mask_shape)
    except ValueError as e:
        raise ValueError(f"mask_shape (the shaping of an edit's mask): {e}") from None


def shape_mask(mask, **params):
    """mask fp32 [1,T,H,W] or [T,H,W] on the GPU -> (shaped, support) of the same shape: one ``ops.mask_shape`` call."""
    check_shape_args(**params)
    m = mask.reshape(-1, *mask.shape[-2:]).contiguous()
    shaped, support = ops.mask_shape(m, **params)
    return shaped.reshape(mask.shape), support.reshape(mask.shape)
