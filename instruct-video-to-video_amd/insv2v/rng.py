"""Stream ids of the seeded noise (include/insv2v_hip.h, section "seeded noise").

The generator lives in the HIP kernels (csrc/rng.h): a value is a pure function of (seed, stream id, element index).  This module only
packs the stream id - integers, no generator of its own.  Layout of the 54-bit id (the header documents the same):

    bits 52-53  kind    ENC = 0, INIT = 1, STEP = 2, MASK = 3
    bits 28-51  unit    < 2^24   the (video, prompt) unit, numbered globally by the driver
    bits 16-27  window  < 2^12   the window of the long-video plan (run_loveu_tgve.split_batch)
    bits  0-15  step    < 2^16   the sampling step inside the window (MASK: the draw)

  ENC   element index over the whole video's posterior noise [T,4,h,w]                 (window = step = 0)
  INIT  element index over the NEW frames [n,4,h,w] of window k                        (step = 0)
  STEP  element index over the clip's [F,4,h,w] at window k, sampling step i
  MASK  element index over the chunk's [F,4,h,w] of the mask estimate (inference.estimate_mask): window = chunk index, step = draw index
"""
import operator

ENC, INIT, STEP = 0, 1, 2


class _Kind(int):
    """A kind that is passed by NAME only.  ``stream_id`` has always refused the bare integer 3; it still does, so nothing that was an
    error before MASK existed became a valid stream: ``MASK == 3`` (the value of the 2-bit field), but only the object itself is taken."""
    __slots__ = ()


MASK = _Kind(3)
UNIT_BITS, WINDOW_BITS, STEP_BITS = 24, 12, 16


def stream_id(kind, unit, window=0, step=0):
    """The int64 stream id of one purpose; injective over the documented ranges, ValueError outside them."""
    if kind is not MASK and kind not in (ENC, INIT, STEP):
        raise ValueError(f"stream_id: kind must be ENC, INIT, STEP or MASK, got {kind!r}")
    for name, v, bits in (("unit", unit, UNIT_BITS), ("window", window, WINDOW_BITS), ("step", step, STEP_BITS)):
        v = _index(v, name)
        if not 0 <= v < (1 << bits):
            raise ValueError(f"stream_id: {name} = {v} outside [0, 2^{bits})")
    return (int(kind) << (UNIT_BITS + WINDOW_BITS + STEP_BITS)) | (int(unit) << (WINDOW_BITS + STEP_BITS)) | (int(window) << STEP_BITS) | int(step)


def _index(v, name):
    try:
        return operator.index(v)
    except TypeError:
        raise ValueError(f"{name} must be an integer, got {type(v).__name__}") from None


def as_int64(v, name="seed"):
    """A Python int as the int64 the C ABI takes: [-2^63, 2^64) is accepted and taken as its 64 two's-complement bits."""
    v = _index(v, name)
    if not -(1 << 63) <= v < (1 << 64):
        raise ValueError(f"{name} = {v} does not fit 64 bits")
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v
