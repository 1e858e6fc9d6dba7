"""Host side of the segmented row schedule of the text cross-attention kernels (units of 128 rows per sample) and of the GroupNorm
fold of insv2v_rowlin (units of 32 rows per (sample, frame) group): fused.row_units states what the launchers implement, and the
*_supported predicates accept every rows_per_sample."""
import os
import sys

import pytest

from conftest import PKG


def _brute(M, seg_rows, unit):
    """Walk the rows segment by segment, opening a new unit every `unit` rows of a segment: [(segment, [rows])]."""
    units = []
    for s in range(M // seg_rows):
        rows = list(range(s * seg_rows, (s + 1) * seg_rows))
        for u0 in range(0, seg_rows, unit):
            units.append((s, rows[u0:u0 + unit]))
    return units


@pytest.mark.parametrize("unit", [32, 128])
def test_row_units_against_brute_force(unit):
    from insv2v.fused import row_units, unit_rows
    for seg_rows in range(1, 301):
        for segments in (1, 3):
            M = segments * seg_rows
            ups, n = row_units(M, seg_rows, unit)
            want = _brute(M, seg_rows, unit)
            assert ups == -(-seg_rows // unit) and n == segments * ups == len(want), (seg_rows, segments)
            seen = []
            for q in range(n):
                s, row0, valid = unit_rows(q, seg_rows, unit)
                rows = list(range(row0, row0 + valid))
                assert (s, rows) == want[q], (seg_rows, segments, q)
                assert 1 <= valid <= unit
                assert all(r // seg_rows == s for r in rows), "a unit holds rows of two segments"
                seen += rows
            assert seen == list(range(M)), "every real row exactly once"
            if seg_rows % unit == 0:   # aligned: the plain tiling of the M rows
                assert n == M // unit
                assert all(unit_rows(q, seg_rows, unit)[1:] == (q * unit, unit) for q in range(n))


def test_row_units_rejects_partial_segments():
    from insv2v.fused import row_units
    with pytest.raises(ValueError):
        row_units(100, 33, 32)
    with pytest.raises(ValueError):
        row_units(0, 32, 32)


def test_xattn_supported_at_ragged_rows():
    """With the library loaded as the ABI-consistency tests load it: the two predicates no longer ask for 128-row samples."""
    from insv2v import _lib, ops
    if not os.path.exists(_lib.LIB_PATH):
        sys.path.insert(0, PKG)
        import build
        build.build(verbose=False)
    _lib.load()
    assert ops.xattn_fused_supported(320, 8, 77, 72)
    assert ops.xattn_attn_supported(640, 8, 77, 320)
    assert ops.xattn_fused_supported(320, 8, 77, 128) and ops.xattn_attn_supported(640, 8, 96, 1)
    # what stays unsupported
    assert not ops.xattn_fused_supported(320, 8, 64, 72) and not ops.xattn_fused_supported(320, 8, 97, 72)
    assert not ops.xattn_attn_supported(640, 8, 64, 320) and not ops.xattn_fused_supported(640, 8, 77, 72)
