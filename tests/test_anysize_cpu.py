"""Host logic of the any-frame-size path (no GPU): the size plan of a latent through the UNet against the sizes the unmodified
reference's tensors had (tests/golden/unet_tiny_anysize.npz, written by tools/gen_golden_anysize.py), the stacking limit at a ragged
size, the refusal of a degenerate latent, and the dispatch predicates that are plain Python."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_plan_sizes_match_the_reference():
    from insv2v.unet import plan_sizes
    table = np.load(os.path.join(GOLDEN, "unet_tiny_anysize.npz"))["size_table"]
    assert {(45, 80), (60, 106), (20, 14)} <= {(int(r[0]), int(r[1])) for r in table}
    for row in table.tolist():
        H, W = row[:2]
        plan = plan_sizes(H, W, 4)
        assert plan["down"] == [tuple(row[2 + 2 * i:4 + 2 * i]) for i in range(4)], (H, W)
        assert plan["up"] == [tuple(row[10 + 2 * i:12 + 2 * i]) for i in range(3)], (H, W)
        for (h, w), (th, tw) in zip(plan["down"][:0:-1], plan["up"]):   # every target is the x2 image or that image less one row / column
            assert th in (2 * h - 1, 2 * h) and tw in (2 * w - 1, 2 * w)
    assert plan_sizes(45, 80)["down"] == [(45, 80), (23, 40), (12, 20), (6, 10)] and plan_sizes(45, 80)["up"] == [(12, 20), (23, 40), (45, 80)]


@pytest.mark.parametrize("H,W", [(0, 8), (8, 0), (-1, 4)])
def test_degenerate_latent_is_refused(H, W):
    from insv2v.unet import plan_sizes
    with pytest.raises(ValueError, match="reaches 0"):
        plan_sizes(H, W)


def test_max_clips_in_flight_at_a_ragged_size():
    """16 frames at latent 45x80 (a 360x640 video): a [3 n * 16 * 3600, 640] fp16 tensor must fit one 2 GiB descriptor - 221 184 000 bytes
    per clip, so 9 clips (1.99 GB); 10 would need 2.21 GB."""
    from insv2v.inference import max_clips_in_flight
    assert max_clips_in_flight(16, 45, 80) == 9
    assert 3 * 9 * 16 * 45 * 80 * 640 * 2 < 2 ** 31 - 2 ** 20 < 3 * 10 * 16 * 45 * 80 * 640 * 2
    assert max_clips_in_flight(16, 32, 48) == 20   # the bench's size keeps its cap


def test_winograd_and_conv_geometry_rules():
    from insv2v import ops
    for hw in ((5, 7), (23, 40), (12, 21), (45, 80)):   # odd sizes take the Winograd form (ceil(H/2) x ceil(W/2) tiles)
        assert ops.winograd_ok((4, *hw), 1280) and ops.winograd_ok((4, *hw), 2560, 1280)
    assert not ops.winograd_ok((4, 23, 130), 1280) and not ops.winograd_ok((4, 23, 40), 1300)
    # the upsample form is exact x2 only: a cropped target takes the direct convolution
    assert ops.winograd_ok((4, 12, 20), 1280, upsample=True) and ops.winograd_ok((4, 12, 20), 1280, upsample=True, out_size=(24, 40))
    for size in ((23, 40), (24, 39), (23, 39)):
        assert not ops.winograd_ok((4, 12, 20), 1280, upsample=True, out_size=size)
    assert ops._conv_geometry((2, 12, 20), 1, (1, 1), True) == (24, 40)
    assert ops._conv_geometry((2, 12, 20), 1, (1, 1), True, (23, 40)) == (23, 40)
    assert ops._conv_geometry((2, 45, 80), 2, (1, 1), False) == (23, 40)
    with pytest.raises(ValueError):
        ops._conv_geometry((2, 12, 20), 1, (1, 1), False, (12, 20))
