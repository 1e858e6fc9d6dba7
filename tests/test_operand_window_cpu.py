"""Host side of "any stack or frame that fits in memory runs" (DESIGN.md section 12), without a GPU: the up-front check of the row
kernels' operand windows on known geometries, the grouping of run_stacked under a caller's cap, the CLI switch, and the unchanged
default cap."""
import inspect

import pytest

from insv2v.fused import OPERAND_WINDOW, check_operand_windows, row_kernel_extents
from insv2v.inference import InferenceIP2PVideo, max_clips_in_flight, stack_groups
from insv2v.run_loveu_tgve import build_parser, check_args, edit_videos


@pytest.mark.parametrize("clips,F,h,w", [(46, 16, 32, 48), (16, 24, 48, 64), (20, 16, 45, 80)])
def test_stacks_beyond_the_default_cap_are_accepted(clips, F, h, w):
    """C2 x 46, C5 x 16 and 45 x 80 x 20: all beyond max_clips_in_flight, all beyond 2 GiB at level 0 or at C = 640, none with a
    per-base extent anywhere near the window."""
    assert clips > max_clips_in_flight(F, h, w)
    assert 3 * clips * F * h * w * 640 * 2 > OPERAND_WINDOW
    assert check_operand_windows(3 * clips, F, h, w) is None
    worst = max(b for lvl, C in enumerate((320, 640)) for _, _, b in row_kernel_extents(3 * clips, F, (-(-h // 2 ** lvl)) * (-(-w // 2 ** lvl)), C))
    assert worst < OPERAND_WINDOW // 8


def test_a_sample_beyond_the_window_is_refused_and_names_tattn():
    """32 frames at 1920 x 1792 (240 x 224 latents): one sample at C = 640 is 32 x 53 760 x 640 x 2 = 2.2 GB, which the temporal attention
    would have to address from one base.  A UNet whose first level is 640 wide is refused, by name and with the sizes; at the default
    widths that level is 320 wide (1.1 GB) and the level of 640 channels has a quarter of the pixels, so the same frame runs.  At the
    default widths the first frames to be refused are 4K-class: 32 frames at 3840 x 2176."""
    assert 32 * 240 * 224 * 640 * 2 >= OPERAND_WINDOW
    with pytest.raises(ValueError, match="insv2v_tattn_attn") as e:
        check_operand_windows(3, 32, 240, 224, channels=(640, 1280))
    msg = str(e.value)
    assert "32 frames" in msg and "240 x 224" in msg and str(32 * 240 * 224 * 640 * 2) in msg and str(OPERAND_WINDOW) in msg
    assert check_operand_windows(3, 32, 240, 224) is None
    with pytest.raises(ValueError, match="insv2v_tattn_fused"):
        check_operand_windows(3, 32, 480, 272)
    assert check_operand_windows(3, 16, 480, 272) is None       # 16 frames of the same 4K-class frame: 1.34 GB per sample


def test_one_sample_is_the_unit_of_the_attention_kernels():
    """The launchers split at whole samples, so the window bounds ONE sample's frames x pixels x channels - whatever the number of samples,
    odd or even pixel counts, 16 or 32 frame slots - and a 128-row tile for the feed-forward."""
    F, C = 16, 320
    HW = -(-OPERAND_WINDOW // (F * C * 2))        # the first pixel count of a sample that does not fit
    assert F * HW * C * 2 >= OPERAND_WINDOW > F * (HW - 1) * C * 2
    for samples in (1, 3, 300):
        assert check_operand_windows(samples, F, 1, HW - 1, channels=(320,)) is None
        with pytest.raises(ValueError, match="one sample of 16 frames"):
            check_operand_windows(samples, F, 1, HW, channels=(320,))
    ext = dict((e, b) for e, _, b in row_kernel_extents(60, 16, 1536, 320) if "K / V" not in _)
    assert ext == {"insv2v_rowlin": 256 * 960 * 2, "insv2v_ffn_fused": 128 * 320 * 2, "insv2v_tattn_fused": 16 * 1536 * 320 * 2,
                   "insv2v_xattn_fused": 16 * 1536 * 320 * 2}
    # windows of more than 32 frames take the unfused temporal path (insv2v_rowlin / insv2v_gemm + insv2v_attention); the text
    # cross-attention still addresses a sample
    assert [e for e, _, _ in row_kernel_extents(3, 48, 64, 640)] == ["insv2v_rowlin", "insv2v_xattn_attn", "insv2v_xattn_attn"]
    assert row_kernel_extents(3, 16, 64, 1280) == []


def test_xattn_kv_stream_limit_stays():
    """The samples' K / V streams are addressed from ONE base: samples x 176 KiB (C = 320) / 320 KiB (C = 640) stay below the window."""
    assert check_operand_windows(11915, 1, 8, 8, channels=(320,)) is None
    with pytest.raises(ValueError, match="insv2v_xattn_fused"):
        check_operand_windows(11916, 1, 8, 8, channels=(320,))
    with pytest.raises(ValueError, match="insv2v_xattn_attn"):
        check_operand_windows(6554, 1, 8, 8, channels=(640,))
    with pytest.raises(ValueError):
        check_operand_windows(0, 16, 32, 48)


def _groups_before(n, cap):
    """The grouping run_stacked did before it took max_clips, restated."""
    if n <= cap:
        return [n]
    ng = -(-n // cap)
    return [n // ng + (1 if g < n % ng else 0) for g in range(ng)]


def test_stack_groups_is_the_grouping_of_run_stacked():
    for cap in range(1, 25):
        for n in range(1, 70):
            g = stack_groups(n, cap)
            assert g == _groups_before(n, cap) and sum(g) == n and max(g) <= cap and max(g) - min(g) <= 1
    assert stack_groups(0, 5) == []
    # the defaults: 20 clips at 45 x 80 run as 7 + 7 + 6 under the default cap of 9, as one chain under max_clips=20
    assert stack_groups(20, max_clips_in_flight(16, 45, 80)) == [7, 7, 6] and stack_groups(20, 20) == [20]
    assert stack_groups(46, max_clips_in_flight(16, 32, 48)) == [16, 15, 15] and stack_groups(46, 46) == [46]
    with pytest.raises(ValueError):
        stack_groups(3, 0)


def test_max_clips_parameters_default_to_none():
    assert inspect.signature(InferenceIP2PVideo.run_stacked).parameters["max_clips"].default is None
    assert inspect.signature(edit_videos).parameters["max_clips"].default is None


def test_cli_max_stack():
    p = build_parser()
    assert p.parse_args([]).max_stack is None
    assert p.parse_args(["--max-stack", "30"]).max_stack == 30
    with pytest.raises(SystemExit):
        check_args(p.parse_args(["--max-stack", "0"]))


def test_default_cap_is_unchanged():
    assert max_clips_in_flight(16, 32, 48) == 20 and max_clips_in_flight(16, 45, 80) == 9 and max_clips_in_flight(24, 48, 64) == 7
    assert max_clips_in_flight() == 20 and max_clips_in_flight(32, 152, 240) == 1
