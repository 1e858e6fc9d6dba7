"""The dispatch rule of the VAE's mid AttnBlock (insv2v/vae.py attn_plan): pure host arithmetic, no GPU.

"scores" = the three batched GEMMs around a row softmax (the [N, h*w, h*w] score tensor in memory), "flash" = insv2v_attention with one
head of C channels.  The default is a memory rule: flash above FLASH_MIN_HW = 4096 tokens for the widths the kernel takes (128, 512).
"""
import pytest


def test_threshold_constants():
    from insv2v import vae
    assert vae.FLASH_MIN_HW == 4096
    # above every geometry with a golden or a bench number (C2 h*w = 1536, C5 h*w = 3072)
    assert vae.FLASH_MIN_HW > 3072


@pytest.mark.parametrize("C,HW,want", [(512, 1536, "scores"), (512, 3072, "scores"), (512, 4096, "scores"), (512, 4097, "flash"),
                                       (128, 40000, "flash"), (256, 5000, "scores")])
def test_default_rule(C, HW, want):
    from insv2v.vae import attn_plan
    assert attn_plan(C, HW) == want
    assert attn_plan(C, HW, flash=None) == want


def test_default_refuses_what_neither_form_runs():
    from insv2v.vae import attn_plan
    with pytest.raises(ValueError) as e:
        attn_plan(256, 40000)
    assert "256" in str(e.value) and "40000" in str(e.value)
    assert str(40000 * 40000 * 2) in str(e.value)      # the byte count of one frame's scores


@pytest.mark.parametrize("HW", [1, 35, 4096, 5000, 40000])
def test_forced_flash_needs_a_width_the_kernel_takes(HW):
    from insv2v.vae import attn_plan
    with pytest.raises(ValueError) as e:
        attn_plan(256, HW, flash=True)
    assert "256" in str(e.value) and str(HW) in str(e.value)
    assert attn_plan(512, HW, flash=True) == "flash" and attn_plan(128, HW, flash=True) == "flash"


def test_forced_scores_window():
    """The batched score GEMM is refused by insv2v_gemm once one frame's scores reach 2^31 - 2^20 bytes (gemm.hip beyond_window):
    32 760^2 x 2 B is 128 bytes past that, 32 752^2 x 2 B is below."""
    from insv2v.vae import attn_plan, SCORE_WINDOW
    assert SCORE_WINDOW == 2 ** 31 - 2 ** 20
    with pytest.raises(ValueError) as e:
        attn_plan(512, 32760, flash=False)
    assert "512" in str(e.value) and "32760" in str(e.value) and str(32760 * 32760 * 2) in str(e.value)
    assert attn_plan(512, 32752, flash=False) == "scores"
    # h*w that is no multiple of 8: the score rows are padded to HWp columns
    assert attn_plan(512, 32759, flash=False) == "scores"   # 32759 x 32760 x 2 = window - 65 392
    with pytest.raises(ValueError):
        attn_plan(512, 32761, flash=False)                   # 32761 x 32768 x 2


def test_autoencoder_refuses_up_front():
    """moments / decode call attn_plan for their mid-block geometry before the first launch: a 256-wide VAE (no flash form) at a latent of
    200 x 200 raises ValueError from a model with no weights loaded and no GPU."""
    import torch
    from insv2v.vae import AutoencoderKL
    dd = dict(ch=64, ch_mult=(1, 2, 4, 4), num_res_blocks=2, attn_resolutions=[], z_channels=4, in_channels=3, out_ch=3, resolution=256,
              double_z=True, dropout=0.0)
    vae = AutoencoderKL(dd, device="cpu")
    assert vae.attn_flash is None
    with pytest.raises(ValueError) as e:
        vae.decode(torch.zeros(1, 4, 200, 200))
    assert "40000" in str(e.value)
    with pytest.raises(ValueError) as e:
        vae.moments(torch.zeros(1, 3, 1600, 1600))
    assert "40000" in str(e.value)
    with pytest.raises(ValueError):
        AutoencoderKL(dd, device="cpu", attn_flash=True).decode(torch.zeros(1, 4, 8, 8))
