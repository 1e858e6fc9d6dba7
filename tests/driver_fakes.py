"""CPU fakes of the model and the pipe that the drivers of ``insv2v/run_loveu_tgve.py`` are driven with in the ``*_cpu.py`` tests: the
model encodes and decodes by indexing, the pipe returns its ``latent`` and records the keywords of every call."""
import torch


class Model:
    scale_factor = 0.5

    class unet:
        device = torch.device("cpu")

    def encode_image_to_latent(self, frames, noise=None, **kw):
        return frames[:, :, :1].repeat(1, 1, 4, 1, 1)[..., ::8, ::8].contiguous()

    def decode_latent_to_image(self, latent):
        return latent[:, :, :3].repeat_interleave(8, -1).repeat_interleave(8, -2)


class UnseededModel(Model):
    """A model whose encoder must see no seed keyword."""

    def encode_image_to_latent(self, frames, noise=None, **kw):
        assert not kw
        return super().encode_image_to_latent(frames, noise)


class RecordingPipe:
    """Records the keywords of every call the drivers make."""
    num_ddim_steps = 4

    def __init__(self):
        self.calls = []

    def __call__(self, **kw):
        self.calls.append(("call", sorted(kw)))
        return {"latent": kw["latent"]}

    def second_clip_forward(self, **kw):
        self.calls.append(("second", sorted(kw)))
        return {"latent": kw["latent"]}

    def run_stacked(self, calls, **kw):
        self.calls.append(("stacked", [sorted(c) for c in calls], sorted(kw)))
        return [{"latent": c["latent"]} for c in calls]
