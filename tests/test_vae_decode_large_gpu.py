"""GPU: the temporal VAE decoder at the pipelines' default size (latents 72 x 128 -> 576 x 1024 pixels) on the shipped widths, where a
chunk of 8 frames in 16-bit storage holds token tensors of 2.4 GB (256 channels at 576 x 1024: 302 MB per frame) and a chunk of 4 frames
in TT_F32 storage likewise -- tt_gemm's wide route (include/ttvdm.h "Operand sizes").

No reference runs at this size; the test uses what tests/test_vae_decoder_gpu.py already relies on: the videos of one decode call do
not mix.  Two videos decoded JOINTLY (wide route) against each video decoded ALONE (half the size: narrow route, ran before the wide
route existed):
  * TT_F32 and split16 (2 videos x 2 frames): every element inside the north-star tolerance (rtol 1e-3 / atol 1e-4);
  * 16-bit storage (2 videos x 4 frames): bit-equal if every tt_gemm launch of the joint decode ran the tile configuration of its
    counterpart in the decodes alone.  It does not: at half the rows several Linear launches change route (the q / k / v projections of
    the mid-block attention are 576 tiles of the persistent kernel jointly and 288 tiles of the tiled template alone), as they do between
    any two chunk sizes.  Then: relative L2 between joint and alone at most TWICE what the commit before the wide route gives for the
    same comparison at a size both sides of which it runs -- 2 videos x 2 frames jointly against alone, measured on MI355X:
        bf16  2.02856e-2 (max abs 2.9e-2)   fp16  2.54558e-3 (max abs 3.9e-3)      (worst of the two videos; this commit gives the same
        figures there, digit for digit: nothing on that side of 2 GiB changed)
    (the factor 2 is this project's usual margin over a measured value).
Every leg prints its max abs difference and asserts that the joint decode really took the wide route (ops.WIDE_LAUNCHES)."""
import re

import pytest
import torch

from tests.parity_common import assert_north_star, err_stats
from tests.test_vae_decoder_gpu import REAL

pytestmark = pytest.mark.gpu
PARENT_REL_L2 = {torch.bfloat16: 2.02856e-2, torch.float16: 2.54558e-3}
LAT_H, LAT_W = 72, 128


def _model(dtype):
    from this_and_that_vdm_amd.svd.autoencoder_kl_temporal_decoder import AutoencoderKLTemporalDecoder
    from this_and_that_vdm_amd.utils.synthetic import fill_parameters_
    with torch.device("cuda"):
        p = AutoencoderKLTemporalDecoder(**REAL).to(dtype).eval()
    with torch.no_grad():
        fill_parameters_(p, "vae.")
    if dtype == torch.float32:
        p.compute_dtype = torch.float32
    return p.prepare()


def _latents(videos, frames, dtype):
    g = torch.Generator(device="cuda").manual_seed(17)
    return (torch.randn(videos * frames, 4, LAT_H, LAT_W, generator=g, device="cuda") * 3.0).to(dtype).float()


def _decode(ops, p, z, frames):
    """(sample, tile configuration of every tt_gemm launch -- the kernel instance without the wide flag --, wide launches)"""
    n0 = ops.WIDE_LAUNCHES
    ops.PROFILE = []
    try:
        out = p.decode(z, num_frames=frames).sample
        torch.cuda.synchronize()
        names = [r[0] for r in ops.PROFILE]
    finally:
        ops.PROFILE = None

    def narrow_name(n):
        m = re.fullmatch(r"(gemm_kernel<.*, )(\d+)>", n)
        return f"{m.group(1)}{int(m.group(2)) & ~64}>" if m else n
    return out, [narrow_name(n) for n in names], ops.WIDE_LAUNCHES - n0


def _legs(dtype, split16, frames):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from this_and_that_vdm_amd import ops
    ops.set_f32_split(split16)
    try:
        p = _model(dtype)
        z = _latents(2, frames, dtype)
        joint, cfg_joint, wide = _decode(ops, p, z, frames)
        assert joint.shape == (2 * frames, 3, 8 * LAT_H, 8 * LAT_W) and bool(torch.isfinite(joint).all())
        assert wide > 0, "the joint decode holds operands of 2 GiB and more: some launch must have taken the wide route"
        same = True
        for v in range(2):
            alone, cfg_alone, wide_alone = _decode(ops, p, z[v * frames:(v + 1) * frames], frames)
            assert wide_alone == 0
            same = same and cfg_alone == cfg_joint
            st = err_stats(joint[v * frames:(v + 1) * frames], alone)
            print(f"[decode 576x1024] {dtype}{' split16' if split16 else ''} video {v}: joint ({wide} wide launches) vs alone: max abs diff "
                  f"{st['max_abs']:.3g}, rel L2 {st['rel_l2']:.3g}; same tile configurations: {cfg_alone == cfg_joint}")
            yield v, joint[v * frames:(v + 1) * frames], alone, st, same
    finally:
        ops.set_f32_split(False)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@torch.no_grad()
def test_8_frames_at_576x1024_in_16_bit_storage(dtype):
    for v, joint, alone, st, same in _legs(dtype, False, 4):
        if same:
            assert torch.equal(joint, alone), f"video {v}: same tile configurations, different bits"
        else:
            assert st["rel_l2"] <= 2 * PARENT_REL_L2[dtype], (v, st)


@pytest.mark.parametrize("split16", [False, True], ids=["TT_F32", "split16"])
@torch.no_grad()
def test_4_frames_at_576x1024_in_fp32_storage(split16):
    for v, joint, alone, st, same in _legs(torch.float32, split16, 2):
        assert_north_star(joint, alone, f"video {v} decoded jointly against alone")
