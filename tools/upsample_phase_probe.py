"""The three Upsample2D convs of the UNet decoder at 32x56 latents (CFG batch 2 x 14 frames), nine-tap index map (tt_gemm upsample = 1)
against the phase-packed route (upsample = 2) on the tile shapes it may take: us per launch in isolation, warm operands, eager.
An isolated sweep does not predict the step: it only ranks tile shapes per level; the step decides (bench.py, A/B with
TT_UPSAMPLE_PHASES).   usage: python tools/upsample_phase_probe.py [reps]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from this_and_that_vdm_amd import _lib, ops                      # noqa: E402
from this_and_that_vdm_amd.packing import pack_conv3x3, pack_upsample_phases      # noqa: E402

LEVELS = [(28, 16, 28, 640), (28, 8, 14, 1280), (28, 4, 7, 1280)]      # (nimg, h, w, C): output rows 50176 / 12544 / 3136
TILES = {11: "128x128x64 2-deep 8 waves", 3: "256x128x32 3-deep", 16: "128x128x64 4-deep 8 waves"}


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    lib = _lib.load()
    dt = torch.bfloat16
    for nimg, h, w, c in LEVELS:
        x = torch.randn(nimg * h * w, c, device="cuda").to(dt)
        wt = (torch.randn(c, c, 3, 3) * (9 * c) ** -0.5).to(dt)
        w9, wp = pack_conv3x3(wt).cuda(), pack_upsample_phases(wt, dt).cuda()
        bias = torch.zeros(c, device="cuda")
        out = torch.empty(nimg * 4 * h * w, c, device="cuda", dtype=dt)
        conv = lambda up: (nimg, h, w, 2 * h, 2 * w, 1, up)
        gf = 2.0 * nimg * 4 * h * w * c * c * 1e-9
        t1 = timed(lambda: ops.gemm(x, w9, mode=1, conv=conv(1), bias=bias, out=out), reps)
        line = f"{nimg * 4 * h * w:6d} x {c:4d} x 9*{c:<4d}  upsample=1 {t1:7.1f} us ({9 * gf / t1 * 1e3:5.0f} TFLOP/s) | upsample=2:"
        for cfg in (-1, 11, 3, 16):
            lib.tt_gemm_set_tile_override(cfg)
            try:
                t2 = timed(lambda: ops.gemm(x, wp, mode=1, conv=conv(2), bias=bias, out=out), reps)
            finally:
                lib.tt_gemm_set_tile_override(-1)
            line += f"  {'planner' if cfg < 0 else 'cfg %d' % cfg} {t2:6.1f} us ({4 * gf / t2 * 1e3:4.0f})"
        print(line, flush=True)


if __name__ == "__main__":
    main()
