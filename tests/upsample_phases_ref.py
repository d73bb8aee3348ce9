"""Reference arithmetic of tt_gemm's ``upsample = 2`` (the nearest-x2 upsampling 3x3 conv on phase-packed weights), shared by
tests/test_upsample_phases_cpu.py and tests/test_upsample_phases_gpu.py.  A plain module, not a conftest.

Output pixel (Y, X) of phase (py, px) = (Y & 1, X & 1) sees 2 x 2 distinct low-res pixels: tap (r, c) of the phase reads low-res
pixel (Y // 2 + r - 1 + py, X // 2 + c - 1 + px), and a pixel outside the LOW-RES image reads as zero (that alone reproduces the zero
padding of the upsampled image)."""
import torch
import torch.nn.functional as F

ROWS = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}          # phase -> the 3x3 rows (columns) that fall on its tap 0 and on its tap 1


def phase_conv(x: torch.Tensor, wp: torch.Tensor) -> torch.Tensor:
    """x [nimg, I, h, w], wp [O, 16 * I] with k index (phase py*2 + px, tap r*2 + c, channel) -> [nimg, O, 2h, 2w]: the four 2 x 2
    convs, written independently of the pack (and of the kernel's index arithmetic)"""
    n, i, h, w = x.shape
    o = wp.shape[0]
    taps = wp.reshape(o, 2, 2, 2, 2, i)
    out = torch.zeros(n, o, 2 * h, 2 * w, dtype=x.dtype)
    xp = F.pad(x, (1, 1, 1, 1))
    for py in (0, 1):
        for px in (0, 1):
            e = taps[:, py, px].permute(0, 3, 1, 2).contiguous()                 # [O, I, r, c]
            out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + h + 1, px:px + w + 1], e)
    return out


def upsample_conv(x: torch.Tensor, w9: torch.Tensor) -> torch.Tensor:
    """what Upsample2D computes: F.conv2d(F.interpolate(nearest x2), 3x3, padding 1)"""
    return F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w9, padding=1)


def summed_taps(w9: torch.Tensor, acc_dtype) -> torch.Tensor:
    """[O, I, 3, 3] -> [O, 16 * I]: the taps of every phase added up in `acc_dtype`, written without the pack's loop order (one
    index_select + sum per tap)"""
    o, i = w9.shape[:2]
    w = w9.to(acc_dtype)
    blocks = []
    for py in (0, 1):
        for px in (0, 1):
            for r in (0, 1):
                for c in (0, 1):
                    sub = w[:, :, list(ROWS[py][r])][:, :, :, list(ROWS[px][c])]
                    t = sub[:, :, 0, 0].clone()
                    for a in range(sub.shape[2]):
                        for b in range(sub.shape[3]):
                            if a or b:
                                t = t + sub[:, :, a, b]
                    blocks.append(t)
    return torch.stack(blocks, 1).reshape(o, 16 * i)
