"""How far two videos are from each other: MSE / PSNR, SSIM (Wang, Bovik, Sheikh, Simoncelli 2004) and MS-SSIM (Wang, Simoncelli, Bovik
2003) of frames, computed on the device by ``tt_frame_metrics`` / ``tt_frames_pool2`` (include/ttvdm.h states every operation).

    m = compare_frames(pipe(...).frames, reference_frames, ms_ssim=True)
    m.psnr, m.ssim, m.ms_ssim            # the video: means over its frames
    m.frame_psnr, m.frame_ssim           # per frame, numpy fp64

The kernels leave SUMS per frame and channel in device records; ``compare_frames`` copies the records to the host ONCE and everything
after that is host fp64: a frame's value is the mean over its channels and windows (pixels for the MSE), a video's value the mean over
its frames.  SSIM is the 11-tap Gaussian window (sigma 1.5) over "valid" windows only, C1 = (0.01 L)^2, C2 = (0.03 L)^2 with L = 255
for uint8 and 1 for float32 frames -- what skimage (gaussian_weights=True, use_sample_covariance=False), torchmetrics and
pytorch-msssim compute.  These are distances between two videos; what they say about picture QUALITY depends on what the second video is."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MS_SSIM_MIN_SIZE = 176          # 11 x 16: scale 5 of a 176-pixel axis still holds one full window
REC_DTYPE = np.dtype([("sse", "<f8", (4,)), ("ssim_sum", "<f8", (4,)), ("cs_sum", "<f8", (4,)), ("count", "<i8")])


@dataclass
class VideoMetrics:
    """``frame_*``: numpy fp64 per frame, shape [F] (or [B, F] for a batch of videos); the plain names: the mean over the frames of a
    video, a float (or [B]).  ``psnr`` is ``inf`` where the MSE is 0.  ``ms_ssim`` / ``frame_ms_ssim`` are None unless requested; a
    frame whose mean cs at one of scales 1-4 (or ssim at scale 5) is negative has no MS-SSIM -- the power is undefined -- and reads
    ``nan`` (it is not clamped), and so does the video that holds it."""
    data_range: float
    frame_mse: np.ndarray
    frame_psnr: np.ndarray
    frame_ssim: Optional[np.ndarray]
    frame_cs: Optional[np.ndarray]
    frame_ms_ssim: Optional[np.ndarray] = None

    @staticmethod
    def _video(x):
        if x is None:
            return None
        v = x.mean(axis=-1)
        return float(v) if v.ndim == 0 else v

    mse = property(lambda self: self._video(self.frame_mse))
    psnr = property(lambda self: self._video(self.frame_psnr))
    ssim = property(lambda self: self._video(self.frame_ssim))
    cs = property(lambda self: self._video(self.frame_cs))
    ms_ssim = property(lambda self: self._video(self.frame_ms_ssim))

    def to_dict(self) -> dict:
        """plain lists and floats for JSON; a value that is not finite travels as the string "inf" / "-inf" / "nan" """
        def plain(v):
            if v is None:
                return None
            if isinstance(v, np.ndarray):
                return [plain(e) for e in v]
            v = float(v)
            return v if np.isfinite(v) else str(v)
        out = dict(data_range=self.data_range)
        for name in ("mse", "psnr", "ssim", "cs", "ms_ssim"):
            out[name] = plain(getattr(self, name))
            out["frame_" + name] = plain(getattr(self, "frame_" + name))
        return out


def _host_array(x, who="compare_frames"):
    """lists (of lists) of PIL images or arrays -> one numpy array; numpy arrays as they are"""
    if isinstance(x, np.ndarray):
        return x
    if isinstance(x, (list, tuple)):
        if not x:
            raise ValueError(f"{who}: an empty list of frames")
        return np.stack([_host_array(e, who) for e in x], 0)
    arr = np.asarray(x)                               # a PIL image
    if arr.dtype == object:
        raise ValueError(f"{who}: cannot read frames from {type(x).__name__}")
    return arr[..., None] if arr.ndim == 2 else arr


def _describe(x, who="compare_frames"):
    """-> (source, shape, kind): source is a device tensor or a numpy array, not yet uploaded or converted.  `who` names the public
    function in the messages (export.py reads its frames through this too)"""
    from .svd.pipeline_utils import DevicePixels
    if isinstance(x, DevicePixels):
        x = x.pixels
    if torch.is_tensor(x) and not x.is_cuda:
        x = x.numpy()
    if torch.is_tensor(x):
        if x.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"{who}: uint8 or float32 frames on the device, got {x.dtype}")
        kind = "uint8" if x.dtype == torch.uint8 else "float32"
    else:
        x = _host_array(x, who)
        if x.dtype != np.uint8 and not np.issubdtype(x.dtype, np.floating):
            raise ValueError(f"{who}: uint8 or floating-point frames, got {x.dtype}")
        kind = "uint8" if x.dtype == np.uint8 else "float32"
    shape = tuple(x.shape)
    if len(shape) not in (4, 5) or not 1 <= shape[-1] <= 4 or 0 in shape:
        raise ValueError(f"{who}: frames are [F, H, W, C] or [B, F, H, W, C] with 1 to 4 channels, got {shape}")
    return x, shape, kind


def _on_device(x, device):
    """the ONE upload of a host operand (uint8 stays uint8), as contiguous [N, H, W, C]"""
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x if x.dtype == np.uint8 else x.astype(np.float32, copy=False))).to(device)
    return x.reshape(-1, *x.shape[-3:]).contiguous()


def _compare(a, b, ms_ssim: bool, sse_only: bool) -> VideoMetrics:
    from . import ops
    a, shape, kind = _describe(a)
    b, shape_b, kind_b = _describe(b)
    if shape != shape_b:
        raise ValueError(f"compare_frames: the two videos differ in shape: {shape} and {shape_b}")
    if kind != kind_b:
        raise ValueError(f"compare_frames: the two videos differ in kind: {kind} and {kind_b} (both uint8, or both floating point in [0, 1])")
    h, w, ch = shape[-3:]
    if not sse_only and (h < 11 or w < 11):
        raise ValueError(f"compare_frames: SSIM needs frames of at least 11 x 11 pixels, got {h} x {w}")
    if ms_ssim and (h % 16 or w % 16 or h < MS_SSIM_MIN_SIZE or w < MS_SSIM_MIN_SIZE):
        raise ValueError(f"compare_frames: MS-SSIM needs a height and a width that are multiples of 16 and at least {MS_SSIM_MIN_SIZE} "
                         f"(five scales, the last one still a full window), got {h} x {w}")
    dev = [t.device for t in (a, b) if torch.is_tensor(t)]
    if len(dev) == 2 and dev[0] != dev[1]:
        raise ValueError(f"compare_frames: the two videos are on different devices: {dev[0]} and {dev[1]}")
    device = dev[0] if dev else torch.device("cuda")
    a, b = _on_device(a, device), _on_device(b, device)
    n = a.shape[0]
    data_range = 255.0 if kind == "uint8" else 1.0
    levels = len(MS_SSIM_WEIGHTS) if ms_ssim else 1
    records = torch.empty((levels, n, ops.METRICS_BYTES), dtype=torch.uint8, device=device)
    for lvl in range(levels):
        if lvl:
            a, b = ops.frames_pool2(a), ops.frames_pool2(b)
        ops.frame_metrics(a, b, data_range=data_range, sse_only=sse_only, out=records[lvl])
    rec = np.frombuffer(records.cpu().numpy().tobytes(), dtype=REC_DTYPE).reshape(levels, n)      # the one device-to-host copy
    return _from_records(rec, shape, data_range, sse_only)


def _from_records(rec: np.ndarray, shape, data_range: float, sse_only: bool = False) -> VideoMetrics:
    """host fp64 from here on.  rec: [levels, N] records (levels 1 or 5), shape: the videos' [F, H, W, C] or [B, F, H, W, C]"""
    h, w, ch = shape[-3:]
    lead = shape[:-3]
    mse = rec["sse"][0][:, :ch].sum(axis=1) / float(h * w * ch)
    with np.errstate(divide="ignore", invalid="ignore"):
        psnr = np.where(mse == 0.0, np.inf, 10.0 * np.log10(data_range * data_range / mse))
        if sse_only:
            return VideoMetrics(data_range, mse.reshape(lead), psnr.reshape(lead), None, None)
        windows = rec["count"].astype(np.float64) * ch
        ssim = rec["ssim_sum"][:, :, :ch].sum(axis=2) / windows            # [levels, N]
        cs = rec["cs_sum"][:, :, :ch].sum(axis=2) / windows
        ms = None
        if rec.shape[0] == len(MS_SSIM_WEIGHTS):
            wts = MS_SSIM_WEIGHTS
            ms = np.ones_like(mse)
            for lvl in range(4):
                ms = ms * np.power(cs[lvl], wts[lvl])                      # a negative mean: nan, by design
            ms = (ms * np.power(ssim[4], wts[4])).reshape(lead)
    return VideoMetrics(data_range, mse.reshape(lead), psnr.reshape(lead), ssim[0].reshape(lead), cs[0].reshape(lead), ms)


def compare_frames(a, b, *, ms_ssim: bool = False) -> VideoMetrics:
    """PSNR, SSIM (and MS-SSIM) between videos a and b.  Each may be a device uint8 or float32 NHWC tensor ([F, H, W, C] or
    [B, F, H, W, C]; float frames in [0, 1]), ``DevicePixels``, a numpy array of either shape, or a list (or list of lists) of PIL
    images -- what ``pipe(...).frames`` returns for "pil" and "np" and what ``ops.frames_out`` writes.  Host inputs are uploaded once, as
    uint8 where they are uint8.  Both must have the same shape and kind, frames of at least 11 x 11 pixels; MS-SSIM needs a height and a
    width that are multiples of 16 and at least 176.  ValueError for anything else, before any launch.  A frame whose mean cs at one of
    the first four scales is negative has the MS-SSIM ``nan`` (the power is undefined; nothing is clamped)."""
    return _compare(a, b, ms_ssim, False)


def psnr(a, b):
    """the video's PSNR in dB (mean over frames; ``inf`` for identical videos); frames of any size"""
    return _compare(a, b, False, True).psnr


def ssim(a, b):
    """the video's SSIM (mean over frames)"""
    return _compare(a, b, False, False).ssim


def ms_ssim(a, b):
    """the video's MS-SSIM (mean over frames; ``nan`` if a frame's is undefined, see ``compare_frames``)"""
    return _compare(a, b, True, False).ms_ssim
