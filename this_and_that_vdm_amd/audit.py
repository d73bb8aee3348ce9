"""Range audit: which tensor first went non-finite, which site would overflow in fp16 but not in bf16, how many Q / K / V values the
fp8 attention route clipped -- answered on the device, with exact integers.

    with audit.RangeAudit() as a:
        audit.watch(unet, "unet")
        loop.begin(...); loop.run()
    rep = a.report()
    print(rep.verdict("fp16"))

While the ``with`` block is active (``ops.AUDIT`` is set), every ops function that records a write in the ledger (``ops._wrote``) also
runs ``tt_tensor_stats`` over the tensor it just wrote, on the same stream, accumulating into the record slot of the call's SITE.  A
captured DenoiseLoop step contains those launches, so a replayed graph audits every step and the report needs ONE device-to-host copy.

Site names: ``<module path>/<op>#<n>`` -- the innermost watched module whose forward is running (torch's global forward hooks,
installed only while an audit is active), the ops function, and the ordinal of the call among that module's calls of that op in the
current step (a module invoked twice in one step keeps counting, so names stay unique).  Calls outside any watched module are
``<top>/<op>#<n>``.  ``region(name)`` marks a repeated stretch (DenoiseLoop wraps each step in one, "step" -- or "step.unet_only"
where the control-guidance window drops GestureNet): every entry restarts the ordinals where the first entry started them, so a site
revisited in a later step gets the same name and the same slot; unwatched calls inside it are ``<step>/<op>#<n>``.

What the audit CANNOT see: values that never reach memory.  Attention probabilities (the flash kernels keep them in registers), the
GEGLU gate inside the persistent GEMM (only the gated product is stored) and every fp32 accumulator (only the rounded output is
stored) are invisible to it; an overflow there shows up only in what the kernel stores afterwards.  Padding a kernel zeroes (the
sequence padding of V^T, the zero tail of patch rows) is counted as zeros of the site.  And magnitudes measured on synthetic
(hash-filled) weights say nothing about a trained checkpoint: run the audit on the checkpoint in question.
"""
from __future__ import annotations

import ctypes as C
import itertools
import json
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, ops

STATS_BYTES = C.sizeof(_lib.TtTensorStats)
# the record as a numpy structured type (field order and offsets of include/ttvdm.h)
STATS_DTYPE = np.dtype([("count", "<u8"), ("n_nan", "<u8"), ("n_pinf", "<u8"), ("n_ninf", "<u8"), ("n_zero", "<u8"), ("n_ge", "<u8", (4,)),
                        ("hist", "<u8", (64,)), ("sum", "<f8"), ("sum_sq", "<f8"), ("max_abs", "<f4"), ("min_abs_nonzero", "<f4"),
                        ("max_val", "<f4"), ("min_val", "<f4")])
assert STATS_DTYPE.itemsize == STATS_BYTES == 616

THR_E4M3, THR_FP16, THR_SPLIT16 = 448.0, 65520.0, 16773120.0        # e4m3 saturates; rounds to inf in fp16; split16's high term overflows
DEFAULT_THRESHOLDS = ops.STATS_THRESHOLDS                            # the three above and one free threshold
HIST_BIAS = 40                                                       # hist[b] holds finite non-zero |x| in [2^(b-40), 2^(b-39)); b = 0 also everything below
BF16_OVERFLOW = float(np.frombuffer(np.uint32(0x7f7f8000).tobytes(), np.float32)[0])     # the smallest fp32 magnitude that rounds to inf in bf16

# Ledger writes that are NOT audited, with the reason.  Only fp32 statistic or scratch buffers may stand here -- never a tensor a later
# launch reads as an activation operand.  (The fp32 statistic buffers the library has today -- groupnorm_stats' scale / shift rows,
# gemm's per-tile column sums -- are not ledger writes at all, so the set is empty; uint8 outputs are skipped by type, not by name.)
EXEMPT: Dict[str, str] = {}

_GENERATION = itertools.count(1)
_DTYPE_NAME = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16", torch.float8_e4m3fn: "e4m3"}


def empty_record() -> np.ndarray:
    """the record of no values at all: zeros, max_abs 0, min_abs_nonzero +inf, max_val -inf, min_val +inf"""
    r = np.zeros((), STATS_DTYPE)
    r["min_abs_nonzero"], r["max_val"], r["min_val"] = np.inf, -np.inf, np.inf
    return r


def decode(buf, n: Optional[int] = None) -> List[dict]:
    """Records (a uint8 torch tensor on any device, a numpy array or bytes, whole records) -> a list of dicts of plain Python numbers:
    the fields of TtTensorStats, ``n_ge`` and ``hist`` as lists.  A device tensor costs one device-to-host copy."""
    if isinstance(buf, torch.Tensor):
        buf = buf.detach().reshape(-1).cpu().numpy()
    raw = np.frombuffer(bytes(buf), np.uint8) if isinstance(buf, (bytes, bytearray)) else np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    if raw.size % STATS_BYTES:
        raise ValueError(f"{raw.size} bytes are not a whole number of {STATS_BYTES}-byte records")
    recs = raw.view(STATS_DTYPE)
    out = []
    for r in recs[:n]:
        d = {}
        for name in STATS_DTYPE.names:
            v = r[name]
            d[name] = [int(x) for x in v] if v.ndim else (int(v) if v.dtype.kind == "u" else float(v))
        out.append(d)
    return out


def watch(model: torch.nn.Module, root: str) -> None:
    """Name the modules of `model` for the active audit: sites inside ``model.<path>``'s forward become ``<root>.<path>/op#n``."""
    if ops.AUDIT is None:
        raise RuntimeError("audit.watch: no RangeAudit is active (call it inside the `with` block)")
    ops.AUDIT.watch(model, root)


class RangeAudit:
    """Context manager: sets the process-wide ``ops.AUDIT`` (like ops.PROFILE / ops.NORM_TRACE; one audit at a time) and holds the device
    buffer of ``capacity`` records.  ``thresholds``: the four fp32 values of n_ge (verdict() needs the defaults' first three).
    ``keep_tensors=True`` (debugging, eager launches only): a clone of every audited tensor is kept in ``kept[site]``; a site visited
    again keeps its last tensor."""

    def __init__(self, capacity: int = 8192, thresholds: Sequence[float] = DEFAULT_THRESHOLDS, keep_tensors: bool = False, device=None):
        if capacity < 1 or len(thresholds) != 4:
            raise ValueError("RangeAudit: capacity >= 1 and four thresholds")
        self.capacity, self.thresholds, self.keep_tensors = int(capacity), tuple(float(t) for t in thresholds), bool(keep_tensors)
        self.generation = next(_GENERATION)
        self._thr = (C.c_float * 4)(*self.thresholds)
        self._device = device
        self.buf: Optional[torch.Tensor] = None
        self._slots: Dict[str, int] = {}
        self._meta: List[tuple] = []                    # slot -> (site, shape, dtype name)
        self.kept: Dict[str, torch.Tensor] = {}
        self._paths: Dict[int, str] = {}
        self._stack: List[Optional[str]] = []
        self._counters: Dict[tuple, int] = {}
        self._region_base: Dict[str, Dict[tuple, int]] = {}
        self._hooks = []
        self._top = "<top>"

    # ---- activation
    def __enter__(self):
        if ops.AUDIT is not None:
            raise RuntimeError("a RangeAudit is already active")
        from torch.nn.modules import module as _m
        self._hooks = [_m.register_module_forward_pre_hook(self._pre)]
        try:
            self._hooks.append(_m.register_module_forward_hook(self._post, always_call=True))
        except TypeError:                                # (a torch without always_call: a forward that raises leaves its name on the stack,
            self._hooks.append(_m.register_module_forward_hook(self._post))      # which __exit__ clears)
        ops.AUDIT = self
        return self

    def __exit__(self, *exc):
        ops.AUDIT = None
        for h in self._hooks:
            h.remove()
        self._hooks, self._stack = [], []
        return False

    def _pre(self, module, args):
        self._stack.append(self._paths.get(id(module)))

    def _post(self, module, args, output):
        if self._stack:
            self._stack.pop()

    def watch(self, model: torch.nn.Module, root: str) -> None:
        for name, m in model.named_modules():
            self._paths[id(m)] = f"{root}.{name}" if name else root

    class _Region:
        def __init__(self, audit, name):
            self.audit, self.name = audit, name

        def __enter__(self):
            a = self.audit
            a._counters = dict(a._region_base.setdefault(self.name, dict(a._counters)))
            self.outer, a._top = a._top, f"<{self.name}>"
            return a

        def __exit__(self, *exc):
            self.audit._top = self.outer
            return False

    def region(self, name: str):
        """A stretch that repeats (one denoise step): every entry restarts the site ordinals where the FIRST entry of `name` started them,
        and calls outside any watched module are named ``<name>/op#n`` inside it (two kinds of step never share such a site)."""
        return RangeAudit._Region(self, name)

    # ---- called by ops._wrote
    def site_name(self, op: str) -> str:
        path = next((p for p in reversed(self._stack) if p is not None), self._top)
        key = (path, op)
        n = self._counters.get(key, 0)
        self._counters[key] = n + 1
        return f"{path}/{op}#{n}"

    def record(self, t: torch.Tensor, op: str) -> None:
        if not t.is_floating_point() or op in EXEMPT:       # uint8 frames / resized pixels; named fp32 statistic buffers
            return
        name = self.site_name(op)
        slot = self._slots.get(name)
        if slot is None:
            if len(self._meta) >= self.capacity:
                raise RuntimeError(f"RangeAudit: site {name!r} is number {len(self._meta) + 1}, the audit holds {self.capacity} records "
                                   "(RangeAudit(capacity=...))")
            if self.buf is None:
                dev = t.device if self._device is None else torch.device(self._device)
                one = torch.from_numpy(np.frombuffer(empty_record().tobytes(), np.uint8).copy())
                self.buf = one.repeat(self.capacity).to(dev)
            slot = self._slots[name] = len(self._meta)
            self._meta.append((name, tuple(t.shape), _DTYPE_NAME.get(t.dtype, str(t.dtype))))
        if t.device != self.buf.device:
            raise RuntimeError(f"RangeAudit: site {name!r} is on {t.device}, the audit's records on {self.buf.device}")
        # every slot starts as the empty record, so a first visit and a revisit (a later step, a graph replay) are the same launch
        ops.tensor_stats(t, thresholds=self._thr, out=self.buf, slot=slot, accumulate=True)
        if self.keep_tensors:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("RangeAudit(keep_tensors=True) is for eager launches only (DenoiseLoop(use_graph=False))")
            self.kept[name] = t.detach().clone()

    # ---- a capture's warm-up pass must not count: DenoiseLoop saves the records before it and puts them back afterwards
    def snapshot(self):
        return None if self.buf is None else self.buf.clone()

    def restore(self, snap) -> None:
        if self.buf is None:
            return
        if snap is None:                                 # the buffer was created during the pass: back to empty records
            one = torch.from_numpy(np.frombuffer(empty_record().tobytes(), np.uint8).copy())
            self.buf.copy_(one.repeat(self.capacity))
        else:
            self.buf.copy_(snap)

    def report(self) -> "RangeAuditReport":
        """Every site visited so far, in execution order (one device-to-host copy; synchronises the device)."""
        n = len(self._meta)
        recs = decode(self.buf[:n * STATS_BYTES]) if n else []
        rows = [dict(site=s, shape=list(shape), dtype=dt, record=r) for (s, shape, dt), r in zip(self._meta, recs)]
        return RangeAuditReport(rows, self.thresholds)


def _finite_nonzero(r: dict) -> int:
    return r["count"] - r["n_nan"] - r["n_pinf"] - r["n_ninf"] - r["n_zero"]


def _below(r: dict, exp2: int) -> int:
    """finite non-zero values with |x| < 2^exp2 (whole histogram bins: exp2 >= -39)"""
    return sum(r["hist"][:max(0, min(64, exp2 + HIST_BIAS))])


class RangeAuditReport:
    """rows: one dict per site in execution order -- ``site``, ``shape``, ``dtype`` ("f32" / "f16" / "bf16" / "e4m3"), ``record`` (decode())."""

    def __init__(self, rows: List[dict], thresholds: Sequence[float] = DEFAULT_THRESHOLDS):
        self.rows, self.thresholds = rows, tuple(float(t) for t in thresholds)

    def __len__(self):
        return len(self.rows)

    def sites(self) -> List[str]:
        return [r["site"] for r in self.rows]

    def row(self, site: str) -> dict:
        return next(r for r in self.rows if r["site"] == site)

    def nonfinite(self) -> List[dict]:
        """the sites that hold NaN or +-inf, in execution order.  After ONE step the first of them is where the step first went non-finite
        in memory; records accumulate over steps and a spoiled step hands its latents to the next, so after several steps the sites
        before that one hold NaN as well"""
        return [r for r in self.rows if r["record"]["n_nan"] + r["record"]["n_pinf"] + r["record"]["n_ninf"] > 0]

    def worst(self, k: int = 10) -> List[dict]:
        """the k sites with the largest finite magnitude (ties in execution order)"""
        return sorted(self.rows, key=lambda r: -r["record"]["max_abs"])[:k]

    def _thr_index(self, value: float) -> int:
        if value not in self.thresholds:
            raise RuntimeError(f"verdict needs the threshold {value} among the audit's ({self.thresholds})")
        return self.thresholds.index(value)

    def verdict(self, storage: str) -> dict:
        """What storing this run's tensors in `storage` would do, from the records alone:
          "fp16"           sites whose finite values reach 65520 (they round to inf in fp16; sites already stored in fp16 show the damage
                           as +-inf instead and are listed with that count); flush: |x| < 2^-25 becomes zero
          "bf16"           sites whose max_abs rounds to inf in bf16 (the count is not recorded: None); fp32's exponent range, so
                           nothing flushes that fp32 holds as a normal number (reported 0)
          "split16"        fp32 sites with values at or above 65520 * 2^8, where the high term h = fp16(x 2^-8) overflows; flush:
                           |x| < 2^-28, where the low term fp16(8 x) is zero as well
          "fp8_attention"  the e4m3 sites (Q | K, V^T of the fp8 attention route) with values AT the clip 448 (the conversion saturates,
                           so these were >= 448 before it); flush: their zeros (the values that flushed cannot be told from true zeros)
        -> {"storage", "sites": [{"site", "dtype", "count", "share"}] in execution order, "first": the first such site or None,
            "flush_share": the share of finite non-zero values (zeros for fp8_attention: of all values) over the considered sites that
            would flush to zero, "considered": how many sites the verdict looked at}"""
        hits, flushed, base, considered = [], 0, 0, 0
        for row in self.rows:
            r, dt = row["record"], row["dtype"]
            n = None
            if storage == "fp16":
                n = r["n_pinf"] + r["n_ninf"] if dt == "f16" else r["n_ge"][self._thr_index(THR_FP16)]
                flushed, base = flushed + _below(r, -25), base + _finite_nonzero(r)
            elif storage == "bf16":
                n = (None if r["max_abs"] >= BF16_OVERFLOW else 0) if dt == "f32" else r["n_pinf"] + r["n_ninf"] if dt == "bf16" else 0
                base += _finite_nonzero(r)
            elif storage == "split16":
                if dt != "f32":
                    continue
                n = r["n_ge"][self._thr_index(THR_SPLIT16)]
                flushed, base = flushed + _below(r, -28), base + _finite_nonzero(r)
            elif storage == "fp8_attention":
                if dt != "e4m3":
                    continue
                n = r["n_ge"][self._thr_index(THR_E4M3)]
                flushed, base = flushed + r["n_zero"], base + r["count"]
            else:
                raise ValueError(f"verdict: storage {storage!r} (fp16, bf16, split16 or fp8_attention)")
            considered += 1
            if n is None or n > 0:
                hits.append(dict(site=row["site"], dtype=dt, count=n, share=None if n is None or not r["count"] else n / r["count"]))
        return dict(storage=storage, sites=hits, first=hits[0]["site"] if hits else None, flush_share=flushed / base if base else 0.0,
                    considered=considered)

    def to_json(self, **kw) -> str:
        """rows and thresholds as JSON (non-finite floats as the strings "inf" / "-inf" / "nan": strict JSON has no spelling for them)"""
        def clean(v):
            if isinstance(v, float) and not math.isfinite(v):
                return "nan" if v != v else ("inf" if v > 0 else "-inf")
            if isinstance(v, dict):
                return {k: clean(x) for k, x in v.items()}
            if isinstance(v, (list, tuple)):
                return [clean(x) for x in v]
            return v
        return json.dumps(dict(thresholds=list(self.thresholds), rows=clean(self.rows)), allow_nan=False, **kw)

    def table(self, storages=("fp16", "bf16", "split16", "fp8_attention")) -> str:
        lines = [f"{len(self.rows)} sites; non-finite: {len(self.nonfinite())}" +
                 (f" (first: {self.nonfinite()[0]['site']})" if self.nonfinite() else "")]
        for s in storages:
            v = self.verdict(s)
            lines.append(f"{s:14s} {len(v['sites']):5d} of {v['considered']:5d} sites overflow / clip, flush share {v['flush_share']:.3e}" +
                         (f", first: {v['first']}" if v["first"] else ""))
        for r in self.worst(5):
            lines.append(f"  max_abs {r['record']['max_abs']:.6g}  {r['dtype']:5s} {r['site']}")
        return "\n".join(lines)
