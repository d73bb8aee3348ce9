"""Route census of tt_gemm's host planner (csrc/gemm.hip): a fixed list of problems and knob states, and for each the answers of
the four planner entry points -- (tt_gemm_plan's return code, cfg[0..6], tt_gemm_ws_bytes, tt_gemm_stats_rows, tt_gemm_gn_fused).

The planner looks at the pointers of a problem (null or not, alignment) and never follows them, so the addresses here are made up
and nothing needs a GPU.  The library caches its knobs per process, so the census is taken in a process of its own:

    python -m tests.gemm_route_census            # prints {"sha": <of the problem list>, "answers": [...], "rows": [...]} as JSON

tests/test_gemm_routes_cpu.py runs that with every TT_* variable removed and compares it with tests/golden/gemm_route_census.json;
tests/golden/make_gemm_route_census.py writes the fixture from another build of the library (TT_LIBTTVDM)."""
import ctypes as C
import hashlib
import json
import os
import sys

BF16, F16, F32 = 0, 1, 2
PTR = dict(a0=0x10000, a1=0x18000, w=0x20000, out=0x30000, residual=0x40000, blend=0x50000, rowvec=0x60000, bias=0x70000,
           stats_out=0x80000, ws=0x100000)
ENV_PREFIX = "TT_"


class Lcg:
    """The sample's own generator: the census must not change with the Python version."""
    def __init__(self, seed):
        self.x = seed

    def below(self, n):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) % 2 ** 64
        return (self.x >> 33) % n

    def pick(self, seq):
        return seq[self.below(len(seq))]


# ---- problems: dicts of TtGemmArgs fields (pointers by name: True = the aligned made-up address, an int = that address)
def linear(m, n, k, k1=0, **kw):
    return dict(dict(mode=0, m=m, n=n, k0=k, k1=k1), **kw)


def conv(nimg, h, w, cin, n, k1=0, stride=1, upsample=0, mode=1, **kw):
    if mode == 3:
        ho, wo = (h + 1 - 3) // stride + 1, (w + 1 - 3) // stride + 1
    elif upsample:
        ho, wo = 2 * h, 2 * w
    else:
        ho, wo = (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1
    return dict(dict(mode=mode, m=nimg * ho * wo, n=n, k0=cin, k1=k1, nimg=nimg, hin=h, win=w, hout=ho, wout=wo, stride=stride,
                     upsample=upsample), **kw)


def tconv(batch, frames, hw, k, n, k1=0, **kw):
    return dict(dict(mode=2, m=batch * frames * hw, n=n, k0=k, k1=k1, frames=frames, hw=hw), **kw)


# rows of the step: 32x56 latents (50 176 / 12 544 / 3 136 / 784), 32x48 (10 752 / 2 688), 64x112 (200 704 / 100 352), and ragged counts
STEP_ROWS = [50176, 12544, 3136, 784, 10752, 2688, 200704, 100352]
RAGGED_ROWS = [50000, 12545, 3137, 777, 1568, 392, 64, 33, 6000, 25000]
WIDTHS = [320, 640, 960, 1280, 2560, 5120, 10240]
DEPTHS = [320, 640, 1280, 2560, 5120]
# (nimg, h, w) of the UNet levels whose rows are the counts above
LEVELS = [(28, 32, 56), (28, 16, 28), (28, 8, 14), (28, 4, 7), (7, 32, 48), (7, 16, 24), (28, 64, 112), (14, 64, 112)]
CONV_CH = [(320, 0), (640, 0), (1280, 0), (1920, 0), (2560, 0), (320, 320), (640, 320), (640, 640), (1280, 640), (1280, 1280)]
# the VAE encoder's three mode-3 downsamples at 256x448 for one / 15 images, a tiny one, and two whose un-remapped plan is the wide / N = 160 t tile
MODE3 = [(1, 256, 448, 128, 128), (15, 256, 448, 128, 128), (1, 128, 224, 256, 256), (15, 128, 224, 256, 256), (1, 64, 112, 512, 512),
         (15, 64, 112, 512, 512), (3, 16, 32, 32, 32), (15, 64, 112, 512, 1024), (40, 32, 32, 64, 160), (15, 64, 112, 512, 320)]


def named_problems():
    out = []
    for m in STEP_ROWS + RAGGED_ROWS:
        for n in WIDTHS:
            for k in DEPTHS:
                out.append(linear(m, n, k))
    for m in STEP_ROWS + RAGGED_ROWS[:4]:                         # the GEGLU projections (N = 8 C) and two-source linears
        for c in (320, 640, 1280):
            out.append(linear(m, 8 * c, c, geglu=1, ldo=4 * c))
            out.append(linear(m, c, c, k1=c))
    for lv in LEVELS:
        for cin, k1 in CONV_CH:
            for n in (320, 640, 1280):
                out.append(conv(*lv, cin, n, k1=k1))
        out.append(conv(*lv, 320, 320, stride=2))
        out.append(conv(*lv, 1280, 1280, stride=2))
        out.append(conv(*lv, 640, 640, upsample=1))
        for k, k1 in ((320, 0), (640, 0), (1280, 0), (640, 640)):
            frames = 14 if lv[0] % 14 == 0 else 7
            out.append(tconv(lv[0] // frames, frames, lv[1] * lv[2], k, k, k1=k1))
    for s in MODE3:
        out.append(conv(*s[:4], s[4], stride=2, mode=3))
        out.append(conv(*s[:4], s[4], stride=2, mode=1))           # its mode-1 twin: what the plan would be without mode3_plan
    return out


def seg_of(p, rng):
    """A stats_seg for the problem: the consumer's GroupNorm segment (rows per frame), or one that does not divide the tile heights."""
    hw = p.get("hout", 0) * p.get("wout", 0) or p.get("hw", 0)
    cands = [64, 96, 100, 128, 192, 256, 448, 1792, 28, 112]
    if hw:
        cands += [hw, hw, hw]
    for d in (1792, 448, 112, 28):
        if p["m"] % d == 0:
            cands += [d, d]
    return rng.pick(cands)


def flag_variants(p, rng):
    """One problem with a seeded choice of the epilogue flags that steer routing."""
    q = dict(p)
    n, m = q["n"], q["m"]
    kind = rng.below(22)
    if kind == 0 and q["mode"] == 0 and n % 16 == 0:
        q.update(geglu=1, ldo=n // 2)
    elif kind == 1:
        q.update(residual=True, ld_res=n)
    elif kind == 2:
        q.update(residual=True, ld_res=n, blend=PTR["residual"], ld_blend=n)                 # a blend with the residual itself
    elif kind == 3:
        q.update(residual=True, ld_res=n, blend=True, ld_blend=n)
    elif kind == 4:
        q.update(blend=True, ld_blend=n)
    elif kind == 5:
        rows = next((d for d in (1792, 448, 112, 64, 32) if m % d == 0), 32)
        q.update(rowvec=True, rowvec_rows=rows, ld_rowvec=n, residual=rng.below(2) == 0, ld_res=n)
    elif kind == 6:
        q.update(rowvec=True, rowvec_rows=1, rowvec_mod=2, ld_rowvec=n, residual=rng.below(2) == 0, ld_res=n)
    elif kind == 7:
        q.update(rowvec=True, rowvec_rows=rng.pick([16, 7, 28]), ld_rowvec=n)
    elif kind == 8:
        q.update(rowvec=True, rowvec_rows=(m // 2 + 31) // 32 * 32, ld_rowvec=n, residual=True, ld_res=n)   # two groups over the launch
    elif kind == 9 and q["mode"] == 0:
        q.update(ln_fold=1, ln_eps=1e-5)
    elif kind == 10 and q["mode"] == 0:
        q.update(ln_fold=2, ln_eps=1e-5)
    elif kind == 11:
        q.update(out_fp8=1)
    elif kind == 12:
        q.update(out_f32=1)
    elif kind == 13:
        hw = q.get("hout", 0) * q.get("wout", 0) or q.get("hw", 0) or 64
        q.update(out_col_hw=hw, out_col_hwp=hw, ldo=hw)
    elif kind == 14:
        q.update(out=PTR["out"] + 4)                                                       # misaligned: 8-byte epilogue stores
    elif kind == 15:
        q.update(bias=PTR["bias"] + 8)                                                     # ... 16-byte fp32 vectors
    elif kind == 16:
        q.update(ldo=n + 2)
    elif kind == 17:
        q.update(ldo=n + 4)
    elif kind == 18:
        q.update(residual=PTR["residual"] + 4, ld_res=n + 2)
    elif kind == 19:
        q.update(presplit=1 + rng.below(3))
    if rng.below(3) == 0:
        q["bias"] = q.get("bias", True)
    if rng.below(2) == 0:
        q["stats_seg"] = seg_of(q, rng)
        if rng.below(3) == 0:
            q["stats_out"] = True
    return q


def problems():
    """[(problem, in_every_knob_state)]: the named shapes on 16-bit storage, then a seeded sample of flags / dtypes on top of them."""
    rng = Lcg(20251016)
    named = named_problems()
    out = [(dict(p, dtype=BF16), False) for p in named]
    out += [(dict(p, dtype=F32), False) for i, p in enumerate(named) if i % 3 == 0]
    for i in range(2600):
        p = flag_variants(rng.pick(named), rng)
        p["dtype"] = rng.pick([BF16, BF16, F16, F32])
        out.append((p, i % 8 == 0))
    # the problems every knob state sees: the sample's every eighth, the mode-3 pairs, and a few routes by name
    keep = [conv(*s[:4], s[4], stride=2, mode=3) for s in MODE3] + [conv(*s[:4], s[4], stride=2, mode=1) for s in MODE3[-3:]]
    keep += [linear(50176, 2560, 320, geglu=1, ldo=1280), linear(3136, 10240, 1280, geglu=1, ldo=5120), linear(200704, 320, 320),
             linear(200704, 320, 320, residual=True, ld_res=320), linear(50176, 320, 320), linear(50176, 320, 320, ln_fold=1, ln_eps=1e-5),
             conv(28, 32, 56, 320, 320), conv(28, 16, 28, 640, 640), conv(28, 8, 14, 1280, 1280), conv(28, 4, 7, 1280, 1280),
             conv(28, 8, 14, 1280, 1280, k1=1280, stats_seg=112), linear(3136, 1280, 5120), linear(3136, 1280, 5120, stats_seg=112),
             linear(784, 1280, 1280), linear(12544, 1920, 640, ln_fold=1, ln_eps=1e-5), tconv(2, 14, 1792, 320, 320), linear(64, 5120, 640, geglu=1, ldo=2560),
             linear(8000, 640, 640), linear(4096, 1280, 1280), linear(5000, 1024, 1024),    # 257..383 tiles of 128 x 128, short K: the 128 x 64 tile
             linear(4864, 1280, 1280), linear(4992, 1280, 1280), linear(3200, 1280, 5120), linear(3328, 1280, 5120)]   # either side of 384 / 256 tiles
    for p in keep:
        for dt in (BF16, F16, F32):
            out.append((dict(p, dtype=dt), True))
    return out


# ---- knob states: (setter, value, value that restores the default)
def knob_states():
    st = [("default", None, None)]
    st += [("tt_gemm_set_tile_override", c, -1) for c in range(21)]
    st += [("tt_gemm_set_big_tile", v, 1) for v in (0, 2, 3, 4)]
    st += [("tt_gemm_set_streaming_square", v, 2) for v in (0, 1)]
    st += [("tt_gemm_set_f32_split", 1, 0)]
    return st


def to_args(p):
    from this_and_that_vdm_amd._lib import TtGemmArgs
    taps = {0: 1, 1: 9, 2: 3, 3: 9}[p["mode"]]
    g = TtGemmArgs()
    f = dict(a0=True, lda0=p["k0"], w=True, ldw=taps * (p["k0"] + p["k1"]), out=True, ldo=p["n"])
    if p["k1"]:
        f.update(a1=True, lda1=p["k1"])
    f.update(p)
    for k, v in f.items():
        if k in PTR:
            v = PTR[k] if v is True else (None if v is False else v)
        setattr(g, k, v)
    return g


def answers(lib, g):
    cfg = (C.c_int32 * 7)()
    rc = lib.tt_gemm_plan(C.byref(g), cfg)
    return [rc] + list(cfg) + [lib.tt_gemm_ws_bytes(C.byref(g)), lib.tt_gemm_stats_rows(C.byref(g)), lib.tt_gemm_gn_fused(C.byref(g))]


def rows_of(probs=None):
    """[(state, problem, with_workspace)] in census order."""
    probs = problems() if probs is None else probs
    out = []
    for st in knob_states():
        for p, everywhere in probs:
            if st[0] == "default" or everywhere:
                out += [(st, p, False), (st, p, True)]
    return out


def sha_of(rows):
    return hashlib.sha256(json.dumps([[s[0], s[1], p, w] for s, p, w in rows], sort_keys=True).encode()).hexdigest()


def walk(lib, rows):
    """The TtGemmArgs of every row, in order, with the row's knob state in force while the caller looks at it."""
    state = None
    for st, p, with_ws in rows:
        if st is not state:
            if state is not None and state[1] is not None:
                getattr(lib, state[0])(state[2])
            if st[1] is not None:
                assert getattr(lib, st[0])(st[1]) == 0, st
            state = st
        g = to_args(p)
        if with_ws:                                   # exactly the workspace tt_gemm_ws_bytes asks for
            need = lib.tt_gemm_ws_bytes(C.byref(g))
            g.ws, g.ws_bytes = (PTR["ws"], need) if need else (None, 0)
        yield g
    if state[1] is not None:
        getattr(lib, state[0])(state[2])


def take(lib, answers=answers):
    rows = rows_of()
    table, index = {}, []
    for g in walk(lib, rows):
        a = tuple(answers(lib, g))
        index.append(table.setdefault(a, len(table)))
    return dict(sha=sha_of(rows), answers=[list(a) for a in table], rows=index)


def load_lib():
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def clean_env(lib_path=None):
    """The child's environment: no TT_* variable, so a developer's shell cannot change the answers."""
    env = {k: v for k, v in os.environ.items() if not k.startswith(ENV_PREFIX)}
    if lib_path:
        env["TT_LIBTTVDM"] = lib_path
    return env


def run_child(lib_path=None):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.gemm_route_census"], cwd=root, env=clean_env(lib_path), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"route census failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(r.stdout.splitlines()[-1])


if __name__ == "__main__":
    print(json.dumps(take(load_lib()), separators=(",", ":")))
