"""What tests/test_kernel_names_cpu.py asks the library about kernel instance names (tt_gemm_kernel / tt_conv3x3_kernel /
tt_attention_kernel, include/ttvdm.h), in a process of its own: the library reads its knobs from the environment once.

    python -m tests.kernel_names census|grid|pins      # prints one JSON line

The queries look at the pointers of a problem (null or not, alignment) and never follow them, so the addresses are made up and
nothing needs a GPU."""
import ctypes as C
import json
import sys

from tests import gemm_route_census as census

BF16, F16, F32 = census.BF16, census.F16, census.F32


def name_of(query, args):
    """(return code, name) of a tt_*_kernel query"""
    buf = C.create_string_buffer(96)
    rc = query(C.byref(args), buf, len(buf))
    return rc, buf.value.decode()


# ---- tt_gemm_kernel over the route census: per row (tt_gemm_plan's rc, cfg[0..5], tt_gemm_is_wide, tt_gemm_kernel's rc, the name)
def gemm_answers(lib, g):
    cfg = (C.c_int32 * 7)()
    rc = lib.tt_gemm_plan(C.byref(g), cfg)
    return [rc] + list(cfg)[:6] + [lib.tt_gemm_is_wide(C.byref(g))] + list(name_of(lib.tt_gemm_kernel, g))


# ---- attention: dtype x head_dim x mask x variant x keys, as dicts; attn_args() makes a problem tt_attention's validation can accept of each
VARIANTS = ("plain", "fp8", "qx", "v_rows")
KEYS = (64, 128, 192, 200)


def attention_grid():
    return [dict(dtype=dt, head_dim=d, mask=mask, variant=v, lk=lk)
            for dt in (BF16, F16, F32) for d in (64, 128) for mask in (0, 1, 2) for v in VARIANTS for lk in KEYS]


def attn_accepted(c):
    """tt_attention's rules for the variants (include/ttvdm.h): which cases of the grid it serves"""
    if c["variant"] == "fp8":
        return c["mask"] == 0 and c["dtype"] != F32
    if c["variant"] == "qx":
        return c["mask"] != 0 and c["head_dim"] == 64 and c["dtype"] != F32
    if c["variant"] == "v_rows":
        return c["mask"] == 0 and c["head_dim"] == 64 and c["dtype"] != F32
    return True


def attn_args(c):
    from this_and_that_vdm_amd._lib import TtAttnArgs
    a = TtAttnArgs()
    nseq, lq, heads, frames, ctx = 4, 96, 2, 2, 2
    d, lk = c["head_dim"], c["lk"]
    stride = (lk + 15) // 16 * 16
    width = heads * d
    a.nseq, a.lq, a.heads, a.head_dim, a.mask, a.lk = nseq, lq, heads, d, c["mask"], lk
    a.k_seq_stride = a.v_seq_stride = stride
    a.frames, a.ctx_batches, a.dtype, a.batch0 = frames, ctx, c["dtype"], 0
    a.q, a.ldq, a.k, a.ldk, a.out, a.ldo = 0x10000, width, 0x20000, width, 0x40000, width
    a.vt, a.ldvt = 0x30000, (nseq if c["mask"] == 0 else ctx) * stride
    if c["variant"] == "fp8":
        a.fp8 = 1
    elif c["variant"] == "qx":
        a.q = None
        a.qx, a.ldqx, a.wq, a.ldwq, a.bq, a.qc, a.ln_eps = 0x50000, 320, 0x60000, 320, 0x70000, 320, 1e-5
    elif c["variant"] == "v_rows":
        a.v_rows, a.ldvt = 1, width
    return a


# ---- tt_conv3x3: the shape of tests/test_error_bounds_gpu.py::test_conv3x3_patch_kernel, and one per other pixel tile / column count
CONV_SHAPES = [(4, 16, 28, 128, 64, 128), (2, 32, 56, 64, 0, 320), (2, 16, 32, 64, 64, 640)]       # (nimg, h, w, c0, c1, n)


def conv_args(shape, dtype):
    from this_and_that_vdm_amd._lib import TtConvArgs
    nimg, h, w, c0, c1, n = shape
    a = TtConvArgs()
    a.x0, a.c0, a.ld0, a.w, a.ldw = 0x10000, c0, c0, 0x20000, 9 * (c0 + c1)
    if c1:
        a.x1, a.c1, a.ld1 = 0x18000, c1, c1
    a.nimg, a.h, a.w_img, a.n, a.out, a.ldo, a.dtype = nimg, h, w, n, 0x30000, n, dtype
    return a


def grid(lib):
    out = dict(attention=[], conv=[])
    for split in (0, 1):
        lib.tt_gemm_set_f32_split(split)
        out["attention"] += [[split, c] + list(name_of(lib.tt_attention_kernel, attn_args(c))) for c in attention_grid()]
    lib.tt_gemm_set_f32_split(0)
    out["conv"] = [[list(s), dt] + list(name_of(lib.tt_conv3x3_kernel, conv_args(s, dt))) for s in CONV_SHAPES for dt in (BF16, F16)]
    return out


# ---- the cases the Python mirror of the dispatch used to get wrong (the test pins the expected names by hand)
def pins(lib):
    from this_and_that_vdm_amd import ops
    out = dict(f32_split=[ops.f32_split(), lib.tt_gemm_get_f32_split()])
    sq = census.linear(200704, 320, 320, residual=True, ld_res=320, rowvec=True, rowvec_rows=1, rowvec_mod=2, ld_rowvec=320, dtype=BF16)
    out["sq320_rowvec"] = name_of(lib.tt_gemm_kernel, census.to_args(sq))
    out["attn_v_rows_128"] = name_of(lib.tt_attention_kernel, attn_args(dict(dtype=BF16, head_dim=64, mask=0, variant="v_rows", lk=128)))
    lib.tt_gemm_set_f32_split(1)
    out["attn_split16"] = name_of(lib.tt_attention_kernel, attn_args(dict(dtype=F32, head_dim=64, mask=1, variant="plain", lk=64)))
    out["presplit_a"] = name_of(lib.tt_gemm_kernel, census.to_args(census.linear(3136, 1280, 1280, dtype=F32, presplit=1)))
    lib.tt_gemm_set_f32_split(0)
    small = (C.c_char * 8)()
    out["short_buffer"] = lib.tt_gemm_kernel(C.byref(census.to_args(sq)), small, len(small))
    return out


if __name__ == "__main__":
    lib = census.load_lib()
    what = {"census": lambda: census.take(lib, gemm_answers), "grid": lambda: grid(lib), "pins": lambda: pins(lib)}[sys.argv[1]]
    print(json.dumps(what(), separators=(",", ":")))
