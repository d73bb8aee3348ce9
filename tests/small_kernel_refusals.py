"""The refusals of the small kernels' entry points (csrc/elementwise.hip) that guard their vector accesses and 32-bit indices: one valid
argument set per entry point, ONE fault applied at a time, in the manner of tests/attention_refusals.py.  The operands are real host
buffers on 16-byte boundaries, the outputs filled with a pattern: a refusal returns before the first HIP call, so the pattern must still
be there.  A fully valid argument set is never passed, and the rows are answered by a child process that sees no GPU
(`python -m tests.small_kernel_refusals`): a row that were NOT refused would fail to launch there (TT_ELAUNCH) instead of reaching a device.

tests/test_small_kernel_refusals_cpu.py asserts, for every row: TT_EINVAL, the entry point's name in tt_last_error(), output untouched."""
import ctypes as C
import json
import os
import sys

TT_BF16, TT_F16, TT_F32 = 0, 1, 2
TT_EINVAL = -1
NBYTES = 4096
PATTERN = 0xA5
BIG = 1 << 16                 # BIG * BIG = 2^32: past a 32-bit pixel count

# entry point -> (argument names in the ABI's order, the valid set; "A" .. "D": host buffers, the LAST letter names the output)
ENTRIES = {
    "tt_add_rowvec": (("x", "ldx", "rows", "c", "rowvec", "ld_rowvec", "rows_per_vec", "nvec", "y", "ldy", "dtype"),
                      dict(x="A", ldx=16, rows=4, c=16, rowvec="B", ld_rowvec=16, rows_per_vec=2, nvec=2, y="D", ldy=16, dtype=TT_BF16)),
    "tt_add_scaled": (("a", "b", "scale", "y", "n", "dtype"), dict(a="A", b="B", scale=1.0, y="D", n=16, dtype=TT_BF16)),
    "tt_small_linear": (("x", "ldx", "rows", "k", "w", "ldw", "n", "bias", "act_in", "act_out", "accumulate", "y", "ldy", "dtype"),
                        dict(x="A", ldx=16, rows=2, k=16, w="B", ldw=16, n=2, bias=None, act_in=0, act_out=0, accumulate=0, y="D", ldy=2,
                             dtype=TT_BF16)),
    "tt_softmax_rows": (("x", "ldx", "rows", "cols", "y", "ldy", "cols_pad", "dtype"),
                        dict(x="A", ldx=8, rows=2, cols=5, y="D", ldy=8, cols_pad=8, dtype=TT_BF16)),
    "tt_timestep_embedding": (("t", "rows", "dim", "out", "ldo"), dict(t="A", rows=2, dim=8, out="D", ldo=8)),
    "tt_prep_model_input": (("latents", "image_latents", "cond", "sigmas", "step", "batch", "frames", "h", "w", "cpad", "x", "dtype"),
                            dict(latents="A", image_latents="B", cond=None, sigmas="C", step=0, batch=1, frames=1, h=2, w=2, cpad=8, x="D",
                                 dtype=TT_BF16)),
    "tt_cfg_euler_step": (("eps", "ld_eps", "latents", "guidance", "sigmas", "step", "batch", "frames", "h", "w"),
                          dict(eps="A", ld_eps=4, latents="D", guidance=None, sigmas="C", step=0, batch=1, frames=1, h=2, w=2)),
    "tt_cfg3_euler_step": (("eps", "ld_eps", "latents", "guidance", "image_guidance_scale", "sigmas", "step", "frames", "h", "w"),
                           dict(eps="A", ld_eps=4, latents="D", guidance="B", image_guidance_scale=7.5, sigmas="C", step=0, frames=1, h=2, w=2)),
}
# (entry point, fault): a string "X+n" is buffer X moved n bytes off its boundary
ROWS = [
    ("tt_add_rowvec", dict(x="A+2")), ("tt_add_rowvec", dict(y="D+2")), ("tt_add_rowvec", dict(rowvec="B+4")),
    ("tt_add_rowvec", dict(ldx=8)), ("tt_add_rowvec", dict(ldy=8)), ("tt_add_rowvec", dict(ld_rowvec=8)),
    ("tt_add_scaled", dict(a="A+2")), ("tt_add_scaled", dict(b="B+8")), ("tt_add_scaled", dict(y="D+2")),
    ("tt_small_linear", dict(x="A+4")), ("tt_small_linear", dict(w="B+2")), ("tt_small_linear", dict(ldx=8)), ("tt_small_linear", dict(ldw=8)),
    ("tt_small_linear", dict(ldy=1)),
    ("tt_softmax_rows", dict(x="A+4")), ("tt_softmax_rows", dict(y="D+2")), ("tt_softmax_rows", dict(y="D+8", dtype=TT_F32)),
    ("tt_timestep_embedding", dict(ldo=4)), ("tt_timestep_embedding", dict(rows=1 << 20, dim=1 << 13, ldo=1 << 13)),
    ("tt_prep_model_input", dict(h=0)), ("tt_prep_model_input", dict(w=-1)), ("tt_prep_model_input", dict(h=BIG, w=BIG)),
    ("tt_prep_model_input", dict(h=46341, w=46341)),
    ("tt_cfg_euler_step", dict(h=0)), ("tt_cfg_euler_step", dict(w=0)), ("tt_cfg_euler_step", dict(h=BIG, w=BIG)),
    ("tt_cfg3_euler_step", dict(w=0)), ("tt_cfg3_euler_step", dict(h=BIG, w=BIG)),
]


def row_id(entry, fault):
    return entry + ":" + ",".join(f"{k}={v}" for k, v in fault.items())


def take(lib):
    raw = {n: (C.c_ubyte * (NBYTES + 64))() for n in "ABCD"}
    base = {n: (C.addressof(b) + 15) // 16 * 16 for n, b in raw.items()}

    def value(v):
        if isinstance(v, str):
            name, _, off = v.partition("+")
            return base[name] + int(off or 0)
        return v

    out = {}
    for entry, fault in ROWS:
        assert fault, "a row without a fault would be a valid call"
        names, valid = ENTRIES[entry]
        args = dict(valid, **fault)
        C.memset(base["D"], PATTERN, NBYTES)
        code = getattr(lib, entry)(*[value(args[n]) for n in names], None)
        untouched = C.string_at(base["D"], NBYTES) == bytes([PATTERN]) * NBYTES
        out[row_id(entry, fault)] = [code, lib.tt_last_error().decode(), untouched]
    return out


def run_child():
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("TT_")}
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")           # the child sees no GPU
    r = subprocess.run([sys.executable, "-m", "tests.small_kernel_refusals"], cwd=root, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"small-kernel refusals failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(r.stdout.splitlines()[-1])


if __name__ == "__main__":
    from this_and_that_vdm_amd import _lib
    print(json.dumps(take(_lib.load()), separators=(",", ":")))
