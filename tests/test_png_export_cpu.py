"""CPU: the format and the host half of the PNG export.  The restatement of tests/png_reference.py writes files that Pillow (an
independent decoder) reads back to the exact pixels, whose IDAT zlib inflates -- checking the Adler-32 -- to the restated filtered
bytes and whose chunk CRCs are right; tt_png_code_lengths against the restatement's own package-merge in cost, with the Kraft sum and
the limit; tt_png_block_header against the restatement bit for bit; tt_png_plan against both; the restatement's file sizes against
Pillow's; the refusals of the three device entry points (in a child process that sees no GPU); and png_host.cpp under the address and
undefined-behaviour sanitizers in a stand-alone program.

The size bound, 1.02 x Pillow's ``save(format="PNG")`` on the committed generator's frames, is a margin over ratios measured on a CPU
prototype of the format (0.995 - 0.999); it is held HERE, on the restatement, and the GPU tests hold the library to the restatement's
bytes."""
import io
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from tests import png_reference as ref
from tests import png_refusals as refusals

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}


@pytest.fixture(scope="module")
def lib():
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _lib_lengths(counts, limit):
    from this_and_that_vdm_amd import export
    return export.png_code_lengths(counts, limit)


def _decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    a = np.asarray(im)
    return im, a if a.ndim == 3 else a[..., None]


def _rand(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.int64).astype(np.uint8)


FILE_CASES = {
    "the generator, 64 x 96": (ref.generator_frame(64, 96), 5),
    "grey, odd sizes": (ref.generator_frame(9, 97, 1, ch=1), 5),
    "grey + alpha": (ref.generator_frame(9, 97, 2, ch=2), 5),
    "RGBA": (ref.generator_frame(9, 97, 3, ch=4), 5),
    "one pixel": (_rand((1, 1, 3), 1), 5),
    "one row": (_rand((1, 7, 3), 2), 5),
    "one column": (_rand((5, 1, 3), 3), 5),
    "uniform noise, two stripes": (_rand((96, 128, 3), 4), 5),
    "a flat frame": (np.full((64, 96, 3), 77, dtype=np.uint8), 5),
    **{f"filter {k}": (ref.generator_frame(24, 31, 4), k) for k in range(5)},
}


@pytest.mark.parametrize("name", list(FILE_CASES))
def test_the_restatements_files_decode_to_the_exact_pixels(name):
    frame, kind = FILE_CASES[name]
    data = ref.png_file(frame, kind)
    im, back = _decode(data)
    assert im.mode == MODES[frame.shape[2]] and im.size == (frame.shape[1], frame.shape[0]) and np.array_equal(back, frame)
    chunks = ref.chunks_of(data)
    assert [c[0] for c in chunks] == [b"IHDR", b"IDAT", b"IEND"] and all(c[2] for c in chunks)
    stream, types = ref.filter_frame(frame, kind)
    assert zlib.decompress(chunks[1][1]) == stream.tobytes()               # zlib checks the stream's Adler-32
    assert kind == 5 or set(types) == {kind}
    parts = ref.stripes_of(stream)
    assert ref.adler_combine([ref.adler_pair(p) for p in parts], [len(p) for p in parts]) == zlib.adler32(stream.tobytes())


def test_adaptive_uses_several_types_and_a_tie_goes_to_the_lowest():
    _, types = ref.filter_frame(ref.generator_frame(64, 96), 5)
    assert len(set(types)) >= 2
    _, types = ref.filter_frame(np.zeros((3, 5, 3), dtype=np.uint8), 5)    # every type costs 0
    assert types == [0, 0, 0]


# ---- code lengths
def _fibonacci(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


def _count_cases():
    rng = np.random.default_rng(21)
    cases = {}
    for i in range(6):
        c = rng.integers(0, 1 << rng.integers(1, 16), size=286) * (rng.random(286) < rng.choice([0.1, 0.5, 1.0]))
        c[256] = 1
        cases[f"random {i}"] = (c.astype(np.int64), 15)
    for i in range(4):
        c = rng.integers(0, 1 << rng.integers(1, 12), size=19) * (rng.random(19) < 0.8)
        c[rng.integers(19)] += 1
        cases[f"random code-length counts {i}"] = (c.astype(np.int64), 7)
    one = np.zeros(286, dtype=np.int64)
    one[97] = 5
    cases["a single symbol"] = (one, 15)
    cases["all 286 equal"] = (np.full(286, 7, dtype=np.int64), 15)
    cases["all 19 equal"] = (np.full(19, 3, dtype=np.int64), 7)
    fib = np.zeros(286, dtype=np.int64)
    fib[:21] = _fibonacci(21)                                              # unlimited Huffman depth: 20
    cases["fibonacci, 21 symbols"] = (fib, 15)
    cases["fibonacci, 12 symbols, limit 7"] = (np.array(_fibonacci(12) + [0] * 7, dtype=np.int64), 7)
    return cases


COUNT_CASES = _count_cases()


@pytest.mark.parametrize("name", list(COUNT_CASES))
def test_code_lengths_are_optimal_within_the_limit(lib, name):
    counts, limit = COUNT_CASES[name]
    got = _lib_lengths(counts, limit)
    want = ref.package_merge(counts, limit)
    used = int((counts > 0).sum())
    assert np.array_equal(got > 0, counts > 0) and int(got.max()) <= limit
    assert ref.cost(counts, got) == ref.cost(counts, want)
    if used >= 2:
        assert ref.kraft(got, limit) == 1 << limit
    else:
        assert got[counts > 0].tolist() == [1]
    if name.startswith("fibonacci, 21"):
        assert int(got.max()) == 15 and int(ref.package_merge(counts, 32).max()) == 20     # the limit binds


# ---- the block header
def _header_cases():
    rng = np.random.default_rng(22)

    def from_counts(c):
        c = np.asarray(c, dtype=np.int64).copy()
        c[256] = 1
        return c, _lib_lengths(c, 15)

    sparse = np.zeros(286, dtype=np.int64)
    sparse[[0, 150]] = [40, 9]                                             # zeros of 149 = 138 + 11, then 105
    hand = np.zeros(286, dtype=np.uint8)
    hand[0:7], hand[20:28], hand[256] = 8, 9, 2                            # a run of 7: v, 16 x 6; a run of 8: v, 16 x 6, v
    noise = rng.integers(1, 200, size=286)
    noise[257:] = 0
    return {
        "HLIT 257, zero runs of 138 and 11": from_counts(sparse),
        "repeats of 6 and 7": ((hand > 0).astype(np.int64), hand),
        "all 286 equal": from_counts(np.full(286, 5)),
        "256 literals, no match": from_counts(noise),
        "random": from_counts(rng.integers(0, 3000, size=286) * (rng.random(286) < 0.6)),
        "fibonacci": from_counts(np.concatenate([_fibonacci(21), np.zeros(265, dtype=np.int64)])),
    }


@pytest.mark.parametrize("name", ["HLIT 257, zero runs of 138 and 11", "repeats of 6 and 7", "all 286 equal", "256 literals, no match", "random",
                                  "fibonacci"])
def test_block_header_equals_the_restatement_bit_for_bit(lib, name):
    from this_and_that_vdm_amd import export
    counts, lengths = _header_cases()[name]
    hlit, toks = ref.cl_tokens(lengths)
    if name.startswith("HLIT 257"):
        assert hlit == 257 and (18, 7, 127) in toks and (18, 7, 0) in toks
    if name.startswith("repeats"):
        assert toks[:6] == [(8, 0, 0), (16, 2, 3), (18, 7, 2), (9, 0, 0), (16, 2, 3), (9, 0, 0)], toks[:10]
    cl_lengths = _lib_lengths(ref.cl_counts(lengths), 7)
    want = ref.header_bits(lengths, cl_lengths).array()
    got, stripe_bits = export.png_block_header(counts, lengths)
    assert got.size == want.size and np.array_equal(got, want)
    extra = sum(int(counts[s]) * (ref.LENGTH_EXTRA[s - 257] + 1) for s in range(257, 286))
    assert stripe_bits == want.size + ref.cost(counts, lengths) + extra + 3


def test_block_header_refusals(lib):
    from this_and_that_vdm_amd import export
    counts = np.zeros(286, dtype=np.int64)
    counts[[5, 256]] = [3, 1]
    good = _lib_lengths(counts, 15)
    for lengths, fragment in ((np.where(np.arange(286) == 5, 16, good), "lengths\\[5\\] = 16"), (np.where(np.arange(286) == 5, 0, good), "symbol 5 is used"),
                              (np.where(np.arange(286) == 256, 0, good), "symbol 256 is used"), (np.full(286, 1), "Kraft sum exceeds 1")):
        with pytest.raises(RuntimeError, match=fragment):
            export.png_block_header(counts, lengths)
    words = np.zeros(80, dtype=np.uint32)
    import ctypes
    bits = ctypes.c_int64(0)
    c32, l8 = counts.astype(np.uint32), good.astype(np.uint8)
    assert lib.tt_png_block_header(c32.ctypes.data, l8.ctypes.data, words.ctypes.data, 71, ctypes.byref(bits)) == refusals.EINVAL
    assert b"cap too small" in lib.tt_last_error()
    assert lib.tt_png_block_header(None, l8.ctypes.data, words.ctypes.data, 72, ctypes.byref(bits)) == refusals.EINVAL
    assert b"null counts" in lib.tt_last_error()


def test_plan_gives_the_restatements_sizes_and_codes(lib):
    from this_and_that_vdm_amd import export
    stream, _ = ref.filter_frame(np.concatenate([ref.generator_frame(64, 96), _rand((64, 96, 3), 9)], 0), 5)
    parts = ref.stripes_of(stream)
    assert len(parts) == 2
    records = np.stack([ref.record_of(p) for p in parts]).astype(np.uint32)
    tables, headers, total = export.png_plan(records)
    tables, headers = tables.view(np.uint32), headers.view(np.uint32)
    sizes = [len(ref.stripe_bytes(p, _lib_lengths)) for p in parts]
    assert total == sum(sizes) and tables[:, 286].tolist() == [0, sizes[0]] and not tables[:, 287].any()
    for k, p in enumerate(parts):
        lengths = _lib_lengths(records[k, :286], 15)
        codes = ref.canonical(lengths)
        for s in range(286):
            width = int(lengths[s])
            rev = int(format(codes[s], f"0{width}b")[::-1], 2) if width else 0
            assert tables[k, s] == (width << 16 | rev), (k, s)
        bits, _ = export.png_block_header(records[k, :286], lengths)
        assert headers[k, 0] == bits.size
        assert np.array_equal(np.unpackbits(headers[k, 1:].view(np.uint8), bitorder="little")[:bits.size], bits)


# ---- sizes, on the restatement
@pytest.mark.parametrize("h,w", [(64, 96), (256, 384)])
def test_the_formats_files_are_no_larger_than_pillows(h, w):
    from PIL import Image
    frame = ref.generator_frame(h, w)
    mine = ref.png_file(frame, 5)
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="PNG")
    print(f"{h} x {w}: {len(mine)} bytes against Pillow's {len(buf.getvalue())}: {len(mine) / len(buf.getvalue()):.4f}")
    assert np.array_equal(_decode(mine)[1], frame)
    assert len(mine) <= 1.02 * len(buf.getvalue())


def test_a_flat_frame_is_a_few_hundred_bytes():
    from PIL import Image
    frame = np.full((64, 96, 3), 77, dtype=np.uint8)
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="PNG")
    assert len(ref.png_file(frame, 5)) <= 1.02 * len(buf.getvalue())


# ---- refusals
def test_every_refusal_of_the_device_entry_points_precedes_the_device():
    got = refusals.run_child()
    for family, (entry, _, _, rows) in refusals.FAMILIES.items():
        for fault, code, fragment in rows:
            rc, msg = got[refusals.row_id(family, fault)]
            assert rc == code and fragment in msg and msg.startswith(entry + ":"), (family, fault, rc, msg)


def test_encode_png_refuses_before_it_touches_a_device():
    from this_and_that_vdm_amd import export
    rgb = np.zeros((2, 8, 8, 3), dtype=np.uint8)
    for frames, kw, fragment in ((np.zeros((2, 2, 8, 8, 3), dtype=np.uint8), {}, "one video per file"), (rgb, dict(filter="best"), "filter"),
                                 (rgb, dict(filter=6), "filter"), (rgb.astype(np.int32), {}, "uint8 or floating-point"), ([], {}, "empty list"),
                                 (np.zeros((2, 8, 8, 5), dtype=np.uint8), {}, "1 to 4 channels")):
        with pytest.raises(ValueError, match=fragment):
            export.encode_png(frames, **kw)
    with pytest.raises(ValueError, match="loop"):
        export.write_apng(rgb, io.BytesIO(), loop=-1)


# ---- the host code under the sanitizers, on its own
def test_png_host_under_address_and_undefined_sanitizers(tmp_path):
    """png_host.cpp, lib.cpp (tt_set_error) and tests/png_host_check.cpp (its own main) built with the host compiler and run as a child
    process: nothing is preloaded and nothing of it runs under Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(REPO, "this_and_that_vdm_amd", "csrc")
    exe = str(tmp_path / "png_host_check")
    # the runtimes are linked INTO the program (clang's default; gcc needs the two flags)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static, "-I",
           os.path.join(REPO, "include"), "-I", csrc, os.path.join(REPO, "tests", "png_host_check.cpp"), os.path.join(csrc, "png_host.cpp"),
           os.path.join(csrc, "lib.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr):
        pytest.skip("the compiler's sanitizer runtime is missing: " + built.stderr[-300:])
    assert built.returncode == 0, built.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
