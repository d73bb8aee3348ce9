"""GPU: tt_gif_decode_indices and tt_gif_compose (include/ttvdm.h, "GIF import") held to the restatement of
tests/gif_decode_reference.py byte for byte -- index maps, status words and composed frames -- on the frames where the kernels take
another path: code widths that change inside a tiny frame, a full table with and without a deferred clear, the longest self-naming
strings, a clear code before every pixel, empty segments, every interlace pass count, the 72 composition files (inside Pillow's
envelope also against Pillow), batches, streams, poison around every buffer, corrupt data on kernels that clamp, and the refusals
with real buffers.  Small shapes throughout: every test takes seconds."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import gif_decode_reference as g
from tests import gif_decode_refusals as refusals
from this_and_that_vdm_amd.ingest import decode_gif          # the feature under test: without it nothing here is collected

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def item(px, mcs, interlace=False, stream=None, **kw):
    """one image for ``run``: its indices [h, w] in raster order, coded as the writer codes them unless ``stream`` gives the bytes"""
    px = np.asarray(px, dtype=np.uint8)
    h, w = px.shape
    sent = px[g.interlace_rows(h)] if interlace else px
    return dict(w=w, h=h, interlace=interlace, min_code_size=mcs, data=g.lzw_stream(sent, mcs, **kw) if stream is None else stream, indices=px)


def run(items, offsets=None):
    """-> ([map [h, w] per image], [status per image]) from ops.gif_indices"""
    from this_and_that_vdm_amd import ops
    lens = [len(it["data"]) for it in items]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]) if offsets is None else np.asarray(offsets)
    npix = np.array([it["w"] * it["h"] for it in items])
    moffs = np.concatenate([[0], np.cumsum(npix)[:-1]])
    t = lambda a, dt: torch.from_numpy(np.asarray(a).astype(dt)).to(DEV)
    data = t(np.frombuffer(b"".join(it["data"] for it in items), dtype=np.uint8), np.uint8)
    maps, status = ops.gif_indices(data, t(offs, np.int64), t(lens, np.int32), t(npix, np.int32), t([it["min_code_size"] for it in items], np.int32),
                                   t([it["h"] if it["interlace"] else 0 for it in items], np.int32), t(moffs, np.int64), int(npix.sum()))
    maps = maps.cpu().numpy()
    return [maps[o:o + n].reshape(it["h"], it["w"]) for o, n, it in zip(moffs, npix, items)], status.cpu().tolist()


def want(it):
    return g.index_map(it)


def check(items):
    maps, status = run(items)
    for i, it in enumerate(items):
        ref, st = want(it)
        assert status[i] == st and np.array_equal(maps[i], ref), (i, it["w"], it["h"], it["min_code_size"], status[i], st)
    return maps, status


def test_tiny_frames_at_three_code_sizes():
    rng = np.random.default_rng(1)
    items = [item(rng.integers(0, 1 << mcs, size=(h, w)), mcs) for mcs in (2, 5, 8) for h, w in ((1, 1), (7, 1), (5, 3), (13, 17))]
    widths = {min(12, (4 + 1 + r).bit_length()) for _, r, _ in g.read_codes(items[2]["data"], 2)}
    assert len(widths) >= 3, "the 3 x 5 frame at size 2 no longer changes its code width several times"
    maps, status = check(items)
    assert status == [0] * 12 and all(np.array_equal(m, it["indices"]) for m, it in zip(maps, items))


def test_a_full_table_with_a_clear_and_with_a_deferred_clear():
    px = np.random.default_rng(2).integers(0, 256, size=(96, 96))
    plain, deferred = item(px, 8), item(px, 8, deferred=True)
    assert sum(c == 256 for c, _, _ in g.read_codes(plain["data"], 8)) == 3 and sum(c == 256 for c, _, _ in g.read_codes(deferred["data"], 8)) == 1
    assert max(r for _, r, _ in g.read_codes(deferred["data"], 8)) > 4096
    maps, status = check([plain, deferred])
    assert status == [0, 0] and np.array_equal(maps[0], px) and np.array_equal(maps[1], px)


def test_the_longest_self_naming_strings():
    constant = np.full((64, 64), 5)
    checker = (np.add.outer(np.arange(64), np.arange(64)) % 2) * 3
    items = [item(constant, 3), item(checker, 2), item(constant, 8)]
    codes = g.read_codes(items[0]["data"], 3)
    assert sum(1 for c, r, _ in codes if r >= 1 and c == 8 + 2 + r - 1) > 80, "the constant frame's codes no longer name the entry being made"
    maps, status = check(items)
    assert status == [0, 0, 0] and np.array_equal(maps[0], constant) and np.array_equal(maps[1], checker)


@pytest.mark.parametrize("segment", [1, 7, 64])
def test_files_of_the_device_coder_with_a_clear_before_every_few_pixels(segment, tmp_path):
    from this_and_that_vdm_amd import export, ingest
    video = np.random.default_rng(3).integers(0, 256, size=(2, 5, 3, 3)).astype(np.uint8)
    path = str(tmp_path / "v.gif")
    q = export.write_gif(torch.from_numpy(video).to(DEV), path, lzw="device", segment=segment)
    hd = g.parse(open(path, "rb").read())
    clears = sum(c == (1 << hd["frames"][0]["min_code_size"]) for c, _, _ in g.read_codes(hd["frames"][0]["data"], hd["frames"][0]["min_code_size"]))
    assert clears == -(-15 // segment)
    got = ingest.read_gif(path, DEV).cpu().numpy()
    which = np.arange(2) if q.palettes.shape[0] == 2 else np.zeros(2, dtype=int)
    assert np.array_equal(got, np.stack([q.palettes[which[i]][q.indices[i]] for i in range(2)]))
    assert np.array_equal(got, g.decode(open(path, "rb").read())[0])


def test_three_clear_codes_in_a_row_and_none_at_the_start():
    # min code size 2: clear 4, end 5, first entry 6.  1 2 | | | 3 0 6 (= "3 0") 1 end: no clear code first, three in a row, an entry named
    codes = [1, 2, 4, 4, 4, 3, 0, 6, 1, 5]
    it = dict(w=7, h=1, interlace=False, min_code_size=2, data=g.pack(codes, 2))
    ref, st = want(it)
    assert st == 0 and ref.tolist() == [[1, 2, 3, 0, 3, 0, 1]]
    check([it])


def test_interlaced_frames_of_every_pass_count():
    rng = np.random.default_rng(4)
    items = [item(rng.integers(0, 32, size=(h, 6 + h % 3)), 5, interlace=True) for h in (1, 2, 3, 4, 5, 8, 9, 17)]
    maps, status = check(items)
    assert status == [0] * 8 and all(np.array_equal(m, it["indices"]) for m, it in zip(maps, items))


@functools.lru_cache(maxsize=None)
def composition_references():
    """-> [(name, bytes, the restatement's frames, inside Pillow's envelope)], computed once"""
    return [(name, data, g.decode(data)[0], not g.outside_pillows_envelope(g.parse(data))) for name, data in g.handcrafted_files()]


def test_the_72_composition_files():
    from this_and_that_vdm_amd import ingest
    inside = 0
    for name, data, ref, in_envelope in composition_references():
        got = ingest.decode_gif(data, DEV).cpu().numpy()
        assert got.shape == ref.shape and np.array_equal(got, ref), name
        if in_envelope:
            inside += 1
            assert np.array_equal(got, g.pillow_frames(data)), name
    assert inside >= 64


@pytest.mark.parametrize("transparent", [-1, 2])
def test_a_first_frame_smaller_than_the_screen(transparent):
    from this_and_that_vdm_amd import ingest
    rng = np.random.default_rng(6)
    table = rng.integers(0, 256, size=(8, 3))
    frames = [dict(indices=rng.integers(0, 8, size=(5, 9)), left=4, top=3, transparent=transparent, disposal=1),
              dict(indices=rng.integers(0, 8, size=(11, 6)), left=0, top=2, transparent=transparent, disposal=1)]
    data = g.gif_file(20, 14, frames, global_table=table, background=3)
    got, hd = ingest.decode_gif(data, DEV, info=True)
    assert (hd.height, hd.width, hd.frames, hd.loop, hd.durations) == (14, 20, 2, 0, [0.05, 0.05])
    ref = g.decode(data)[0]
    assert np.array_equal(got.cpu().numpy(), ref) and np.array_equal(ref, g.pillow_frames(data))
    assert ref[0, 0, 0].tolist() == table[max(transparent, 0)].tolist()                                   # the canvas before frame 0


def batch_items():
    rng = np.random.default_rng(7)
    return [item(rng.integers(0, 256, size=(40, 50)), 8), item(np.full((33, 9), 2), 2), item(rng.integers(0, 16, size=(17, 23)), 4, interlace=True),
            item(rng.integers(0, 4, size=(1, 300)), 2), item(rng.integers(0, 256, size=(70, 70)), 8, deferred=True)]


def test_every_frame_of_a_batch_equals_what_it_gets_alone():
    items = batch_items()
    maps, status = check(items)
    for i, it in enumerate(items):
        alone, st = run([it])
        assert st == [status[i]] and np.array_equal(alone[0], maps[i]), i


def test_a_second_call_and_another_stream_give_the_same_bytes():
    from this_and_that_vdm_amd import ingest
    items = batch_items()
    first = run(items)
    again = run(items)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        other = run(items)
        frames_side = ingest.decode_gif(composition_references()[5][1], DEV).cpu().numpy()
    side.synchronize()
    for a, b, c in zip(first[0], again[0], other[0]):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert first[1] == again[1] == other[1]
    assert np.array_equal(frames_side, composition_references()[5][2])


POISON = 0xA7


def test_poison_around_every_buffer_stays():
    from this_and_that_vdm_amd import _lib
    lib = _lib.load()
    items = batch_items()
    lens = np.array([len(it["data"]) for it in items])
    npix = np.array([it["w"] * it["h"] for it in items])
    n, data_bytes, maps_bytes = len(items), int(lens.sum()), int(npix.sum())
    ws_bytes = lib.tt_gif_decode_ws_bytes(n, data_bytes)
    guard = 4096
    up = lambda v: -(-v // 16) * 16
    sizes = [up(maps_bytes), up(4 * n), up(ws_bytes), up(n * 13 * 11 * 3)]
    arena = torch.full((sum(sizes) + guard * (len(sizes) + 1),), POISON, dtype=torch.uint8, device=DEV)
    at, parts = guard, []
    for s in sizes:
        parts.append(arena[at:at + s])
        at += s + guard
    maps, status, ws, out = parts
    t = lambda a, dt: torch.from_numpy(np.asarray(a).astype(dt)).to(DEV)
    data = t(np.frombuffer(b"".join(it["data"] for it in items), dtype=np.uint8), np.uint8)
    offs, moffs = np.concatenate([[0], np.cumsum(lens)[:-1]]), np.concatenate([[0], np.cumsum(npix)[:-1]])
    args = [t(offs, np.int64), t(lens, np.int32), t(npix, np.int32), t([it["min_code_size"] for it in items], np.int32),
            t([it["h"] if it["interlace"] else 0 for it in items], np.int32), t(moffs, np.int64)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.tt_gif_decode_indices(data.data_ptr(), data_bytes, *[a.data_ptr() for a in args], n, maps.data_ptr(), maps_bytes, status.data_ptr(), ws.data_ptr(),
                                     ws_bytes, stream) == 0, lib.tt_last_error()
    # five frames drawn onto a 13 x 11 canvas from the first bytes of the maps
    table = (_lib.TtGifComposeFrame * n)(*[_lib.TtGifComposeFrame(i, i, 6, 5, -1, i % 4, 0x112233, 0, 30 * i) for i in range(n)])
    tab = t(np.frombuffer(table, dtype=np.uint8), np.uint8)
    pal = t(np.random.default_rng(8).integers(0, 256, size=(n, 256, 3)), np.uint8)
    assert lib.tt_gif_compose(maps.data_ptr(), maps_bytes, tab.data_ptr(), pal.data_ptr(), n, 11, 13, 0x445566, out.data_ptr(), stream) == 0, lib.tt_last_error()
    host = arena.cpu().numpy()
    used = np.zeros(host.size, dtype=bool)
    at = guard
    for s, real in zip(sizes, (maps_bytes, 4 * n, ws_bytes, n * 13 * 11 * 3)):
        used[at:at + real] = True
        at += s + guard
    assert (host[~used] == POISON).all(), "bytes outside the index maps, status, the workspace or the output changed"
    got_maps = host[guard:guard + maps_bytes]
    for it, o, c in zip(items, moffs, npix):
        assert np.array_equal(got_maps[o:o + c].reshape(it["h"], it["w"]), want(it)[0])
    assert (host[used][maps_bytes:maps_bytes + 4 * n] == 0).all()                                           # every status word is 0
    assert (host[-guard - up(n * 13 * 11 * 3):][:n * 13 * 11 * 3] != POISON).any()


def test_corrupt_data_marks_its_own_frame_alone():
    rng = np.random.default_rng(9)
    good = item(rng.integers(0, 4, size=(6, 10)), 2)
    # the codes of 90 pixels for a rectangle of 60, so that a code read as one pixel leaves the frame complete.  Min code size 2: the code
    # at place 3 is 4 bits wide and may name the entries 6, 7, 8: 12 lies above the next entry; the code at place 0 may name none
    codes = g.lzw_codes(rng.integers(0, 4, size=90), 2)
    assert codes[0] == 4 and 4 not in codes[1:]
    above = dict(w=10, h=6, interlace=False, min_code_size=2, data=g.pack(codes[:4] + [12] + codes[5:], 2))
    first = dict(w=10, h=6, interlace=False, min_code_size=2, data=g.pack(codes[:1] + [6] + codes[2:], 2))
    whole = item(rng.integers(0, 256, size=(30, 30)), 8)
    cut = dict(whole, data=whole["data"][:len(whole["data"]) // 2])
    surplus = dict(item(rng.integers(0, 16, size=(1, 160)), 4), w=10, h=6)                                   # 160 pixels for a 10 x 6 rectangle
    items = [good, above, good, first, good, cut, good, surplus, good]
    maps, status = check(items)
    assert status == [0, g.STATUS_CODE, 0, g.STATUS_CODE, 0, g.STATUS_SHORT, 0, 0, 0]
    assert maps[3][0, 0] == 0                                                                              # an invalid code reads as pixel 0
    assert np.array_equal(maps[7], surplus["indices"].reshape(-1)[:60].reshape(6, 10))
    for i in (0, 2, 4, 6, 8):
        assert np.array_equal(maps[i], good["indices"])
    # a span outside the uploaded bytes: the frame is empty, marked, and its neighbours decode
    lens = [len(it["data"]) for it in (good, whole, good)]
    maps, status = run([good, whole, good], offsets=[0, lens[0] + lens[2] + 1, lens[0] + lens[1]])     # frame 1 ends one byte behind the data
    assert status == [0, g.STATUS_SPAN, 0] and not maps[1].any() and np.array_equal(maps[0], good["indices"]) and np.array_equal(maps[2], good["indices"])


def test_decode_gif_names_the_corrupt_frame_and_the_cause():
    rng = np.random.default_rng(10)
    table = rng.integers(0, 256, size=(16, 3))
    px = [rng.integers(0, 16, size=(9, 12)) for _ in range(3)]
    whole = g.lzw_stream(px[1], 4)
    codes = g.lzw_codes(px[2], 4)
    files = {"short": dict(indices=px[1], stream=whole[:len(whole) // 2]), "code": dict(indices=px[2], stream=g.pack(codes[:1] + [18] + codes[2:], 4)),
             "empty": dict(indices=px[1], stream=b"")}
    texts = {"short": r"decode_gif: frame 1 is corrupt or short \(fewer pixels than the rectangle holds; status 2\)",
             "code": r"decode_gif: frame 1 is corrupt or short \(an invalid LZW code.*status [13]\)",
             "empty": r"decode_gif: frame 1 is corrupt or short \(fewer pixels than the rectangle holds; status 2\)"}
    for name, bad in files.items():
        data = g.gif_file(12, 9, [dict(indices=px[0]), bad, dict(indices=px[2])], global_table=table)
        assert g.decode(data)[1][0] == 0 and g.decode(data)[1][1] != 0 and g.decode(data)[1][2] == 0
        with pytest.raises(ValueError, match=texts[name]):
            decode_gif(data, DEV)
    good = g.gif_file(12, 9, [dict(indices=p) for p in px], global_table=table)
    assert np.array_equal(decode_gif(good, DEV).cpu().numpy(), g.decode(good)[0])


def test_refusal_rows_with_real_buffers_leave_them_untouched():
    from this_and_that_vdm_amd import _lib
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bufs = {k: torch.full((8192,), POISON, dtype=torch.uint8, device=DEV) for k in ("data", "offsets", "lengths", "npix", "mcs", "rows", "map_offsets", "maps", "status")}
    bufs["ws"] = torch.full((max(lib.tt_gif_decode_ws_bytes(3, 1000), 16) + 16,), POISON, dtype=torch.uint8, device=DEV)
    real = dict(refusals.DEC, **{k: v.data_ptr() for k, v in bufs.items()}, ws_bytes=bufs["ws"].numel() - 16)
    for fault, code, fragment in refusals.DEC_ROWS:
        moved = {k: (real[k] + (v - refusals.DEC[k]) if isinstance(v, int) and k in bufs else v) for k, v in fault.items()}
        rc, msg = refusals.dec_call(lib, dict(real, **moved), stream)
        assert rc == code and fragment in msg, (fault, rc, msg)
    cbufs = {k: torch.full((8192,), POISON, dtype=torch.uint8, device=DEV) for k in ("maps", "table", "palettes", "out")}
    creal = dict(refusals.CMP, **{k: v.data_ptr() for k, v in cbufs.items()})
    for fault, code, fragment in refusals.CMP_ROWS:
        moved = {k: (creal[k] + (v - refusals.CMP[k]) if isinstance(v, int) and k in cbufs else v) for k, v in fault.items()}
        rc, msg = refusals.cmp_call(lib, dict(creal, **moved), stream)
        assert rc == code and fragment in msg, (fault, rc, msg)
    torch.cuda.synchronize()
    for v in list(bufs.values()) + list(cbufs.values()):
        assert bool((v == POISON).all())
