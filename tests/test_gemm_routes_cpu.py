"""CPU: the route census of tt_gemm's planner (tests/gemm_route_census.py) against tests/golden/gemm_route_census.json.

Every problem of the census gets, from the library under test, the answers the fixture recorded from the commit before the five
planner entry points became readers of one route resolver (csrc/gemm.hip: wanted_route / granted_route) -- so "no route changed" is
checked, for ~32 500 (knob state, problem, workspace) rows.  The second test keeps the census from going vacuous: the recorded
answers must reach every route, the planner's own tile choices, the fall-backs and the refusal."""
import json
import os

import pytest

from tests import gemm_route_census as census

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_route_census.json")
# tt_gemm_plan's cfg[0..5] of the routes that are not the tiled template, and of the tiled template's tile table indices
PP, W320, W320H = (256, 256, 64, 0, 2, 4), (256, 320, 64, 0, 4, 2), (128, 320, 64, 0, 2, 2)
TILE16 = {1: (128, 64, 64, 3, 2, 2), 2: (64, 64, 64, 4, 2, 2), 3: (256, 128, 32, 3, 4, 2), 7: (128, 160, 64, 2, 4, 1),
          11: (128, 128, 64, 2, 4, 2), 16: (128, 128, 64, 4, 4, 2)}
TILE32 = {0: (128, 128, 32, 2, 2, 2), 1: (64, 64, 32, 4, 2, 2)}


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def _describe(row):
    st, p, with_ws = row
    return f"{st[0]}({st[1]}) ws={'asked' if with_ws else 'none'} {p}"


def test_every_census_row_keeps_its_recorded_answers(golden):
    rows = census.rows_of()
    assert census.sha_of(rows) == golden["sha"], "the census's problem list changed: regenerate the fixture (tests/golden/make_gemm_route_census.py)"
    got = census.run_child()
    assert got["sha"] == golden["sha"] and len(got["rows"]) == len(golden["rows"]) == len(rows)
    bad = [(i, golden["answers"][w], got["answers"][g]) for i, (w, g) in enumerate(zip(golden["rows"], got["rows"]))
           if golden["answers"][w] != got["answers"][g]]
    lines = [f"{_describe(rows[i])}\n    recorded {w}\n    now      {g}" for i, w, g in bad[:12]]
    assert not bad, f"{len(bad)} of {len(rows)} census rows changed their (rc, cfg[0..6], ws_bytes, stats_rows, gn_fused):\n" + "\n".join(lines)


def test_the_census_reaches_every_route(golden):
    rows = census.rows_of()
    assert len(rows) == len(golden["rows"])
    seen = set()
    plain = {}                                                          # default state: (problem, with_ws) -> answers
    for (st, p, with_ws), idx in zip(rows, golden["rows"]):
        rc, *rest = golden["answers"][idx]
        tile, splitk, ws, stats, gn = tuple(rest[:6]), rest[6], rest[7], rest[8], rest[9]
        default, f32 = st[0] == "default", p["dtype"] == census.F32
        if default:
            plain[(json.dumps(p, sort_keys=True), with_ws)] = (rc, tile, splitk)
        if rc == -2:
            seen.add("unsupported")
            continue
        assert rc == 0, _describe((st, p, with_ws))
        if tile == PP and default:
            # one launch or two: the persistent kernel's own bar on the WHOLE problem (pp_ok: >= 400 tiles at 75 % fill for GEGLU, 460 / 90 otherwise)
            tiles = -(-p["m"] // 256) * -(-p["n"] // 256)
            rounds = -(-tiles // 256)
            min_tiles, fill = (400, 75) if p.get("geglu") else (460, 90)
            seen.add("pp" if tiles >= min_tiles and tiles * 100 >= rounds * 256 * fill else "pp two-part")
        elif tile[:3] == (32, 320, 320):
            seen.add("sq320")
        elif tile == W320:
            seen.add("w320")
        elif tile == W320H:
            seen.add("w320h split-k" if splitk > 1 else "w320h")
        elif tile[3] > 0:                                               # the tiled template
            if default and not f32:
                seen.update(f"tiled cfg {c}" for c, t in TILE16.items() if t == tile)
            if f32:
                seen.update(f"f32 cfg {c}" for c, t in TILE32.items() if t == tile)
            if splitk > 1:
                seen.add("split16 split-k" if f32 and st[0] == "tt_gemm_set_f32_split" else ("tiled split-k" if not f32 else "f32 split-k?"))
            if splitk == 1 and ws > 0 and not with_ws:
                seen.add("split plan without its workspace")
            if stats and tile[1] != 320:
                seen.add("stats: whole tile" if stats == tile[0] else "stats: wave row" if stats == tile[0] // tile[4] else "stats: other")
        if stats and splitk > 1:
            seen.add("stats: split-k")
        if gn:
            seen.add("gn fused")
    # a mode-3 plan that mode3_plan remapped: its mode-1 twin (same shape, same tiles) plans a tile without the mode-3 gather
    for (key, with_ws), (rc, tile, splitk) in plain.items():
        p = json.loads(key)
        if p["mode"] == 3 and p["dtype"] != census.F32:
            twin = plain.get((json.dumps(dict(p, mode=1), sort_keys=True), with_ws))
            if twin and twin[1] != tile and twin[1] not in (TILE16[1], TILE16[2], TILE16[11], TILE16[16]):
                seen.add("mode 3 remapped")
    want = {"pp", "pp two-part", "sq320", "w320", "w320h", "w320h split-k", "tiled split-k", "split plan without its workspace",
            "f32 cfg 0", "f32 cfg 1", "split16 split-k", "mode 3 remapped", "unsupported", "stats: whole tile", "stats: wave row", "gn fused"}
    want |= {f"tiled cfg {c}" for c in TILE16}
    assert not want - seen, sorted(want - seen)
