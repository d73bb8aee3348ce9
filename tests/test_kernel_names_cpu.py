"""CPU: the kernel instance names the library reports (tt_gemm_kernel / tt_conv3x3_kernel / tt_attention_kernel: what ops.PROFILE
records) are names of kernels the library holds, agree with the plan of the same problem, and are right where the Python mirror of
the dispatch they replace was wrong.  The queries run in child processes (tests/kernel_names.py): the library reads its knobs from
the environment once per process."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

from tests import gemm_route_census as census
from tests import kernel_names as kn
from tests.test_gemm_routes_cpu import PP, W320, W320H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = {kn.BF16: "bf16_tag", kn.F16: "f16_tag", kn.F32: "f32_tag"}


def child(what, **env):
    r = subprocess.run([sys.executable, "-m", "tests.kernel_names", what], cwd=ROOT, env=dict(census.clean_env(), **env),
                       capture_output=True, text=True)
    assert r.returncode == 0, f"tests.kernel_names {what} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return json.loads(r.stdout.splitlines()[-1])


def strip_symbol(sym):
    """demangled kernel symbol -> the form the library reports: no return type, no parameter list, no namespace qualifiers"""
    sym = sym.strip()
    depth = 0
    for i in range(len(sym) - 1, -1, -1):             # the parameter list: the last top-level (...) group
        depth += sym[i] == ")"
        depth -= sym[i] == "("
        if depth == 0:
            sym = sym[:i]
            break
    sym = re.sub(r"^void\s+", "", sym)
    return re.sub(r"(\(anonymous namespace\)|\w+)::", "", sym)


@pytest.fixture(scope="module")
def symbols():
    """the kernels of the loaded library, by stripped name"""
    from this_and_that_vdm_amd import _lib
    census.load_lib()                                  # (builds the library if it is missing)
    lib_path = _lib.LIB_PATH
    readelf = "/opt/rocm/llvm/bin/llvm-readelf"
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-C", lib_path], capture_output=True, text=True, check=True).stdout
        syms = [ln.split(None, 2)[2] for ln in out.splitlines() if len(ln.split(None, 2)) == 3]
    elif os.path.exists(readelf):
        out = subprocess.run([readelf, "-sW", "--demangle", lib_path], capture_output=True, text=True, check=True).stdout
        syms = [ln.split(None, 7)[7] for ln in out.splitlines() if len(ln.split(None, 7)) == 8]
    else:
        pytest.skip("no symbol lister (nm, llvm-readelf)")
    kernels = {strip_symbol(s) for s in syms if s.startswith("void ") and "__device_stub__" not in s and re.search(r"_kernel[<(]", s)}
    assert len(kernels) > 400 and "sq320_kernel<bf16_tag, true, true>" in kernels, len(kernels)
    return kernels


def test_strip_symbol():
    assert strip_symbol("void ttg::gemm_kernel<f32_tag, 64, 64, 32, 4, 2, 2, 44>(ttg::GemmP)") == "gemm_kernel<f32_tag, 64, 64, 32, 4, 2, 2, 44>"
    assert strip_symbol("void (anonymous namespace)::attn_kernel<bf16_tag, 64, 0, false, true, false>((anonymous namespace)::AttnP)") == \
        "attn_kernel<bf16_tag, 64, 0, false, true, false>"
    assert strip_symbol("void (anonymous namespace)::tattn_kernel<f16_tag, 64, 16>(char const*, long, char*, long, int, int, int, int, float)") == \
        "tattn_kernel<f16_tag, 64, 16>"


def test_every_census_row_names_a_built_kernel_that_agrees_with_its_plan(symbols):
    rows = census.rows_of()
    got = child("census")
    assert got["sha"] == census.sha_of(rows) and len(got["rows"]) == len(rows) > 30000
    families, refused = set(), 0
    for (st, p, with_ws), idx in zip(rows, got["rows"]):
        plan_rc, *tile, wide, rc, name = got["answers"][idx]
        tile, where = tuple(tile), f"{st[0]}({st[1]}) ws={with_ws} {p} -> {got['answers'][idx]}"
        assert rc == plan_rc, where
        if rc != 0:
            refused += 1
            continue
        assert name in symbols, where
        family, args = name.split("<", 1)
        args = args[:-1].split(", ")
        assert args[0] == TAGS[p["dtype"]], where
        families.add(family)
        # the kernels that are not the tiled template sit exactly on the tiles test_gemm_routes_cpu.py names
        assert (family == "gemm_pp_kernel") == (tile == PP), where
        assert (family == "gemm_w320_kernel") == (tile == W320), where
        assert (family == "gemm_w320h_kernel") == (tile == W320H), where
        assert (family == "sq320_kernel") == (tile[:3] == (32, 320, 320)), where
        if family == "gemm_kernel":
            assert tuple(int(v) for v in args[1:7]) == tile and tile[3] > 0, where
            kmode = int(args[7])
            assert bool(kmode & 64) == bool(wide), where
            assert bool(kmode & 8) == (p["dtype"] == kn.F32 and st[0] == "tt_gemm_set_f32_split"), where
    assert families == {"gemm_kernel", "gemm_pp_kernel", "gemm_w320_kernel", "gemm_w320h_kernel", "sq320_kernel"} and refused > 0


@pytest.mark.parametrize("conv_bn", [None, "160"])
def test_attention_and_conv3x3_name_built_kernels(symbols, conv_bn):
    got = child("grid", **({"TT_CONV_BN": conv_bn} if conv_bn else {}))
    served = 0
    for split, c, rc, name in got["attention"]:
        assert (rc == 0) == kn.attn_accepted(c), (split, c, rc, name)
        if rc == 0:
            served += 1
            assert name in symbols and name.split("<")[1].startswith(TAGS[c["dtype"]]), (split, c, name)
            want = "attn8_kernel" if c["variant"] == "fp8" else \
                ("attn_pipe_kernel" if c["variant"] == "v_rows" and c["lk"] in (128, 192) else "attn_kernel")
            assert name.split("<")[0] == want, (split, c, name)
            if want == "attn_kernel":
                assert name.endswith(", true>") == bool(split and c["dtype"] == kn.F32 and c["head_dim"] == 64), (split, c, name)
    assert served == 2 * (72 + 16 + 16 + 8)          # per mode: plain everywhere, fp8 and qx on 16 cases each, v_rows on 8
    assert len(got["conv"]) == 2 * len(kn.CONV_SHAPES)
    tiles = set()
    for (nimg, h, w, c0, c1, n), dt, rc, name in got["conv"]:
        assert rc == 0 and name in symbols and name.startswith(f"conv_patch_kernel<{TAGS[dt]}, "), (h, w, n, name)
        th, tw, bn = (int(v) for v in name[:-1].split(", ")[1:])
        assert h % th == 0 and w % tw == 0 and bn == (160 if conv_bn or (n % 160 == 0 and n % 128) else 128), (h, w, n, name)
        tiles.add((th, tw))
    assert tiles == {(16, 8), (8, 14), (8, 16)}


def test_the_cases_the_python_mirror_got_wrong():
    got = child("pins")
    assert got["f32_split"] == [False, 0]
    assert got["sq320_rowvec"] == [0, "sq320_kernel<bf16_tag, true, true>"]                      # the row vector is a template argument
    assert got["attn_v_rows_128"] == [0, "attn_pipe_kernel<bf16_tag>"]
    rc, name = got["attn_split16"]
    assert rc == 0 and name == "attn_kernel<f32_tag, 64, 1, false, false, true>"                 # AttnRoute::SPLIT16, not the plain kernel
    rc, name = got["presplit_a"]
    m = re.fullmatch(r"gemm_kernel<f32_tag, (\d+, ){6}(\d+)>", name)
    assert rc == 0 and m and int(m.group(2)) & 32 and int(m.group(2)) & 8, name                  # + 32: the A operand arrives pre-split
    assert got["short_buffer"] == -1                                                             # TT_EINVAL: the name does not fit


def test_the_library_reads_the_switches_its_own_way():
    """values atoi reads as 0 although they are not the string "0": both sides are in the mode the library is in"""
    got = child("pins", TT_F32_SPLIT="00")
    assert got["f32_split"] == [False, 0]
    assert got["sq320_rowvec"][0] == 0
    got = child("pins", TT_ATTN_PIPE="00")
    assert got["attn_v_rows_128"] == [0, "attn_kernel<bf16_tag, 64, 0, false, true, false>"]
    got = child("pins", TT_F32_SPLIT="2")
    assert got["f32_split"] == [True, 1]


def test_ops_holds_no_copy_of_the_dispatch():
    src = open(os.path.join(ROOT, "this_and_that_vdm_amd", "ops.py")).read()
    assert "TT_ATTN_PIPE" not in src and "TT_F32_SPLIT" not in src
    assert "kmode" not in src and "cfg[" not in src
