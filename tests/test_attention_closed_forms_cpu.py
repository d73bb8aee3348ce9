"""CPU: the closed-form attention cases of tests/attention_closed_forms.py against the emulation of the kernels' arithmetic in the same
module -- every family on every route shape passes its bound (worst err/bound per family printed), the margin and range assumptions of the
families hold in fp64 on the storage values, and every kernel defect of the list below that changes what a route shape computes makes at
least one family fail there:

    drop_last   the last key dropped                      leak_next  the key behind the last one let in (padding, or the next sequence's first)
    double      a key counted twice                       unmasked   the padding of the ragged last tile unmasked
    scale       softmax scale x 1.01 (F3; not asked of fp8, whose u_P = 2^-4 hides it)
    no_batch0   the context pairing computed without batch0        causal_ge  causal `>` written as `>=`

A defect that leaves a route shape's arithmetic alone is not run there (unmasked where lk is a multiple of the tile, leak_next / unmasked
under the causal mask, which covers those keys anyway); tests/attention_closed_forms.mutants_for has the rule."""
import time

import pytest
import torch

from tests import attention_closed_forms as cf

ROUTES = cf.routes()
WORST = {}
CAUGHT = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    t0 = time.time()
    yield
    print(f"\n[closed forms, emulation] module time {time.time() - t0:.1f} s; worst err/bound per family:")
    for k, v in sorted(WORST.items()):
        print(f"[closed forms, emulation]   {k}: {v:.3g}")
    print("[closed forms, emulation] route shapes on which each mutant ran and was caught: " + ", ".join(f"{k} {v}" for k, v in sorted(CAUGHT.items())))


def _passes(P):
    out, slow = cf.emulate(P)
    ratio, msg = cf.check(P, out)
    assert msg is None, msg
    key = f"{P.family} {P.entry}"
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    return out, slow


def _fails(P, mutant):
    out, _ = cf.emulate(P, mutant)
    return cf.check(P, out)[1] is not None


# which family to try first against a mutant (any family may catch it)
FIRST = {"drop_last": "F1", "leak_next": "F1", "double": "F1", "unmasked": "F1", "scale": "F3", "no_batch0": "F2", "causal_ge": "F2"}


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: r.id)
def test_emulation_passes_and_mutants_fail(route):
    probs = {}
    for fam in route.families:
        P = probs[fam] = route.make(fam)
        if fam == "F2":
            cf.assert_margin(P)
        if fam == "F3" and P.ptype == "fp8":
            cf.assert_fp8_range(P)
        plain, slow = _passes(P)
        if route.slow_later is not None:
            assert slow == route.slow_later, f"{P.name}: a later tile took the slow path: {slow}"
        if fam != "F3":
            # the layout contracts leave the emulation's bits alone as well
            Pp = route.make(fam, poison=True)
            assert torch.equal(_passes(Pp)[0], plain), Pp.name
            # ... and a padding key that is let in meets the poisoned fill: on the poisoned buffers BOTH families fail, F2 because the
            # leaked key carries a selected code twice as loud and +-256 in V (tt_temporal_attention's poison sits in columns, not keys)
            if route.slow_later is None and not route.causal and not route.temporal:
                for mutant in ["leak_next"] + (["unmasked"] if route.unmasked else []):
                    assert _fails(Pp, mutant), f"{Pp.name}: mutant {mutant} passes on poisoned padding"
                    CAUGHT[mutant + " (poisoned, " + fam + ")"] = CAUGHT.get(mutant + " (poisoned, " + fam + ")", 0) + 1
            if route.views:
                for cb, cls in ((2, 1), (3, 2)):
                    assert torch.equal(_passes(route.make(fam, cb=cb, cls=cls))[0], plain)
    if route.slow_later is not None:
        return
    P0 = probs["F1"]
    for mutant in cf.mutants_for(route, P0):
        order = [FIRST[mutant]] + [f for f in route.families if f != FIRST[mutant]]
        if mutant == "scale":
            order = ["F3"]
        assert any(_fails(probs[f], mutant) for f in order), f"{route.id}: mutant {mutant} passes every family"
        CAUGHT[mutant] = CAUGHT.get(mutant, 0) + 1
    if route.batch0:
        full = {fam: cf.emulate(probs[fam])[0] for fam in ("F1", "F2")}
        for b0 in (1, 2):
            for fam in ("F1", "F2"):
                P = route.make(fam, batch0=b0)
                out, _ = _passes(P)
                assert torch.equal(out, full[fam][b0 * P.kw["frames"] * P.kw["lq"]:]), P.name
            assert _fails(P, "no_batch0"), f"{route.id}: batch0 = {b0} ignored passes F2"
            CAUGHT["no_batch0"] = CAUGHT.get("no_batch0", 0) + 1


def _ratio(P, mutant):
    return cf.check(P, cf.emulate(P, mutant)[0])[0]


def test_sensitivity_per_family():
    """What each family is there for, as figures (lk = 200, d = 64; the emulation's err/bound under a defect).  F1 counts keys: a dropped last
    key moves every non-zero output by 1 / 200 of itself against a bound of UNIT -- 35 x in bf16, 280 x in fp16 (the issue's figures; the floors
    below sit 15 % under them).  F3 sees the scale and the weights: 1 % of scale breaks the bound in bf16 and by more than 10 x in fp16, a
    dropped last key by more than 100 x.  F2 is bit for bit or not at all: a dropped last key reads as a wrong V row."""
    for dt, f1_floor, f3_scale_floor in (("bf16", 30.0, 1.0), ("f16", 240.0, 10.0)):
        assert _ratio(cf.attention("F1", dt=dt, lk=200), "drop_last") >= f1_floor
        P3 = cf.attention("F3", dt=dt, lk=200)
        assert _ratio(P3, "scale") > f3_scale_floor and _ratio(P3, "drop_last") > 100.0
        assert _ratio(cf.attention("F2", dt=dt, lk=200), "drop_last") == float("inf")


def test_causal_traps_catch_a_missing_mask():
    """F2 under the causal mask: without the mask the trap keys win for the queries in front of them, and every trapped code is selected by
    some query in front of its trap"""
    for d, l in ((64, 50), (64, 257), (80, 130)):
        P = cf.encoder("F2", dt="bf16", d=d, l=l, causal=True)
        assert cf.check(P, cf.emulate(P)[0])[1] is None
        P.causal = False                                    # the kernel defect: no causal mask at all
        got = cf.emulate(P)[0]
        wrong = (got != P.expected).any(1)
        assert int(wrong.sum()) >= 4 * P.kw["nseq"], (P.name, int(wrong.sum()))


def test_split16_mode_at_head_dim_128_keeps_the_exact_instance():
    """the d = 128 split16 route shapes run with the process-wide switch ON and expect the exact-fp32 instance (attention.hip resolve_attention)"""
    P = cf.attention("F3", dt="f32", d=128, lk=150, split=True)
    assert P.split_mode and not P.split and P.u_p == 0.0 and P.kernel == "attn_kernel<f32_tag, 128, 0, false, false, false>"
    P = cf.attention("F3", dt="f32", d=64, lk=150, split=True)
    assert P.split_mode and P.split and P.u_p > 0.0 and P.kernel == "attn_kernel<f32_tag, 64, 0, false, false, true>"


def test_interesting_keys_and_codes():
    """the set I holds what the issue lists, and the codes are what the margins assume"""
    for lk in (1, 5, 40, 64, 78, 150, 200, 257):
        I = cf.interesting(lk)
        nt = (lk + 63) // 64
        want = {t * 64 for t in range(nt)} | {min(t * 64 + 63, lk - 1) for t in range(nt)} | {j for j in (lk - 1, lk - 2) if j >= 0}
        want |= {t * 64 + o for t in (0, nt - 1) for o in (15, 16, 31, 32) if t * 64 + o < lk}
        assert set(I) == want and len(I) <= 64
    for d in (64, 128):
        h = cf.codes(d, 20)
        assert torch.equal(h @ h.t(), d * torch.eye(20, dtype=torch.float64))
    g = cf.codes(80, 20) @ cf.codes(80, 20).t()
    assert torch.equal(g.diagonal(), torch.full((20,), 80.0, dtype=torch.float64)) and float((g - 80 * torch.eye(20)).abs().max()) <= 16


def test_q_row_permutation_matches_packing():
    """the fused query projection's row order written out in the builder is packing.permute_q_rows"""
    from this_and_that_vdm_amd.packing import permute_q_rows
    P = cf.attention("F2", dt="bf16", lk=5, mask=1, ctx_batches=2, qproj=True)
    assert torch.equal(P.bufs["wq"].double(), permute_q_rows(P.w_logical))
