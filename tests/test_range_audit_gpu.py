"""GPU: the range audit around the fused denoise loop, on the tiny models of tests/parity_common.build_pair.  The audit must not
change a single output bit, must describe exactly the tensors the ops functions wrote (pointer, rows and stride at every call site),
must name its sites alike in every step and in graph and eager mode, and its verdicts must name a planted overflow."""
import numpy as np
import pytest
import torch

from tests import tensor_stats_reference as R
from tests.parity_common import build_pair
from this_and_that_vdm_amd import audit, ops

pytestmark = pytest.mark.gpu
NP_BITS = {"f32": (torch.int32, np.uint32), "f16": (torch.int16, np.uint16), "bf16": (torch.int16, np.uint16), "e4m3": (torch.uint8, np.uint8)}
STEPS = 3


def _kw(steps=STEPS, with_cn=True):
    from this_and_that_vdm_amd.svd.scheduling_euler_discrete import EulerDiscreteScheduler
    from this_and_that_vdm_amd.utils.synthetic import synthetic_inputs
    inp = synthetic_inputs(2, 4, 8, 16, ctx_tokens=5, ctx_dim=64, seed=3)
    sched = EulerDiscreteScheduler()
    sched.set_timesteps(steps)
    return dict(latents=inp["latents"], image_latents=inp["image_latents"], encoder_hidden_states=inp["encoder_hidden_states"],
                added_time_ids=inp["added_time_ids"], guidance_scale=inp["guidance_scale"], sigmas=sched.sigmas,
                timesteps=sched.timesteps, controlnet_cond=inp["gesture_latents"] if with_cn else None)


@pytest.fixture(scope="module")
def pair16():
    p_unet, p_cn, _, _ = build_pair("tiny_vgl", torch.float16, "cuda:0", True)
    return p_unet, p_cn


def _run(loop, kw, steps=None, **audit_kw):
    """begin + run under a fresh audit -> (latents, report, audit, sites registered by begin())"""
    with audit.RangeAudit(**audit_kw) as a:
        audit.watch(loop.unet, "unet")
        if loop.controlnet is not None:
            audit.watch(loop.controlnet, "controlnet")
        loop.begin(**kw)
        n_begin = len(a.report())
        out = loop.run(steps).clone()
        rep = a.report()
    return out, rep, a, n_begin


@torch.no_grad()
def test_audit_changes_no_output_bit(pair16):
    from this_and_that_vdm_amd.svd.denoise import DenoiseLoop
    kw = _kw()
    for graph in (True, False):
        plain = DenoiseLoop(*pair16, use_graph=graph).begin(**kw).run().clone()
        audited, rep, _, _ = _run(DenoiseLoop(*pair16, use_graph=graph), kw)
        assert torch.equal(plain, audited), f"use_graph={graph}: the audit changed the latents"
        assert len(rep) > 100 and not rep.nonfinite()


@torch.no_grad()
def test_every_record_describes_the_tensor_its_op_wrote(pair16):
    """keep_tensors: a clone of every audited output, taken right after its statistics launch; every site's record must equal the
    reference of its clone -- a wrong pointer, row count or stride at any call site shows here.  And the number of records equals the
    number of ledger writes of floating tensors (minus audit.EXEMPT): a site name used twice would merge two of them."""
    from this_and_that_vdm_amd.svd.denoise import DenoiseLoop
    calls = []
    orig = ops._wrote

    def counting(t, op="op"):
        calls.append((op, t.dtype))
        return orig(t, op)

    ops._wrote = counting
    try:
        _, rep, a, _ = _run(DenoiseLoop(*pair16, use_graph=False), _kw(steps=1), keep_tensors=True)
    finally:
        ops._wrote = orig
    floating = [c for c in calls if c[1].is_floating_point]
    exempt = [c for c in floating if c[0] in audit.EXEMPT]
    print(f"{len(calls)} ledger writes, {len(floating)} of floating tensors, {len(exempt)} exempt {sorted(audit.EXEMPT)}, {len(rep)} records")
    assert len(rep) == len(floating) - len(exempt) and len(set(rep.sites())) == len(rep)
    assert set(a.kept) == set(rep.sites())
    ops_seen = {s.split("/")[1].split("#")[0] for s in rep.sites()}
    print("ops audited:", sorted(ops_seen))
    assert {"gemm", "attention", "groupnorm", "prep_model_input", "cfg_euler_step"} <= ops_seen, ops_seen
    assert any(s.startswith("unet.down_blocks.0.") for s in rep.sites()) and any(s.startswith("controlnet.") for s in rep.sites())
    for row in rep.rows:
        t = a.kept[row["site"]]
        tb, nb = NP_BITS[row["dtype"]]
        assert list(t.shape) == row["shape"]
        R.assert_matches(row["record"], R.reference(t.contiguous().view(tb).cpu().numpy().view(nb), row["dtype"]), row["site"])


@torch.no_grad()
def test_graph_and_eager_steps_give_the_same_report(pair16):
    from this_and_that_vdm_amd.svd.denoise import DenoiseLoop
    kw = _kw()
    _, graph, _, nb_g = _run(DenoiseLoop(*pair16, use_graph=True), kw)
    _, eager, _, nb_e = _run(DenoiseLoop(*pair16, use_graph=False), kw)
    assert graph.sites() == eager.sites() and nb_g == nb_e
    assert graph.rows == eager.rows                           # every field, the fp64 sums included: the same launches on the same bits
    _, one, _, nb_1 = _run(DenoiseLoop(*pair16, use_graph=True), kw, steps=1)
    assert one.sites() == graph.sites() and nb_1 == nb_g      # a step names its sites like every other step
    for i, (r1, rn) in enumerate(zip(one.rows, graph.rows)):
        times = 1 if i < nb_1 else STEPS                      # begin()'s sites once, a step's sites once per step (the warm-up pass of the
        assert rn["record"]["count"] == times * r1["record"]["count"], rn["site"]        # capture is taken back out)
        assert rn["shape"] == r1["shape"]


@torch.no_grad()
def test_successive_audits_and_none_afterwards(pair16):
    from this_and_that_vdm_amd.svd.denoise import DenoiseLoop
    kw = _kw()
    loop = DenoiseLoop(*pair16, use_graph=True)
    out1, rep1, a1, _ = _run(loop, kw)
    out2, rep2, a2, _ = _run(loop, kw)
    assert torch.equal(out1, out2) and rep1.rows == rep2.rows and a1.generation != a2.generation
    torch.cuda.synchronize()
    before, before1 = a2.buf.clone(), a1.buf.clone()
    ops.PROFILE = []
    try:
        out3 = loop.begin(**kw).run().clone()                 # no audit: a graph captured under one must not be replayed
    finally:
        prof, ops.PROFILE = ops.PROFILE, None
    torch.cuda.synchronize()
    assert torch.equal(out3, out1) and torch.equal(a2.buf, before) and torch.equal(a1.buf, before1)
    assert loop._audit is None and prof
    # a loop that began without an audit refuses to step under one (and the other way round)
    loop.begin(**kw)
    with audit.RangeAudit():
        with pytest.raises(RuntimeError, match="call begin\\(\\) again"):
            loop.step()
    # out of capacity: refused before the site's statistics launch, the op itself has run
    with audit.RangeAudit(capacity=3) as small:
        with pytest.raises(RuntimeError, match="holds 3 records"):
            DenoiseLoop(*pair16, use_graph=False).begin(**kw)
        assert len(small.report()) == 3
    assert ops.AUDIT is None


def _first_resblock(unet):
    from this_and_that_vdm_amd.svd.layers import ResnetBlock2D
    return next((n, m) for n, m in unet.named_modules() if isinstance(m, ResnetBlock2D))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@torch.no_grad()
def test_verdict_names_a_planted_overflow(dtype):
    """conv1 of the first ResBlock scaled by 2^18: its output, site <block>/gemm#0, exceeds 65520.  TT_F32 storage holds it: the fp16
    verdict names that site first, the bf16 verdict is empty, nothing is non-finite.  fp16 storage does not: the first non-finite
    site is that same one -- after ONE step: a later step starts from latents the first one already spoiled, and its records
    accumulate into the sites before the planted one."""
    from this_and_that_vdm_amd.svd.denoise import DenoiseLoop
    p_unet, _, _, _ = build_pair("tiny_vgl", dtype, "cuda:0", False)
    name, block = _first_resblock(p_unet)
    block.conv1.weight.mul_(2.0 ** 18)
    block.conv1.bias.mul_(2.0 ** 18)
    assert torch.isfinite(block.conv1.weight).all()
    site = f"unet.{name}/gemm#0"
    _, rep, _, _ = _run(DenoiseLoop(p_unet, None, use_graph=True), _kw(with_cn=False), steps=None if dtype == torch.float32 else 1)
    assert site in rep.sites()
    if dtype == torch.float32:
        v = rep.verdict("fp16")
        print(v["sites"][:3], rep.row(site)["record"]["max_abs"])
        assert v["first"] == site and v["sites"][0]["count"] > 0 and rep.row(site)["record"]["max_abs"] >= 65520.0
        assert rep.verdict("bf16")["sites"] == [] and rep.nonfinite() == []
        assert rep.worst(1)[0]["record"]["max_abs"] >= rep.row(site)["record"]["max_abs"]
    else:
        bad = rep.nonfinite()
        assert bad and bad[0]["site"] == site and bad[0]["record"]["n_pinf"] + bad[0]["record"]["n_ninf"] > 0
        assert rep.verdict("fp16")["first"] == site


@torch.no_grad()
def test_fp8_attention_sites_report_clipped_values():
    """attention_fp8 with the query projection of the first spatial transformer block scaled by 2^12: its Q | K operand (e4m3) sits at
    the clip, which only the statistics can tell -- the conversion saturates silently"""
    from this_and_that_vdm_amd.svd.denoise import DenoiseLoop
    from this_and_that_vdm_amd.svd.layers import BasicTransformerBlock
    kw = _kw(with_cn=False)
    reports = []
    for scale in (1.0, 2.0 ** 12):
        p_unet, _, _, _ = build_pair("tiny_vgl", torch.float16, "cuda:0", False)
        p_unet.attention_fp8 = True
        name, block = next((n, m) for n, m in p_unet.named_modules() if isinstance(m, BasicTransformerBlock))
        block.attn1.to_q.weight.mul_(scale)
        assert torch.isfinite(block.attn1.to_q.weight).all()
        reports.append(_run(DenoiseLoop(p_unet, None, use_graph=True), kw)[1])
    base, scaled = reports
    e4m3 = [r["site"] for r in scaled.rows if r["dtype"] == "e4m3"]
    mine = [s for s in e4m3 if s.startswith(f"unet.{name}/")]
    assert e4m3 and mine and base.sites() == scaled.sites()
    v = scaled.verdict("fp8_attention")
    print("clipped before / after:", [(s["site"], s["count"]) for s in base.verdict("fp8_attention")["sites"]], v["sites"][:2])
    assert v["considered"] == len(e4m3) and v["first"] in mine
    grew = [s for s in mine if scaled.row(s)["record"]["n_ge"][0] > base.row(s)["record"]["n_ge"][0]]
    assert grew and grew[0] in [s["site"] for s in v["sites"]]
    hit = scaled.row(grew[0])["record"]
    assert hit["max_abs"] == 448.0 and hit["n_pinf"] == hit["n_ninf"] == 0 and hit["n_ge"][1] == 0
