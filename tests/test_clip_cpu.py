"""CPU: the CLIP restatement (tests/clip_reference.py) against transformers' recorded and live outputs, and the host side of the native
classes (this_and_that_vdm_amd/clip.py): key layout, strict loading, from_pretrained, constructor refusals.  No kernel runs here."""
import json
import os

import numpy as np
import pytest
import torch

from tests import clip_reference as cr
from tests.parity_common import assert_north_star

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "clip_tiny.npz")
KEYS = os.path.join(HERE, "golden", "clip_keys.json")


def golden_outputs(name):
    """{output name: (recorded tensor, row index of last_hidden_state or None)} and the input of tiny config `name`"""
    g = np.load(GOLDEN)
    x = cr.inputs(name)
    if f"{name}.input" in g.files:
        assert torch.equal(x, torch.from_numpy(g[f"{name}.input"]))
    else:
        m = g[f"{name}.input_moments"]
        # (fp64 sums of ~1e5 fp32 values: the summation order may differ between torch builds, a changed input moves them by far more)
        assert x.double().sum().item() == pytest.approx(m[0], rel=1e-9, abs=1e-7) and x.double().abs().sum().item() == pytest.approx(m[1], rel=1e-9)
    outs = {}
    for k in ("image_embeds", "last_hidden_state"):
        if f"{name}.{k}" in g.files:
            rows = torch.from_numpy(g[f"{name}.{k}_rows"]) if f"{name}.{k}_rows" in g.files else None
            outs[k] = (torch.from_numpy(g[f"{name}.{k}"]), rows)
    return x, outs


def check_against_golden(name, out, what):
    _, outs = golden_outputs(name)
    for k, (want, rows) in outs.items():
        got = getattr(out, k)
        assert_north_star(got if rows is None else got[:, rows.to(got.device)], want, f"{what} {name}.{k}")


def native(name, **override):
    from this_and_that_vdm_amd import clip
    cfg = dict(cr.TINY[name], **override)
    return (clip.CLIPTextModel if "vocab_size" in cfg else clip.CLIPVisionModelWithProjection)(**cfg)


@pytest.mark.parametrize("name", list(cr.TINY))
def test_restatement_reproduces_the_transformers_outputs(name):
    ref, _ = cr.build(name)
    with torch.no_grad():
        check_against_golden(name, ref(cr.inputs(name)), "restatement")


@pytest.mark.parametrize("name", list(cr.TINY))
def test_restatement_equals_live_transformers(name):
    pytest.importorskip("transformers")
    from tests.golden.make_clip_golden import run_transformers
    ref, cfg = cr.build(name)
    x = cr.inputs(name)
    with torch.no_grad():
        got = ref(x)
    for k, want in run_transformers(name, ref, cfg, x).items():
        assert_north_star(getattr(got, k), want, f"{name}.{k}")


@pytest.mark.parametrize("name", list(cr.TINY))
def test_native_state_dict_has_the_checkpoint_layout(name):
    want = json.load(open(KEYS))[name]
    got = {k: list(v.shape) for k, v in native(name).state_dict().items()}
    assert got == want
    assert got == {k: list(v.shape) for k, v in cr.build(name)[0].state_dict().items()}


@pytest.mark.parametrize("name", ["V17", "T77"])
def test_strict_load_with_and_without_position_ids(name):
    ref, cfg = cr.build(name)
    sd = ref.state_dict()
    m = native(name)
    m.load_state_dict(sd, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    prefix = "text_model" if "vocab_size" in cfg else "vision_model"
    npos = ref.state_dict()[f"{prefix}.embeddings.position_embedding.weight"].shape[0]
    native(name).load_state_dict(dict(sd, **{f"{prefix}.embeddings.position_ids": torch.arange(npos)[None]}), strict=True)
    with pytest.raises(RuntimeError):
        native(name).load_state_dict(dict(sd, stray=torch.zeros(1)), strict=True)


@pytest.mark.parametrize("name,sub", [("V17", "image_encoder"), ("T77", "text_encoder")])
def test_from_pretrained_round_trip(tmp_path, name, sub):
    from safetensors.torch import save_file
    from this_and_that_vdm_amd import clip
    ref, cfg = cr.build(name)
    sd = {k: v.half().contiguous() for k, v in ref.state_dict().items()}
    cls = clip.CLIPTextModel if "vocab_size" in cfg else clip.CLIPVisionModelWithProjection
    # single fp16 file, config nested the way a combined CLIPConfig stores it
    d = tmp_path / "single" / sub
    d.mkdir(parents=True)
    json.dump({cls._sub_config: cfg, "model_type": "clip"}, open(d / "config.json", "w"))
    save_file(sd, str(d / "model.fp16.safetensors"))
    m = cls.from_pretrained(str(tmp_path / "single"), subfolder=sub, variant="fp16", torch_dtype=torch.float16)
    assert next(m.parameters()).dtype == torch.float16 and not m.training
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # sharded index, flat config
    d = tmp_path / "sharded" / sub
    d.mkdir(parents=True)
    json.dump(cfg, open(d / "config.json", "w"))
    names = sorted(sd)
    shards = {"model-00001-of-00002.safetensors": names[: len(names) // 2], "model-00002-of-00002.safetensors": names[len(names) // 2:]}
    for f, ks in shards.items():
        save_file({k: sd[k] for k in ks}, str(d / f))
    json.dump({"weight_map": {k: f for f, ks in shards.items() for k in ks}}, open(d / "model.safetensors.index.json", "w"))
    m2 = cls.from_pretrained(str(tmp_path / "sharded"), subfolder=sub)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # save_pretrained -> from_pretrained
    m2.save_pretrained(str(tmp_path / "saved"))
    m3 = cls.from_pretrained(str(tmp_path / "saved"))
    assert dict(m3.config) == dict(m2.config)
    with pytest.raises(OSError):
        cls.from_pretrained(str(tmp_path / "sharded"), subfolder=sub, variant="fp16")


def test_constructor_refusals():
    with pytest.raises(NotImplementedError, match="head dimension 96"):
        native("V17", hidden_size=192)
    with pytest.raises(NotImplementedError, match="head dimension 96"):
        native("T77", hidden_size=192)
    with pytest.raises(NotImplementedError, match="hidden_act"):
        native("V17", hidden_act="relu")
    with pytest.raises(ValueError, match="patches"):
        native("V17", image_size=60)
    native("T77", hidden_act="quick_gelu")


def test_off_device_input_raises():
    m = native("T77")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(cr.inputs("T77"))
    v = native("V17")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        v(cr.inputs("V17"))
    assert next(v.parameters()).dtype == torch.float32
    assert next(v.to(torch.float16).eval().requires_grad_(False).parameters()).dtype == torch.float16


def test_ops_refuse_cpu_tensors():
    from this_and_that_vdm_amd import ops
    z = torch.zeros(8, 64, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.encoder_attention(z, z, z, z.clone(), nseq=1, l=8, heads=1, head_dim=64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.act_rows(z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.patch_tokens(torch.zeros(1, 3, 14, 14), 14, torch.float16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.embed_rows(z, z, ids=torch.zeros(8, dtype=torch.int64), l=8)
