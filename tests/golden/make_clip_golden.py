"""Writes tests/golden/clip_tiny.npz and tests/golden/clip_keys.json: the tiny CLIP configurations of tests/clip_reference.py (V17, V257,
T77) filled with the repository's hash fill, loaded into TRANSFORMERS' OWN CPU fp32 classes, and run there -- the restatement's leaves are
pinned against what transformers computes, the product is then tested against the restatement.  Only inputs, outputs, key names and shapes
are stored (images as two moments of the regenerated input, the 257-token hidden state as every 8th row); the weights regenerate from
the hash (fill_parameters_(..., "clip.")).

    python -m tests.golden.make_clip_golden

transformers names CLIPTextModel's parameters without the ``text_model.`` prefix in some versions; the shipped SD-2.1 checkpoints (and the
restatement, and the product class) have it.  ``to_transformers`` maps whichever way the installed version needs."""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def to_transformers(sd, model):
    """the restatement's state dict under the key names the live transformers module uses"""
    want = set(model.state_dict().keys())
    out = {}
    for k, v in sd.items():
        if k in want:
            out[k] = v
        elif k.startswith("text_model.") and k[len("text_model."):] in want:
            out[k[len("text_model."):]] = v
        elif "text_model." + k in want:
            out["text_model." + k] = v
        else:
            raise KeyError(f"{k}: no such parameter in {type(model).__name__}")
    for k in want - set(out):                       # buffers older versions keep in the state dict
        if k.endswith("position_ids"):
            out[k] = model.state_dict()[k]
    return out


def transformers_model(name, ref, cfg):
    import transformers
    if "vocab_size" in cfg:
        tc = transformers.CLIPTextConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                                         num_hidden_layers=cfg["num_hidden_layers"], num_attention_heads=cfg["num_attention_heads"],
                                         max_position_embeddings=cfg["max_position_embeddings"], hidden_act=cfg["hidden_act"],
                                         layer_norm_eps=cfg["layer_norm_eps"], projection_dim=64,
                                         eos_token_id=cfg["vocab_size"] - 1, bos_token_id=0, pad_token_id=1)
        m = transformers.CLIPTextModel(tc)
    else:
        vc = transformers.CLIPVisionConfig(hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                                           num_hidden_layers=cfg["num_hidden_layers"], num_attention_heads=cfg["num_attention_heads"],
                                           image_size=cfg["image_size"], patch_size=cfg["patch_size"], projection_dim=cfg["projection_dim"],
                                           hidden_act=cfg["hidden_act"], layer_norm_eps=cfg["layer_norm_eps"])
        m = transformers.CLIPVisionModelWithProjection(vc)
    m = m.eval().float()
    m.load_state_dict(to_transformers(ref.state_dict(), m), strict=True)
    return m


def run_transformers(name, ref, cfg, x):
    m = transformers_model(name, ref, cfg)
    with torch.no_grad():
        if "vocab_size" in cfg:
            return {"last_hidden_state": m(input_ids=x).last_hidden_state}
        o = m(pixel_values=x)
        return {"image_embeds": o.image_embeds, "last_hidden_state": o.last_hidden_state}


def main():
    from tests import clip_reference as cr
    arrays, keys = {}, {}
    for name in cr.TINY:
        ref, cfg = cr.build(name)
        x = cr.inputs(name)
        if x.dtype == torch.int64:
            arrays[f"{name}.input"] = x.numpy()
        else:                                       # images regenerate from the hash (clip_reference.inputs): two moments pin them
            arrays[f"{name}.input_moments"] = np.array([x.double().sum().item(), x.double().abs().sum().item()])
        for k, v in run_transformers(name, ref, cfg, x).items():
            v = v.numpy().astype(np.float32)
            if k == "last_hidden_state" and v.shape[1] > 100:      # 257 tokens: every 8th row and the last (the class row is row 0)
                rows = np.unique(np.append(np.arange(0, v.shape[1], 8), v.shape[1] - 1))
                arrays[f"{name}.{k}_rows"] = rows
                v = v[:, rows]
            arrays[f"{name}.{k}"] = v
        keys[name] = {k: list(v.shape) for k, v in ref.state_dict().items()}
    np.savez_compressed(os.path.join(HERE, "clip_tiny.npz"), **arrays)
    with open(os.path.join(HERE, "clip_keys.json"), "w") as f:
        json.dump(keys, f, indent=1, sort_keys=True)
    print({k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main()
