"""Synthetic pretrained checkpoints for the pretrained-weight tests: the same files, from the same seeds, that
tools/gen_pretrained_golden.py loaded with the reference's own code to write tests/golden/pretrained.npz.

ViT / WRN: ``{'model': state_dict}`` files as the reference's ``load_checkpoint`` reads them.  BERT / Wav2Vec2 / HuBERT: directories as
``save_pretrained`` leaves them (config.json from the fixture, weights in one of two key styles):
  * ``new``:    current names, ``model.safetensors``;
  * ``legacy``: LayerNorm ``gamma`` / ``beta`` and weight-norm ``weight_g`` / ``weight_v`` names, ``pytorch_model.bin``.
"""
import hashlib
import json
import os
import struct

import numpy as np
import torch

from oracle import bert_ref as BR
from oracle import vit_ref as V
from oracle import w2v2_ref as WR
from oracle import wrn_ref as W
from oracle.gen_golden import synth_wrn_params
from semireward_amd.utils import synth

VIT_BASE_P16_224 = dict(V.VIT_BASE_P16_96, img_size=224)      # the geometry of an MAE ViT-B/16 pretraining checkpoint

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731

# ---- ViT: (case, source geometry, target geometry, target builder, classes, batch, seed, key prefix)
VIT_SRC = {"s2_28": dict(V.VIT_SMALL_P2_32, img_size=28), "b16_224": VIT_BASE_P16_224, "s2_32": V.VIT_SMALL_P2_32}
VIT_CASES = {
    "s2_32_from_s2_28": ("s2_28", V.VIT_SMALL_P2_32, "vit_small_patch2_32", 10, 3, 301, "module."),         # 14x14 grid -> 16x16
    "b16_96_from_b16_224": ("b16_224", V.VIT_BASE_P16_96, "vit_base_patch16_96", 10, 3, 302, ""),           # 14x14 -> 6x6
    "s2_32_same_grid": ("s2_32", V.VIT_SMALL_P2_32, "vit_small_patch2_32", 10, 3, 303, ""),                 # 16x16 -> 16x16
}
WRN_CASE = ("wrn_28_2", W.WRN_28_2, 100, 4, 32, 311)          # (tag, geometry, classes, batch, image size, seed)
# ---- transformers snapshots: (family, key style, engine tiny builder, classes, batch, length / samples, seed)
HF_CASES = {
    "bert_new": ("bert", "new", "bert_tiny_test", 4, 3, 24, 321), "bert_legacy": ("bert", "legacy", "bert_tiny_test", 4, 3, 24, 322),
    "w2v_new": ("wav2vec2", "new", "wave2vecv2_tiny_test", 4, 2, 400, 331), "w2v_legacy": ("wav2vec2", "legacy", "wave2vecv2_tiny_test", 4, 2, 400, 332),
    "hubert_new": ("hubert", "new", "hubert_tiny_test", 4, 2, 400, 341), "hubert_legacy": ("hubert", "legacy", "hubert_tiny_test", 4, 2, 400, 342),
}


SAMPLES = 16          # values kept per loaded tensor beside its digest (they name the first differing element when a digest differs)


def tensor_digest(t):
    """SHA-256 of a tensor's contiguous bytes in its own dtype: equal digests = bit-equal tensors."""
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def tensor_sample(t):
    a = t.detach().cpu().contiguous().numpy().ravel()
    return a[::max(1, a.size // SAMPLES)][:SAMPLES].astype(np.float64)


def record_loaded(out, tag, named):
    """Fixture entries of the tensors a reference model holds after loading: names, digests, strided samples."""
    names, digests, samples = [], [], []
    for n, t in named:
        names.append(n)
        digests.append(tensor_digest(t))
        samples.append(tensor_sample(t))
    out[f"{tag}/names"], out[f"{tag}/sha256"] = np.array(names), np.array(digests)
    out[f"{tag}/sample_len"] = np.array([s.size for s in samples], dtype=np.int64)
    out[f"{tag}/samples"] = np.concatenate(samples)


def loaded_reference(g, tag):
    """{name: (digest, samples)} of a fixture tag."""
    lens = g[f"{tag}/sample_len"]
    ends = np.cumsum(lens)
    smp = g[f"{tag}/samples"]
    return {str(n): (str(h), smp[e - k:e]) for n, h, k, e in zip(g[f"{tag}/names"], g[f"{tag}/sha256"], lens, ends)}


def assert_loaded(model, g, tag):
    """Every tensor the reference loaded is bit-equal in the engine's fp32 block (or buffers): samples first, for a readable failure."""
    ref = loaded_reference(g, tag)
    assert ref
    for n, (h, s) in ref.items():
        t = model.buffers[n] if n in model.buffers else model.view(n)
        np.testing.assert_array_equal(tensor_sample(t), s, err_msg=n)
        assert tensor_digest(t) == h, n


def vit_pos_embed_shape(case):
    tgt = VIT_CASES[case][1]
    return (1, (tgt["img_size"] // tgt["patch_size"]) ** 2 + 1, tgt["embed_dim"])


def vit_checkpoint(case):
    """A timm-style checkpoint of the source geometry: every parameter (head included), an extra ``mask_token`` and the case's prefix."""
    src, _, _, _, _, seed, prefix = VIT_CASES[case]
    cfg = V.VitCfg(num_classes=1000, **VIT_SRC[src])
    P = synth.synth_params(V.param_shapes(cfg) + [("mask_token", (1, 1, cfg.embed_dim))], seed)
    return {"model": {prefix + k: T(v) for k, v in P.items()}}


def vit_head(case):
    _, tgt, _, C, _, seed, _ = VIT_CASES[case]
    D = tgt["embed_dim"]
    return {k: T(v) for k, v in synth.synth_params([("head.weight", (C, D)), ("head.bias", (C,))], seed + 50).items()}


def vit_input(case):
    _, tgt, _, _, B, seed, _ = VIT_CASES[case]
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    return rng.standard_normal((B, 3, tgt["img_size"], tgt["img_size"])).astype(np.float32)


def wrn_checkpoint():
    """A DataParallel-saved WRN-28-2 (``module.`` keys): parameters, BatchNorm running statistics and counters, its classifier."""
    _, geo, C, _, _, seed = WRN_CASE
    cfg = W.WrnCfg(num_classes=C, **geo)
    sd = {k: T(v) for k, v in synth_wrn_params(cfg, seed).items()}
    rng = np.random.Generator(np.random.PCG64(seed + 2))
    for n, c, _ in W.bn_names(cfg):
        sd[n + ".running_mean"] = T((0.1 * rng.standard_normal(c)).astype(np.float32))
        sd[n + ".running_var"] = T((1.0 + 0.2 * rng.random(c)).astype(np.float32))
        sd[n + ".num_batches_tracked"] = torch.tensor(1234, dtype=torch.int64)
    return {"model": {"module." + k: v for k, v in sd.items()}}


def wrn_head():
    _, _, C, _, _, seed = WRN_CASE
    return {k: T(v) for k, v in synth.synth_params([("classifier.weight", (C, 128)), ("classifier.bias", (C,))], seed + 50).items()}


def wrn_input():
    _, _, _, B, HW, seed = WRN_CASE
    return np.random.Generator(np.random.PCG64(seed + 1)).standard_normal((B, 3, HW, HW)).astype(np.float32)


def hf_geometry(family):
    return BR.BERT_TINY_TEST if family == "bert" else WR.W2V_TINY_TEST


def _engine_params(family, C, seed):
    if family == "bert":
        return BR.synth_params(BR.BertCfg(num_classes=C, **BR.BERT_TINY_TEST), seed)
    return WR.synth_params(WR.W2vCfg(num_classes=C, **WR.W2V_TINY_TEST), seed)


def hf_state_dict(case):
    """The checkpoint of a transformers task model: its prefix, its task head, the style's names."""
    family, style, _, C, _, _, seed = HF_CASES[case]
    P = {k: v for k, v in _engine_params(family, C, seed).items() if not k.startswith("classifier.")}
    D = hf_geometry(family)["hidden"]
    if family == "bert":
        base = {k[len("bert."):]: v for k, v in P.items()}
        extra = [("pooler.dense.weight", (D, D)), ("pooler.dense.bias", (D,))]
        head = [("cls.predictions.bias", (BR.BERT_TINY_TEST["vocab"],)), ("cls.predictions.transform.dense.weight", (D, D))]
        prefix = "bert."
    else:
        base = {k[len("model."):]: v for k, v in P.items()}
        extra = []
        if style == "new":
            head = [("lm_head.weight", (32, D)), ("lm_head.bias", (32,))]
        else:
            head = [("quantizer.codevectors", (1, 16, 32)), ("project_q.weight", (32, 32)), ("project_hid.weight", (32, D))]
        prefix = "hubert." if (family, style) == ("hubert", "legacy") else ("" if family == "hubert" else "wav2vec2.")
    base.update({k: v for k, v in synth.synth_params(extra, seed + 7).items()})
    sd = {prefix + k: T(v) for k, v in base.items()}
    sd.update({k: T(v) for k, v in synth.synth_params(head, seed + 8).items()})
    if style == "legacy":
        ren = {"LayerNorm.weight": "LayerNorm.gamma", "LayerNorm.bias": "LayerNorm.beta",
               "parametrizations.weight.original0": "weight_g", "parametrizations.weight.original1": "weight_v"}
        out = {}
        for k, v in sd.items():
            for a, b in ren.items():
                if k.endswith(a):
                    k = k[:-len(a)] + b
            out[k] = v
        sd = out
        if family == "bert":
            sd["bert.embeddings.position_ids"] = torch.arange(BR.BERT_TINY_TEST["max_pos"], dtype=torch.int64)[None]
    return sd


def hf_head(case):
    family, _, _, C, _, _, seed = HF_CASES[case]
    D = hf_geometry(family)["hidden"]
    shapes = [("classifier.0.weight", (D, D)), ("classifier.0.bias", (D,)), ("classifier.2.weight", (C, D)), ("classifier.2.bias", (C,))]
    return {k: T(v) for k, v in synth.synth_params(shapes, seed + 50).items()}


def hf_input(case):
    family, _, _, _, B, L, seed = HF_CASES[case]
    if family == "bert":
        ids, mask = BR.synth_tokens(seed + 1, B, L, BR.BERT_TINY_TEST["vocab"])
        return {"input_ids": T(ids), "attention_mask": T(mask)}
    return np.random.Generator(np.random.PCG64(seed + 1)).standard_normal((B, L)).astype(np.float32)


_ST = {torch.float32: "F32", torch.int64: "I64"}


def write_safetensors(path, sd):
    header, blobs, off = {}, [], 0
    for k, t in sd.items():
        b = t.contiguous().numpy().tobytes()
        header[k] = {"dtype": _ST[t.dtype], "shape": list(t.shape), "data_offsets": [off, off + len(b)]}
        blobs.append(b)
        off += len(b)
    h = json.dumps(header, separators=(",", ":")).encode()
    h += b" " * (-len(h) % 8)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(h)))
        f.write(h)
        for b in blobs:
            f.write(b)


def write_hf_dir(d, case, config_json):
    """A ``save_pretrained`` directory of ``case``: config.json (text from the fixture) + the style's weights file."""
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "config.json"), "w") as f:
        f.write(config_json)
    sd = hf_state_dict(case)
    if HF_CASES[case][1] == "new":
        write_safetensors(os.path.join(d, "model.safetensors"), sd)
    else:
        torch.save(sd, os.path.join(d, "pytorch_model.bin"))
    return d


def hub_snapshot_dir(cache, name, revision="0123456789abcdef0123456789abcdef01234567"):
    """The Hugging Face hub-cache layout for model ``name``: ``refs/main`` names the snapshot directory returned (created empty)."""
    repo = os.path.join(cache, "models--" + name.replace("/", "--"))
    os.makedirs(os.path.join(repo, "refs"), exist_ok=True)
    with open(os.path.join(repo, "refs", "main"), "w") as f:
        f.write(revision)
    snap = os.path.join(repo, "snapshots", revision)
    os.makedirs(snap, exist_ok=True)
    return snap


def torch_hub_file(torch_home, url):
    """Where ``load_state_dict_from_url(url)`` caches its file under TORCH_HOME (the directory is created)."""
    d = os.path.join(torch_home, "hub", "checkpoints")
    os.makedirs(d, exist_ok=True)
    return os.path.join(d, url.rsplit("/", 1)[-1])
