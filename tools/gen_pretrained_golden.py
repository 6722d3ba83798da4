"""Write tests/golden/pretrained.npz by loading synthetic pretrained checkpoints with the REFERENCE's own loaders (build container only).

TEST INFRASTRUCTURE: imports the reference headless through oracle/_ref_import.py (as oracle/gen_golden.py does) and never runs on the GPU
machine.  The checkpoints are the ones tests/_pretrained_ckpt.py writes from fixed seeds, so the tests regenerate the same files:

  * ViT-S/2@32 (from a 14x14-grid ViT-S/2@28 file and from a same-grid file) and ViT-B/16@96 (from a 14x14-grid ViT-B/16@224 file),
    and WRN-28-2, through ``semilearn.nets.utils.load_checkpoint``;
  * ClassificationBert / ClassificationWave2Vec / ClassificationHubert(name=<dir>) on tiny configs written with ``save_pretrained``, in
    both key styles (current names + safetensors, legacy gamma / weight_g names + pytorch_model.bin).

Recorded: the SHA-256 digest and a strided sample of every loaded tensor (the resampled ``pos_embed`` among them), the
``load_state_dict`` missing / unexpected key lists, eval logits / features on fixed inputs (with a synthetic classifier head set on both sides), and each config.json.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_pretrained_golden.py
"""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn as nn
import transformers  # before the reference's stub packages (a stub ``timm`` would break transformers' import-time probes)
from transformers import BertConfig, HubertConfig, HubertModel, Wav2Vec2Config, Wav2Vec2Model, BertModel  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import _ref_import as R  # noqa: E402
from oracle import wrn_ref as W  # noqa: E402
import _pretrained_ckpt as PC  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pretrained.npz")
record_params = PC.record_loaded


def ref_load_checkpoint(model, path):
    """The reference's load_checkpoint, with the ``match`` it prints captured from its load_state_dict call."""
    utils = R.mod("semilearn.nets.utils")
    rec, orig = [], model.load_state_dict
    model.load_state_dict = lambda sd, strict=True: rec.append(orig(sd, strict=strict)) or rec[-1]
    with contextlib.redirect_stdout(io.StringIO()):
        utils.load_checkpoint(model, path)
    del model.load_state_dict
    return rec[0]


def gen_vit(out, tmp):
    vit = R.mod("semilearn.nets.vit.vit")
    for case, (src, tgt, _, C, _, _, _) in PC.VIT_CASES.items():
        path = os.path.join(tmp, case + ".pth")
        ck = PC.vit_checkpoint(case)
        torch.save(ck, path)
        model = vit.VisionTransformer(num_classes=C, **tgt)
        match = ref_load_checkpoint(model, path)
        out[f"{case}/missing"], out[f"{case}/unexpected"] = np.array(match.missing_keys), np.array(match.unexpected_keys)
        assert tuple(model.pos_embed.shape) == PC.vit_pos_embed_shape(case)
        if src == "s2_32":
            same = torch.equal(model.pos_embed.detach(), ck["model"]["pos_embed"])
            print("same-grid resample is the identity:", same)
        record_params(out, case, [(n, p) for n, p in model.named_parameters() if not n.startswith("head")])
        model.load_state_dict(PC.vit_head(case), strict=False)
        model.eval()
        with torch.no_grad():
            o = model(torch.from_numpy(PC.vit_input(case)))
        out[f"{case}/eval_logits"], out[f"{case}/eval_feat"] = o["logits"].numpy(), o["feat"].numpy()


def gen_wrn(out, tmp):
    wm = R.mod("semilearn.nets.wrn.wrn")
    tag, geo, C, _, _, _ = PC.WRN_CASE
    path = os.path.join(tmp, "wrn.pth")
    torch.save(PC.wrn_checkpoint(), path)
    cfg = W.WrnCfg(num_classes=C, **geo)
    model = wm.WideResNet(first_stride=cfg.first_stride, num_classes=C, depth=cfg.depth, widen_factor=cfg.widen)
    match = ref_load_checkpoint(model, path)
    out[f"{tag}/missing"], out[f"{tag}/unexpected"] = np.array(match.missing_keys), np.array(match.unexpected_keys)
    record_params(out, tag, [(n, t) for n, t in model.state_dict().items() if not n.startswith("classifier")])
    model.load_state_dict(PC.wrn_head(), strict=False)
    model.eval()
    with torch.no_grad():
        o = model(torch.from_numpy(PC.wrn_input()))
    out[f"{tag}/eval_logits"], out[f"{tag}/eval_feat"] = o["logits"].numpy(), o["feat"].numpy()


def hf_config(family, d):
    """A tiny config written by ``save_pretrained``: the engine test builder's geometry, train settings other than the class defaults."""
    g = PC.hf_geometry(family)
    if family == "bert":
        c = BertConfig(vocab_size=g["vocab"], hidden_size=g["hidden"], num_hidden_layers=g["layers"], num_attention_heads=g["heads"],
                       intermediate_size=g["inter"], max_position_embeddings=g["max_pos"], hidden_dropout_prob=0.15,
                       attention_probs_dropout_prob=0.15)
    else:
        c = (HubertConfig if family == "hubert" else Wav2Vec2Config)(
            hidden_size=g["hidden"], num_hidden_layers=g["layers"], num_attention_heads=g["heads"], intermediate_size=g["inter"],
            conv_dim=g["conv_dim"], conv_kernel=g["conv_kernel"], conv_stride=g["conv_stride"], num_conv_pos_embeddings=g["pos_k"],
            num_conv_pos_embedding_groups=g["pos_groups"], feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False,
            hidden_dropout=0.12, attention_dropout=0.08, activation_dropout=0.05, feat_proj_dropout=0.03, layerdrop=0.07, mask_time_prob=0.065,
            mask_time_length=5, mask_time_min_masks=1)
    c.save_pretrained(d)
    with open(os.path.join(d, "config.json")) as f:
        return f.read()


def gen_hf(out, tmp):
    out["meta/transformers_version"] = np.array(transformers.__version__)
    mods = {"bert": ("semilearn.nets.bert.bert", "ClassificationBert"), "wav2vec2": ("semilearn.nets.wave2vecv2.wave2vecv2", "ClassificationWave2Vec"),
            "hubert": ("semilearn.nets.hubert.hubert", "ClassificationHubert")}
    for case, (family, _, _, C, _, _, _) in PC.HF_CASES.items():
        d = os.path.join(tmp, case)
        os.makedirs(d)
        cj = hf_config(family, d)
        PC.write_hf_dir(d, case, cj)
        out[f"{case}/config_json"] = np.array(cj)
        m, cls = mods[family]
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            model = getattr(R.mod(m), cls)(name=d, num_classes=C)
        D = PC.hf_geometry(family)["hidden"]
        model.classifier = nn.Sequential(nn.Linear(D, D), nn.GELU(), nn.Linear(D, C))     # the reference's head at the tiny width
        record_params(out, case, [(n, p) for n, p in model.named_parameters() if not n.startswith("classifier")])
        model.load_state_dict(PC.hf_head(case), strict=False)
        model.eval()
        x = PC.hf_input(case)
        with torch.no_grad():
            o = model(x if family == "bert" else torch.from_numpy(x))
        out[f"{case}/eval_logits"], out[f"{case}/eval_feat"] = o["logits"].numpy(), o["feat"].numpy()


def main():
    torch.manual_seed(0)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        gen_vit(out, tmp)
        gen_wrn(out, tmp)
        gen_hf(out, tmp)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
