"""Pretrained weights from local checkpoints (semireward_amd/nets/pretrained.py) on the CPU: where they are looked up, the reference's key
rules, the pos_embed resample, the refusals and the train settings taken from config.json.  The expected tensors are the reference's own
loads of the same synthetic files (tests/golden/pretrained.npz, tools/gen_pretrained_golden.py).  The backbones are built on the CPU with
the refresh of their bf16 operand copies (a HIP launch) switched off: only the fp32 block is compared here."""
import json
import os
import types

import numpy as np
import pytest
import torch

import _pretrained_ckpt as PC
from semireward_amd.core.algorithmbase import AlgorithmBase
from semireward_amd.nets import bert, hubert, pretrained, vit, wave2vec, wrn
from semireward_amd.nets.surface import ModuleSurface

VIT_URL = "https://example.invalid/releases/download/v.0.0.0/vit_small_patch2_32_mlp_im_1k_32.pth"
BUILDERS = {"vit_small_patch2_32": vit.vit_small_patch2_32, "vit_base_patch16_96": vit.vit_base_patch16_96,
            "bert_tiny_test": bert.bert_tiny_test, "wave2vecv2_tiny_test": wave2vec.wave2vecv2_tiny_test,
            "hubert_tiny_test": hubert.hubert_tiny_test}


@pytest.fixture(autouse=True)
def cpu_env(monkeypatch, tmp_path):
    monkeypatch.setattr(ModuleSurface, "refresh_operands", lambda self: None)
    monkeypatch.setattr(wrn.WideResNet, "refresh_operands", lambda self: None)
    monkeypatch.setenv("TORCH_HOME", str(tmp_path / "torch"))
    monkeypatch.setenv("HF_HUB_CACHE", str(tmp_path / "hf_hub"))
    monkeypatch.delenv("HF_HOME", raising=False)


def hf_dir(tmp_path, g, case, config=None):
    cj = str(g[f"{case}/config_json"])
    if config is not None:
        cj = json.dumps(config(json.loads(cj)))
    return PC.write_hf_dir(str(tmp_path / case), case, cj)


# ---- ViT / WRN ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(PC.VIT_CASES))
def test_pos_embed_resample_bit_equal_to_reference(golden, case):
    g = golden("pretrained")
    ck = PC.vit_checkpoint(case)
    src = ck["model"][PC.VIT_CASES[case][6] + "pos_embed"]
    out = pretrained.resize_pos_embed(src, PC.vit_pos_embed_shape(case))
    digest, sample = PC.loaded_reference(g, case)["pos_embed"]
    assert tuple(out.shape) == PC.vit_pos_embed_shape(case)
    np.testing.assert_array_equal(PC.tensor_sample(out), sample)
    assert PC.tensor_digest(out) == digest


def test_vit_local_file(golden, tmp_path):
    g, case = golden("pretrained"), "s2_32_from_s2_28"
    path = str(tmp_path / "ckpt.pth")
    torch.save(PC.vit_checkpoint(case), path)
    m = vit.vit_small_patch2_32(num_classes=10, device="cpu", pretrained=True, pretrained_path=path)
    PC.assert_loaded(m, g, case)                # pos_embed (resampled) included, in full


def test_vit_url_from_torch_hub_cache_and_key_lists(golden, tmp_path):
    g, case = golden("pretrained"), "s2_32_same_grid"
    torch.save(PC.vit_checkpoint(case), PC.torch_hub_file(str(tmp_path / "torch"), VIT_URL))
    m = vit.vit_small_patch2_32(num_classes=10, device="cpu", pretrained=True, pretrained_path=VIT_URL)
    PC.assert_loaded(m, g, case)                # pos_embed (resampled) included, in full
    # strict=False: the reference's missing / unexpected lists (its head is dropped, the extra mask_token ignored)
    fresh = vit.vit_small_patch2_32(num_classes=10, device="cpu")
    missing, unexpected = pretrained.load_weights(fresh, pretrained.checkpoint_state_dict(PC.vit_checkpoint(case), fresh))
    assert missing == list(g[f"{case}/missing"]) and unexpected == list(g[f"{case}/unexpected"])
    np.testing.assert_array_equal(fresh.view("head.weight").numpy(), vit.vit_small_patch2_32(num_classes=10, device="cpu").view("head.weight").numpy())


def test_wrn_checkpoint_params_and_buffers(golden, tmp_path):
    g, tag = golden("pretrained"), PC.WRN_CASE[0]
    path = str(tmp_path / "wrn.pth")
    torch.save(PC.wrn_checkpoint(), path)
    m = wrn.wrn_28_2(num_classes=100, device="cpu", pretrained=True, pretrained_path=path)
    PC.assert_loaded(m, g, tag)
    assert int(m.buffers["bn1.num_batches_tracked"]) == 1234
    fresh = wrn.wrn_28_2(num_classes=100, device="cpu")
    missing, unexpected = pretrained.load_weights(fresh, pretrained.checkpoint_state_dict(PC.wrn_checkpoint(), fresh))
    assert sorted(missing) == sorted(g[f"{tag}/missing"]) and sorted(unexpected) == sorted(g[f"{tag}/unexpected"])


def test_not_found_warns_and_keeps_the_random_init(capsys, tmp_path):
    m = vit.vit_small_patch2_32(num_classes=10, device="cpu", pretrained=True, pretrained_path=VIT_URL)
    err = capsys.readouterr().err.strip().splitlines()
    cached = os.path.join(str(tmp_path / "torch"), "hub", "checkpoints", "vit_small_patch2_32_mlp_im_1k_32.pth")
    assert len(err) == 1 and "not found" in err[0] and VIT_URL in err[0] and cached in err[0]
    assert torch.equal(m.flat, vit.vit_small_patch2_32(num_classes=10, device="cpu").flat)
    b = bert.bert_tiny_test(num_classes=4, device="cpu", pretrained=True, pretrained_path=str(tmp_path / "nothing"))
    err = capsys.readouterr().err.strip().splitlines()
    assert len(err) == 1 and "not found" in err[0] and str(tmp_path / "nothing") in err[0]
    assert torch.equal(b.flat, bert.bert_tiny_test(num_classes=4, device="cpu").flat)
    assert capsys.readouterr().err == ""            # a tiny test builder without a path looks nowhere and says nothing


def test_shape_mismatch_raises(tmp_path):
    path = str(tmp_path / "b16.pth")
    torch.save(PC.vit_checkpoint("b16_96_from_b16_224"), path)                  # D = 768 into a D = 384 model
    with pytest.raises(RuntimeError, match="size mismatch"):
        vit.vit_small_patch2_32(num_classes=10, device="cpu", pretrained=True, pretrained_path=path)
    m = vit.vit_tiny_test(num_classes=10, device="cpu")
    before = m.flat.clone()
    with pytest.raises(RuntimeError, match="size mismatch for blocks.0.attn.qkv.weight"):
        pretrained.load_weights(m, {"norm.weight": torch.zeros(128), "blocks.0.attn.qkv.weight": torch.zeros(128, 3 * 128)})   # same numel
    assert torch.equal(m.flat, before)               # checked before anything is written


# ---- transformers snapshots --------------------------------------------------------------------------------------------------------------
def test_hf_resolution_order(tmp_path, monkeypatch):
    cache = str(tmp_path / "hf_hub")
    assert pretrained.find_snapshot("bert-base-uncased")[0] is None
    snap = PC.hub_snapshot_dir(cache, "bert-base-uncased")
    assert pretrained.find_snapshot("bert-base-uncased")[0] is None          # no config.json / weights yet
    for f in ("config.json", "model.safetensors"):
        open(os.path.join(snap, f), "w").close()
    assert pretrained.find_snapshot("bert-base-uncased") == (snap, [snap])
    own = tmp_path / "mine"
    own.mkdir()
    for f in ("config.json", "pytorch_model.bin"):
        (own / f).write_text("")
    assert pretrained.find_snapshot("bert-base-uncased", str(own))[0] == str(own)          # pretrained_path first
    assert pretrained.find_snapshot("bert-base-uncased", str(tmp_path / "missing"))[0] == snap
    monkeypatch.delenv("HF_HUB_CACHE")
    monkeypatch.setenv("HF_HOME", str(tmp_path / "hf_home"))
    assert pretrained.find_snapshot("facebook/hubert-base-ls960")[0] is None
    s2 = PC.hub_snapshot_dir(str(tmp_path / "hf_home" / "hub"), "facebook/hubert-base-ls960")
    assert s2.endswith(os.path.join("models--facebook--hubert-base-ls960", "snapshots", "0123456789abcdef0123456789abcdef01234567"))
    for f in ("config.json", "model.safetensors"):
        open(os.path.join(s2, f), "w").close()
    assert pretrained.find_snapshot("facebook/hubert-base-ls960")[0] == s2


@pytest.mark.parametrize("case", list(PC.HF_CASES))
def test_hf_key_styles_load_like_from_pretrained(golden, tmp_path, case):
    g = golden("pretrained")
    family, style, builder, C = PC.HF_CASES[case][:4]
    d = hf_dir(tmp_path, g, case)
    m = BUILDERS[builder](num_classes=C, device="cpu", pretrained_path=d)
    PC.assert_loaded(m, g, case)
    init = BUILDERS[builder](num_classes=C, device="cpu")
    for n in ("classifier.0.weight", "classifier.2.bias"):                           # the classifier stays at init
        assert torch.equal(m.view(n), init.view(n))
    sd = pretrained.read_snapshot(d)[1]
    missing, unexpected = pretrained.load_weights(init, pretrained.hf_state_dict(sd, family))
    assert missing == [n for n, _ in init.names_shapes if n.startswith("classifier.")]
    assert unexpected == []                      # task heads, position_ids dropped; BERT's pooler is a (gradient-free) engine parameter too


def test_hf_normalisation_rules():
    sd = {"bert.embeddings.LayerNorm.gamma": 1, "bert.embeddings.LayerNorm.beta": 2, "bert.embeddings.position_ids": 3, "cls.predictions.bias": 4,
          "bert.encoder.layer.0.output.dense.weight": 5}
    assert pretrained.hf_state_dict(sd, "bert") == {"bert.embeddings.LayerNorm.weight": 1, "bert.embeddings.LayerNorm.bias": 2,
                                                    "bert.encoder.layer.0.output.dense.weight": 5}
    sd = {"wav2vec2.encoder.pos_conv_embed.conv.weight_g": 1, "wav2vec2.encoder.pos_conv_embed.conv.weight_v": 2, "lm_head.weight": 3,
          "quantizer.codevectors": 4, "project_q.weight": 5, "project_hid.bias": 6, "wav2vec2.masked_spec_embed": 7}
    assert pretrained.hf_state_dict(sd, "wav2vec2") == {"model.encoder.pos_conv_embed.conv.parametrizations.weight.original0": 1,
                                                        "model.encoder.pos_conv_embed.conv.parametrizations.weight.original1": 2,
                                                        "model.masked_spec_embed": 7}
    assert pretrained.hf_state_dict({"feature_projection.projection.bias": 1, "hubert.encoder.layer_norm.weight": 2}, "hubert") == \
        {"model.feature_projection.projection.bias": 1, "model.encoder.layer_norm.weight": 2}


def test_safetensors_reader_matches_the_library(tmp_path):
    sd = PC.hf_state_dict("w2v_new")
    p = str(tmp_path / "m.safetensors")
    PC.write_safetensors(p, sd)
    back = pretrained.read_safetensors(p)
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)


def test_train_settings_come_from_config_json(golden, tmp_path):
    g = golden("pretrained")
    b = bert.bert_tiny_test(num_classes=4, device="cpu", pretrained_path=hf_dir(tmp_path, g, "bert_new"))
    assert b.cfg.p_drop == 0.15 and b.cfg.p_head == 0.1 and b.enc_p == dict(attn=0.15, hidden=0.15, act=0.0)
    assert bert.bert_tiny_test(num_classes=4, device="cpu").cfg.p_head == 0.1
    for case in ("w2v_new", "hubert_legacy"):
        w = (wave2vec.wave2vecv2_tiny_test if case.startswith("w2v") else hubert.hubert_tiny_test)(
            num_classes=4, device="cpu", pretrained_path=hf_dir(tmp_path, g, case))
        c = w.cfg
        assert (c.p_hidden, c.p_attn, c.p_act, c.p_featproj, c.layerdrop) == (0.12, 0.08, 0.05, 0.03, 0.07)
        assert (c.mask_time_prob, c.mask_time_length, c.mask_time_min_masks, c.p_head) == (0.065, 5, 1, 0.1)
        assert w.enc_p == dict(attn=0.08, hidden=0.12, act=0.05)
    w = wave2vec.wave2vecv2_tiny_test(num_classes=4, device="cpu",
                                      pretrained_path=hf_dir(tmp_path, g, "w2v_legacy", lambda c: dict(c, apply_spec_augment=False)))
    assert w.cfg.mask_time_prob == 0.0


@pytest.mark.parametrize("case,field,value", [("bert_new", "hidden_size", 256), ("bert_legacy", "vocab_size", 30522),
                                              ("bert_new", "hidden_act", "gelu_new"), ("w2v_new", "conv_bias", True),
                                              ("w2v_legacy", "conv_kernel", [10, 3, 3]), ("hubert_new", "feat_extract_norm", "layer"),
                                              ("hubert_legacy", "do_stable_layer_norm", True), ("w2v_new", "num_conv_pos_embeddings", 128)])
def test_config_geometry_mismatch_is_refused(golden, tmp_path, case, field, value):
    g = golden("pretrained")
    family, _, builder, C = PC.HF_CASES[case][:4]
    d = hf_dir(tmp_path, g, case, lambda c: dict(c, **{field: value}))
    with pytest.raises(NotImplementedError, match=field):
        BUILDERS[builder](num_classes=C, device="cpu", pretrained_path=d)


def test_bert_unequal_dropout_is_refused(golden, tmp_path):
    g = golden("pretrained")
    d = hf_dir(tmp_path, g, "bert_new", lambda c: dict(c, attention_probs_dropout_prob=0.2))
    with pytest.raises(NotImplementedError, match="attention_probs_dropout_prob"):
        bert.bert_tiny_test(num_classes=4, device="cpu", pretrained_path=d)


def test_hub_names_of_the_reference_builders(tmp_path, monkeypatch):
    """Every encoder builder looks up its reference model name in the hub cache, whatever ``pretrained`` says."""
    seen = []
    monkeypatch.setattr(pretrained, "find_hf_weights", lambda model_name, name, path: seen.append((name, path)) or None)
    monkeypatch.setattr(bert, "ClassificationBert", lambda cfg, device: types.SimpleNamespace(init_weights=lambda seed: None))
    monkeypatch.setattr(wave2vec, "ClassificationWave2Vec", lambda cfg, device: types.SimpleNamespace(init_weights=lambda seed: None))
    monkeypatch.setattr(hubert, "ClassificationHubert", lambda cfg, device: types.SimpleNamespace(init_weights=lambda seed: None))
    bert.bert_base_uncased(device="cpu")
    bert.bert_base_cased(device="cpu", pretrained=False, pretrained_path="/x")
    wave2vec.wave2vecv2_base(device="cpu")
    hubert.hubert_base(device="cpu", pretrained=True)
    assert seen == [("bert-base-uncased", None), ("bert-base-cased", "/x"), ("facebook/wav2vec2-base-960h", None), ("facebook/hubert-base-ls960", None)]


# ---- the algorithm -----------------------------------------------------------------------------------------------------------------------
def test_set_model_passes_pretrain_keys_only_when_use_pretrain():
    calls = []

    def builder(num_classes, device, **kw):
        calls.append(kw)
        return types.SimpleNamespace(refresh_operands=lambda: None)

    alg = types.SimpleNamespace(net_builder=builder, num_classes=10, device="cpu", args=types.SimpleNamespace(use_pretrain=True, pretrain_path=VIT_URL))
    AlgorithmBase.set_model(alg)
    alg.args = types.SimpleNamespace(use_pretrain=False, pretrain_path=VIT_URL)
    AlgorithmBase.set_model(alg)
    alg.args = types.SimpleNamespace()
    AlgorithmBase.set_model(alg)
    assert calls == [dict(pretrained=True, pretrained_path=VIT_URL), {}, {}]
