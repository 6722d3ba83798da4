"""Pretrained weights from local checkpoints on the HIP engine: every family loaded through its public builder from files under tmp_path
(TORCH_HOME / HF_HUB_CACHE point there), against the reference's own loads of the same synthetic files (tests/golden/pretrained.npz):
every loaded tensor of the fp32 block bit for bit (SHA-256 digests, the resampled ``pos_embed`` included), eval logits / features within the tolerances of the family's
golden test, and the algorithm path (``use_pretrain`` / hub cache -> model and EMA model -> one train step)."""
import argparse
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _pretrained_ckpt as PC                       # noqa: E402
from oracle import bert_ref as BR                  # noqa: E402
from semireward_amd.nets import bert, hubert, vit, wave2vec, wrn   # noqa: E402
from semireward_amd.utils import synth             # noqa: E402

DEV = "cuda:0"
VIT_URL = "https://example.invalid/releases/download/v.0.0.0/vit_small_patch2_32_mlp_im_1k_32.pth"
BUILDERS = {"vit_small_patch2_32": vit.vit_small_patch2_32, "vit_base_patch16_96": vit.vit_base_patch16_96,
            "bert_tiny_test": bert.bert_tiny_test, "wave2vecv2_tiny_test": wave2vec.wave2vecv2_tiny_test,
            "hubert_tiny_test": hubert.hubert_tiny_test}
# the tolerances of the family's golden test (test_gpu_vit.py, test_gpu_wrn.py, test_gpu_bert.py, test_gpu_w2v.py): (logits, features)
TOL = {"vit": (2e-2, 2e-2), "wrn": (2.5e-2, 2.5e-2), "bert": (4e-2, 2e-2), "wav2vec2": (4e-2, 2.5e-2), "hubert": (4e-2, 2.5e-2)}


@pytest.fixture(autouse=True)
def caches(monkeypatch, tmp_path):
    monkeypatch.setenv("TORCH_HOME", str(tmp_path / "torch"))
    monkeypatch.setenv("HF_HUB_CACHE", str(tmp_path / "hf_hub"))
    monkeypatch.delenv("HF_HOME", raising=False)


def rel(a, b):
    a = a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


@pytest.mark.parametrize("case", list(PC.VIT_CASES))
def test_vit_pretrained_matches_reference(golden, tmp_path, case):
    g = golden("pretrained")
    _, _, builder, C, _, _, _ = PC.VIT_CASES[case]
    if case == "s2_32_same_grid":                  # a URL: the file torch.hub would have cached
        torch.save(PC.vit_checkpoint(case), PC.torch_hub_file(str(tmp_path / "torch"), VIT_URL))
        path = VIT_URL
    else:
        path = str(tmp_path / (case + ".pth"))
        torch.save(PC.vit_checkpoint(case), path)
    m = BUILDERS[builder](num_classes=C, device=DEV, pretrained=True, pretrained_path=path)
    PC.assert_loaded(m, g, case)                   # every loaded tensor bit-equal, the resampled pos_embed included
    m.load_state_dict(PC.vit_head(case), strict=False)
    m.eval()
    lg, ft, _ = m.forward_features(torch.from_numpy(PC.vit_input(case)).to(DEV), None, None, save=False)
    tl, tf = TOL["vit"]
    assert rel(lg, g[f"{case}/eval_logits"]) < tl and rel(ft, g[f"{case}/eval_feat"]) < tf


def test_wrn_pretrained_matches_reference(golden, tmp_path):
    g, (tag, _, C, _, _, _) = golden("pretrained"), PC.WRN_CASE
    path = str(tmp_path / "wrn.pth")
    torch.save(PC.wrn_checkpoint(), path)
    m = wrn.wrn_28_2(num_classes=C, device=DEV, pretrained=True, pretrained_path=path)
    PC.assert_loaded(m, g, tag)
    m.load_state_dict(PC.wrn_head(), strict=False)
    m.eval()
    lg, ft, _ = m.forward_features(torch.from_numpy(PC.wrn_input()).to(DEV))
    tl, tf = TOL["wrn"]
    assert rel(lg, g[f"{tag}/eval_logits"]) < tl and rel(ft, g[f"{tag}/eval_feat"]) < tf


@pytest.mark.parametrize("case", list(PC.HF_CASES))
def test_hf_pretrained_matches_reference(golden, tmp_path, case):
    g = golden("pretrained")
    family, _, builder, C = PC.HF_CASES[case][:4]
    d = PC.write_hf_dir(str(tmp_path / case), case, str(g[f"{case}/config_json"]))
    m = BUILDERS[builder](num_classes=C, device=DEV, pretrained_path=d)
    PC.assert_loaded(m, g, case)
    m.load_state_dict(PC.hf_head(case), strict=False)
    m.eval()
    x = PC.hf_input(case)
    o = m({k: v.to(DEV) for k, v in x.items()} if family == "bert" else torch.from_numpy(x).to(DEV))
    tl, tf = TOL[family]
    assert rel(o["logits"], g[f"{case}/eval_logits"]) < tl and rel(o["feat"], g[f"{case}/eval_feat"]) < tf


def _common_args(**kw):
    return argparse.Namespace(num_train_iter=100, epoch=1, ema_m=0.999, ulb_loss_ratio=1.0, amp=False, lr=5e-4, weight_decay=5e-4,
                              layer_decay=0.65, num_warmup_iter=0, optim="AdamW", T=0.5, hard_label=True, ulb_dest_len=256, N_k=10,
                              start_timing=5, sr_lr=5e-4, sr_ema=False, sr_ema_m=0.99, gpu=0, rank=0, world_size=1, distributed=False, **kw)


def test_vit_algorithm_starts_from_the_torch_hub_cache(golden, tmp_path):
    from semireward_amd.algorithms import get_algorithm
    g, case = golden("pretrained"), "s2_32_same_grid"
    torch.save(PC.vit_checkpoint(case), PC.torch_hub_file(str(tmp_path / "torch"), VIT_URL))
    args = _common_args(algorithm="srflexmatch", num_classes=10, use_cat=True, p_cutoff=0.95, thresh_warmup=True, feature_dim=384,
                        use_pretrain=True, pretrain_path=VIT_URL)
    alg = get_algorithm(args, vit.vit_small_patch2_32)
    assert alg.ema_model is not alg.model
    for m in (alg.model, alg.ema_model):
        PC.assert_loaded(m, g, case)
    assert torch.equal(alg.ema_model.flat, alg.model.flat)
    b = synth.synth_batch(1, 4, 4, 32, 10, 256)
    before = alg.model.flat.clone()
    out, log = alg.train_step(**alg.process_batch(**{k: torch.from_numpy(v) for k, v in b.items()}))
    alg.out_dict, alg.log_dict = out, log
    alg.call_hook("after_train_step")               # the optimizer step (ParamUpdateHook)
    torch.cuda.synchronize()
    assert np.isfinite(float(log["train/total_loss"])) and not torch.equal(alg.model.flat, before)


def test_bert_algorithm_starts_from_the_hf_hub_cache(golden, tmp_path):
    """The hub-cache snapshot of ``bert-base-uncased`` holding the tiny test geometry (a builder with that reference name at the tiny
    width): model and EMA model start from it, with its dropout, and a train step runs."""
    from semireward_amd.algorithms import get_algorithm
    g, case = golden("pretrained"), "bert_new"
    cj = json.loads(str(g[f"{case}/config_json"]))
    snap = PC.hub_snapshot_dir(str(tmp_path / "hf_hub"), "bert-base-uncased")
    PC.write_hf_dir(snap, case, json.dumps(cj))
    builder = lambda num_classes, device, **kw: bert._build(num_classes, dict(kw, device=device), hub_name="bert-base-uncased",   # noqa: E731
                                                            **BR.BERT_TINY_TEST)
    C = PC.HF_CASES[case][3]
    args = _common_args(algorithm="srsoftmatch", num_classes=C, use_cat=False, ema_p=0.5, n_sigma=2, dist_uniform=True, dist_align=True,
                        per_class=False, feature_dim=128)
    alg = get_algorithm(args, builder)
    assert alg.ema_model is not alg.model
    for m in (alg.model, alg.ema_model):
        PC.assert_loaded(m, g, case)
        assert m.cfg.p_drop == cj["hidden_dropout_prob"] and m.cfg.p_head == 0.1
    assert torch.equal(alg.ema_model.flat, alg.model.flat)
    dx = lambda b: {"input_ids": torch.from_numpy(b[0]), "attention_mask": torch.from_numpy(b[1])}   # noqa: E731
    lb, w, s_ = (BR.synth_tokens(900 + j, B, L, BR.BERT_TINY_TEST["vocab"]) for j, (B, L) in enumerate(((3, 20), (5, 24), (5, 17))))
    y = torch.from_numpy(np.arange(3, dtype=np.int64) % C)
    before = alg.model.flat.clone()
    out, log = alg.train_step(**alg.process_batch(x_lb=dx(lb), y_lb=y, x_ulb_w=dx(w), x_ulb_s=dx(s_)))
    alg.out_dict, alg.log_dict = out, log
    alg.call_hook("after_train_step")
    torch.cuda.synchronize()
    assert np.isfinite(float(log["train/total_loss"])) and not torch.equal(alg.model.flat, before)


def test_not_found_keeps_the_random_init_on_the_gpu(capsys):
    m = vit.vit_small_patch2_32(num_classes=10, device=DEV, pretrained=True, pretrained_path=VIT_URL)
    assert "not found" in capsys.readouterr().err
    ref = vit.vit_small_patch2_32(num_classes=10, device=DEV)
    assert torch.equal(m.flat, ref.flat) and torch.equal(m.flat_bf16, ref.flat_bf16)
