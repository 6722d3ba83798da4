"""read_rows_precision (bf16 | bf16x3) without a GPU: the C ABI and its wrappers, the register budget of csrc/x3.hip, the option's
validation, the launch plan of the mode, and a CPU model of its numerics against the reference's golden vectors."""
import argparse
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import vit_ref as V
from semireward_amd.utils import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X3_ENTRIES = ("srhip_gemm_nt_x3", "srhip_attn_fwd_x3", "srhip_layernorm_fwd_f32", "srhip_patch_im2col_f32")


def test_header_declares_the_x3_entries_and_ops_wraps_them():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srhip.h")).read(), flags=re.S)
    for n in X3_ENTRIES + ("SRHIP_X3_EPI_F32", "SRHIP_X3_EPI_GELU_F32", "SRHIP_X3_EPI_RESID_F32"):
        assert re.search(r"\b%s\b" % n, src), n
    from semireward_amd import _lib, ops
    for n in X3_ENTRIES:
        assert n in _lib.SIGNATURES, n
    for n in ("gemm_nt_x3", "attn_fwd_x3", "layernorm_fwd_f32", "patch_im2col_f32"):
        assert callable(getattr(ops, n)), n
    assert (ops.X3_EPI_F32, ops.X3_EPI_GELU_F32, ops.X3_EPI_RESID_F32) == (0, 1, 2)


def test_precise_kernels_keep_their_register_budget(tmp_path):
    """Compiled with the resource remarks on (as test_hot_kernels_keep_their_register_budget does): every kernel of csrc/x3.hip -- the seven
    instantiations of the one GEMM engine, the grouped TN kernel, both attention forwards, both attention backward kernels -- has no scratch,
    no spill and two waves per SIMD."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "semireward_amd", "csrc")
    assert sorted(f for f in os.listdir(csrc) if "x3" in f or "precise" in f) == ["x3.hip"]
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-c",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "o.o"), os.path.join(csrc, "x3.hip")],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    # gemm_x3_kernel<LA, LB, EPI> as the Itanium ABI spells its arguments: layouts ROWS = 0 / COLS = 1, the file's epilogue enum in its order
    epi = {n: i for i, n in enumerate(("F32", "ACC", "DGELU", "GELU_PRE", "GELU", "RESID"))}
    want = {"gemm_x3_kernelILi0ELi%dELi%dEE" % (lb, epi[e]) for lb, es in ((0, ("F32", "GELU", "RESID", "GELU_PRE")), (1, ("F32", "ACC", "DGELU")))
            for e in es}
    gemm = {k: v for k, v in out.items() if "gemm_x3_kernel" in k}
    assert len(gemm) == 7 and all(any(w in k for k in gemm) for w in want), sorted(out)
    assert not any("gemm_nt_x3" in k for k in out), sorted(out)
    rest = {}
    for name, n in (("gemm_tn_x3_grouped_kernel", 1), ("attn_fwd_x3_kernelILb", 2), ("attn_bwd_x3_dq_kernel", 1), ("attn_bwd_x3_dkv_kernel", 1)):
        hit = {k: v for k, v in out.items() if name in k}
        assert len(hit) == n, (name, sorted(out))
        rest.update(hit)
    assert len(out) == len(gemm) + len(rest) + 1 and any("scale_rows_f32_kernel" in k for k in out), sorted(out)
    for k, v in list(gemm.items()) + list(rest.items()):
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["Occupancy [waves/SIMD]"] >= 2, (k, v)


def _args(**kw):
    return argparse.Namespace(**kw)


def test_option_validation(monkeypatch):
    from semireward_amd.algorithms.srflexmatch import backbone_class, read_rows_precision
    from semireward_amd.nets import bert, hubert, vit, wave2vec, wrn
    monkeypatch.delenv("SR_READ_ROWS_PRECISION", raising=False)
    nets = [vit.VisionTransformer, bert.ClassificationBert, wave2vec.ClassificationWave2Vec, hubert.ClassificationHubert, wrn.WideResNet]
    for cls in nets:
        assert read_rows_precision(_args(), cls) == "bf16"
        assert read_rows_precision(_args(read_rows_precision="bf16"), cls) == "bf16"
        with pytest.raises(ValueError):
            read_rows_precision(_args(read_rows_precision="fp32"), cls)
    assert read_rows_precision(_args(read_rows_precision="bf16x3"), vit.VisionTransformer) == "bf16x3"
    for cls in nets[1:]:
        with pytest.raises(NotImplementedError, match=cls.__name__):
            read_rows_precision(_args(read_rows_precision="bf16x3"), cls)
    # the environment variable is the fallback of a missing args field (bench.py, the sweep helper), the args field wins
    monkeypatch.setenv("SR_READ_ROWS_PRECISION", "bf16x3")
    assert read_rows_precision(_args(), vit.VisionTransformer) == "bf16x3"
    assert read_rows_precision(_args(read_rows_precision="bf16"), bert.ClassificationBert) == "bf16"
    with pytest.raises(NotImplementedError):
        read_rows_precision(_args(), wrn.WideResNet)
    monkeypatch.setenv("SR_READ_ROWS_PRECISION", "half")
    with pytest.raises(ValueError):
        read_rows_precision(_args(), vit.VisionTransformer)
    # builders resolve to their engine class without being called (validation comes before any device work)
    assert backbone_class(vit.vit_small_patch2_32) is vit.VisionTransformer
    assert backbone_class(bert.bert_base_uncased) is bert.ClassificationBert
    assert backbone_class(hubert.hubert_base) is hubert.ClassificationHubert
    assert backbone_class(wave2vec.wave2vecv2_base) is wave2vec.ClassificationWave2Vec
    assert backbone_class(wrn.wrn_28_2) is wrn.WideResNet


def test_plan_splits_the_read_launch():
    """split_read: the read launch's columns are exactly the weak rows of every pass; the unread columns moved into it for tile balance form a
    launch of their own; the launch order is gradient | read | moved | deferred; without it the plan is the one the default mode uses."""
    from semireward_amd.algorithms.srflexmatch import _Plan
    nl = nu = 8
    K, Bt = 8, 24
    p = _Plan.cat_passes(nl, nu, K, "cpu", defer_unread=True, rows_per_col=257)
    q = _Plan.cat_passes(nl, nu, K, "cpu", defer_unread=True, rows_per_col=257, split_read=True)
    assert p.x3_cols is None
    for a in ("grad_cols", "inf_cols", "rest_cols", "grad_img", "inf_img", "rest_img"):
        assert torch.equal(getattr(p, a), getattr(q, a)), a
    weak = [k * Bt + j for k in range(K + 1) for j in range(nl, nl + nu)]
    assert q.x3_cols.tolist() == weak
    assert q.mix_cols.numel() > 0 and sorted(q.x3_cols.tolist() + q.mix_cols.tolist()) == q.inf_cols.tolist()
    assert q.x3_img.tolist() == [c % Bt for c in weak] and q.mix_img.tolist() == [c % Bt for c in q.mix_cols.tolist()]
    assert q.perm_cols.tolist() == q.grad_cols.tolist() + q.x3_cols.tolist() + q.mix_cols.tolist() + q.rest_cols.tolist()
    # no read list (serial schedule, SRPseudoLabel's plan): every inference column is read
    r = _Plan.cat_passes(nl, nu, K, "cpu", split_read=True)
    assert torch.equal(r.x3_cols, r.inf_cols) and r.mix_cols.numel() == 0


# ---- CPU model of the mode (numerics contract): split hi = bf16(x), lo = bf16(x - hi); product hi.hi + hi.lo + lo.hi in fp32; everything
# else fp32 in the order of oracle/vit_ref.vit_forward
def _split(t):
    hi = t.to(torch.bfloat16).float()
    return hi, (t - hi).to(torch.bfloat16).float()


def mm_x3(a, b):
    ah, al = _split(a)
    bh, bl = _split(b)
    return ah @ bl + al @ bh + ah @ bh


def vit_forward_x3(P, x, cfg, droppath=None):
    B = x.shape[0]
    D, nh = cfg.embed_dim, cfg.num_heads
    hd = D // nh
    Wp = P["patch_embed.proj.weight"].reshape(D, -1)
    pt = V.patchify(x, cfg.patch_size)
    t = (pt @ Wp.t() if Wp.shape[1] <= 64 else mm_x3(pt, Wp.t())) + P["patch_embed.proj.bias"]      # CIFAR patches: the fp32 kernel
    t = torch.cat((P["cls_token"].expand(B, -1, -1), t), dim=1) + P["pos_embed"]
    N = t.shape[1]
    lin = lambda h_, n_: mm_x3(h_, P[n_ + ".weight"].t()) + P[n_ + ".bias"]   # noqa: E731
    for i in range(cfg.depth):
        b = f"blocks.{i}."
        h = V._ln(t, P[b + "norm1.weight"], P[b + "norm1.bias"])
        q, k, v = lin(h, b + "attn.qkv").reshape(B, N, 3, nh, hd).permute(2, 0, 3, 1, 4)
        s = mm_x3(q, k.transpose(-2, -1)) * (hd ** -0.5)
        e = torch.exp(s - s.amax(dim=-1, keepdim=True))
        o = (mm_x3(e, v) / e.sum(dim=-1, keepdim=True)).transpose(1, 2).reshape(B, N, D)
        o = lin(o, b + "attn.proj")
        if droppath is not None:
            o = o * droppath[i, 0].view(B, 1, 1)
        t = t + o
        h = V._gelu(lin(V._ln(t, P[b + "norm2.weight"], P[b + "norm2.bias"]), b + "mlp.fc1"))
        h = lin(h, b + "mlp.fc2")
        if droppath is not None:
            h = h * droppath[i, 1].view(B, 1, 1)
        t = t + h
    feat = V._ln(t, P["norm.weight"], P["norm.bias"])[:, 0]
    return {"logits": feat @ P["head.weight"].t() + P["head.bias"], "feat": feat}


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_cpu_model_of_the_mode_reproduces_the_reference(golden):
    """The contract's CPU model on the tiny config (eval and injected DropPath) lands within 5e-5 of the fp32 reference's golden logits, where the
    model of today's bf16-operand rounding points (oracle.vit_ref.vit_forward_engine_rounding) sits two orders of magnitude further out."""
    g = golden("vit")
    C, B, seed = [int(v) for v in g["tiny/meta"]]
    cfg = V.VitCfg(num_classes=C, **V.VIT_TINY_TEST)
    P = {k: torch.from_numpy(v) for k, v in synth.synth_params(V.param_shapes(cfg), seed).items()}
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    x = torch.from_numpy(rng.standard_normal((B, 3, cfg.img_size, cfg.img_size)).astype(np.float32))
    dp = torch.from_numpy(synth.synth_droppath(seed + 2, V.drop_path_probs(cfg), B))
    for mode, d in (("eval", None), ("train", dp)):
        out = vit_forward_x3(P, x, cfg, d)
        e = _rel(out["logits"], g["tiny/%s_logits" % mode])
        assert e < 5e-5 and _rel(out["feat"], g["tiny/%s_feat" % mode]) < 5e-5, (mode, e)
        eb = _rel(V.vit_forward_engine_rounding(P, x, cfg, d)["logits"], g["tiny/%s_logits" % mode])
        assert e * 20 < eb, (mode, e, eb)
    # the split itself: hi + lo carries x to 2^-16 relative, the dropped lo.lo term is below 2^-16 of the product
    a = torch.randn(64, 384, dtype=torch.float32)
    hi, lo = _split(a)
    assert float(((hi + lo - a).abs() / a.abs()).max()) <= 2.0 ** -16
