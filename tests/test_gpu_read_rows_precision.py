"""read_rows_precision = bf16x3 on the GPU: the split-bf16 kernels (csrc/x3.hip) against fp64, the ViT forward of the read rows against
the reference's golden vectors, the mask decisions of the reference sweep, which rows the mode touches, and the captured step."""
import argparse
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_srflexmatch as TS                                         # noqa: E402  (measure_mask_identity, used as it is)
import test_gpu_stepgraph as TG                                           # noqa: E402  (the captured-step helpers)
from oracle import vit_ref as V                                           # noqa: E402
from semireward_amd import ops                                            # noqa: E402
from semireward_amd.algorithms import get_algorithm, srflexmatch as SF   # noqa: E402
from semireward_amd.nets import vit                                       # noqa: E402
from semireward_amd.utils import synth                                    # noqa: E402

DEV = "cuda:0"
GEMM_REL = 1e-5           # bf16x3 against fp64 (bf16 gemm_nt: 2.3e-3)
ATTN_REL = 2e-5           # two chained bf16x3 products
FWD_REL = 1e-4            # whole forward against the fp32 reference's golden vectors (CPU model of the mode: <= 1.3e-5; bf16 path: 2e-2)


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def _randn(*shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


# (M, N, K, epilogue): the products of the three ViT configs' blocks (qkv, proj, fc1, fc2; patch embedding at 224) and of the tiny config, at
# 8 and 72 images of 257 tokens (the read launch of the reference batch) and at ragged M
X3_SHAPES = []
for D in (384, 768):
    for M in (2056, 18504, 37 * 5 + 3):
        X3_SHAPES += [(M, 3 * D, D, ops.X3_EPI_F32), (M, D, D, ops.X3_EPI_RESID_F32), (M, 4 * D, D, ops.X3_EPI_GELU_F32),
                      (M, D, 4 * D, ops.X3_EPI_RESID_F32)]
X3_SHAPES += [(197 * 3 - 3 * 3, 384, 768, ops.X3_EPI_F32), (17 * 6, 384, 128, ops.X3_EPI_F32), (17 * 6, 128, 512, ops.X3_EPI_RESID_F32),
              (17 * 6, 512, 128, ops.X3_EPI_GELU_F32)]


@pytest.mark.parametrize("M,N,K,epi", X3_SHAPES)
def test_gemm_nt_x3_against_fp64(M, N, K, epi):
    A, W = _randn(M, K, seed=M + K), _randn(N, K, seed=N + 7, scale=K ** -0.5)
    bias = _randn(N, seed=3, scale=0.1)
    ref = A.double() @ W.double().t() + bias.double()
    rps = 257 if M % 257 == 0 else 1
    if epi == ops.X3_EPI_RESID_F32:
        C0 = _randn(M, N, seed=11)
        nsamp = M // rps
        s = torch.rand(nsamp, generator=torch.Generator().manual_seed(5)).to(DEV) * 1.5
        s[::3] = 0.0                                                     # dropped paths
        outs = []
        for _ in range(2):
            C = C0.clone()
            ops.gemm_nt_x3(epi, A, W, C, M, N, K, bias=bias, row_scale=s, rows_per_sample=rps)
            outs.append(C)
        want = s.double().repeat_interleave(rps)[:, None] * ref
        got = outs[0].double() - C0.double()
        keep = (s.repeat_interleave(rps) != 0)
        assert torch.equal(outs[0][~keep], C0[~keep])                    # a dropped path leaves the residual bit for bit
        err = rel(got[keep], want[keep])
    else:
        outs = []
        for _ in range(2):
            C = torch.full((M, N), float("nan"), device=DEV)
            ops.gemm_nt_x3(epi, A, W, C, M, N, K, bias=bias)
            outs.append(C)
        if epi == ops.X3_EPI_GELU_F32:
            ref = torch.nn.functional.gelu(ref)
        err = rel(outs[0], ref)
    torch.cuda.synchronize()
    print("GEMM_X3 M=%d N=%d K=%d epi=%d rel-L2 vs fp64 %.2e" % (M, N, K, epi, err))
    assert err <= GEMM_REL, err
    assert torch.equal(outs[0], outs[1])                                 # deterministic


def test_gemm_nt_x3_gains_over_bf16_operands():
    """The same product through today's bf16-operand gemm_nt: three orders of magnitude apart."""
    M, N, K = 2056, 1152, 384
    A, W = _randn(M, K, seed=1), _randn(N, K, seed=2, scale=K ** -0.5)
    ref = A.double() @ W.double().t()
    C3 = torch.empty(M, N, device=DEV)
    ops.gemm_nt_x3(ops.X3_EPI_F32, A, W, C3, M, N, K)
    Cb = torch.empty(M, N, device=DEV)
    ops.gemm_nt(ops.EPI_F32, A.to(torch.bfloat16), W.to(torch.bfloat16), Cb, M, N, K)
    e3, eb = rel(C3, ref), rel(Cb, ref)
    print("GEMM x3 %.2e, bf16 operands %.2e" % (e3, eb))
    assert e3 * 100 < eb


@pytest.mark.parametrize("N,H", [(257, 6), (197, 6), (37, 12), (17, 2)])
def test_attn_fwd_x3_against_fp64(N, H):
    # measured on MI355X: see the ATTN_X3 lines of the run (two chained bf16x3 products: ~5e-6)
    B, D = 3, H * 64
    qkv = _randn(B * N, 3 * D, seed=N + H)
    out = torch.full((B * N, D), float("nan"), device=DEV)
    ops.attn_fwd_x3(qkv, out, B, N, H, 64 ** -0.5)
    q, k, v = qkv.double().view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    ref = (torch.softmax((q @ k.transpose(-2, -1)) * 64 ** -0.5, dim=-1) @ v).transpose(1, 2).reshape(B * N, D)
    out2 = torch.empty_like(out)
    ops.attn_fwd_x3(qkv, out2, B, N, H, 64 ** -0.5)
    err = rel(out, ref)
    print("ATTN_X3 N=%d H=%d rel-L2 vs fp64 %.2e" % (N, H, err))
    assert err <= ATTN_REL, err
    assert torch.equal(out, out2)


@pytest.mark.parametrize("tag", ["tiny", "small_p2_32", "small_p16_224", "base_p16_96"])
def test_forward_features_bf16x3_matches_reference_golden(golden, tag):
    g = golden({"small_p16_224": "vit_p16", "base_p16_96": "vit_b16_96"}.get(tag, "vit"))
    C, B, seed = [int(v) for v in g[f"{tag}/meta"]]
    model, cfg = _build(tag)
    P = synth.synth_params(V.param_shapes(cfg), seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    x = torch.from_numpy(rng.standard_normal((B, 3, cfg.img_size, cfg.img_size)).astype(np.float32)).to(DEV)
    dp = torch.from_numpy(synth.synth_droppath(seed + 2, V.drop_path_probs(cfg), B)).to(DEV)
    lg, ft, ctx = model.forward_features(x, None, None, save=False, precision="bf16x3")
    assert ctx is None
    e = (rel(lg, g[f"{tag}/eval_logits"]), rel(ft, g[f"{tag}/eval_feat"]))
    lg2, ft2, _ = model.forward_features(x, None, dp, save=False, precision="bf16x3")
    t = (rel(lg2, g[f"{tag}/train_logits"]), rel(ft2, g[f"{tag}/train_feat"]))
    lgb, _, _ = model.forward_features(x, None, dp, save=False)
    eb = rel(lgb, g[f"{tag}/train_logits"])
    print("FWD_X3 %s: eval logits %.2e feats %.2e, train logits %.2e feats %.2e (bf16 path: %.2e)" % (tag, *e, *t, eb))
    assert max(e + t) <= FWD_REL, (e, t)
    assert max(t) * 50 < eb
    # rows permuted through img_index: permuted outputs, bit for bit
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).to(DEV)
    lg3, ft3, _ = model.forward_features(x, perm.to(torch.int32), dp[:, :, perm].contiguous(), save=False, precision="bf16x3")
    assert torch.equal(lg3, lg2[perm]) and torch.equal(ft3, ft2[perm])
    # the scattering head writes the same rows
    L, F = torch.zeros(B + 2, C, device=DEV), torch.zeros(B + 2, cfg.embed_dim, device=DEV)
    rows = (torch.arange(B, device=DEV) + 2).to(torch.int64)
    model.forward_features(x, None, dp, save=False, precision="bf16x3", out=(L, F, rows))
    assert torch.equal(L[2:], lg2) and torch.equal(F[2:], ft2)
    with pytest.raises(AssertionError):
        model.forward_features(x, None, dp, save=True, precision="bf16x3")


def _build(tag):
    if tag == "tiny":
        return vit.vit_tiny_test(num_classes=10, device=DEV), V.VitCfg(num_classes=10, **V.VIT_TINY_TEST)
    if tag == "small_p16_224":
        return vit.vit_small_patch16_224(num_classes=100, device=DEV), V.VitCfg(num_classes=100, **V.VIT_SMALL_P16_224)
    if tag == "base_p16_96":
        return vit.vit_base_patch16_96(num_classes=10, device=DEV), V.VitCfg(num_classes=10, **V.VIT_BASE_P16_96)
    return vit.vit_small_patch2_32(num_classes=100, device=DEV), V.VitCfg(num_classes=100, **V.VIT_SMALL_P2_32)


# bounds of the mode over the 96 steps of the reference sweep (bf16 operands: max-prob deviation 0.081 at gain 24, 4.4e-4 at gain 1)
X3_MASK_BOUNDS = {24.0: 1e-3, 1.0: 5e-6}


@pytest.mark.parametrize("gain", [24.0, 1.0])
def test_bf16x3_mask_identity_over_the_reference_sweep(golden, gain, monkeypatch):
    monkeypatch.setenv("SR_READ_ROWS_PRECISION", "bf16x3")
    g = golden("srflexmatch_full_sweep")
    st = TS.measure_mask_identity(g, gain)
    line = "MASK_IDENTITY_X3 gain %g: %s" % (gain, json.dumps({k: v for k, v in st.items() if k != "first"}))
    print(line)
    print("MASK_IDENTITY_X3 first differing rows (batch, it, pass, row, same label, ref max-prob, engine max-prob, threshold, ref gap):", st["first"])
    assert st["steps"] == 96 and st["rows"] == 48 * (8 + 72)
    assert st["first_mask_flips_inside_their_room"] == 0, [x for x in st["first"] if x[4]]
    assert st["mask2_flips_clear"] == 0, line
    assert st["max_dev_same_label"] <= X3_MASK_BOUNDS[gain], line
    assert st["flipped_rows"] + st["label_mismatch_rows"] <= 2, line
    for (_, _, _, _, same, refp, mpv, _, gap) in st["first"]:
        if not same:                                                     # a label flip only where the reference's top-two gap is that small
            assert gap <= 2.0 * st["max_dev_same_label"], line


NSa = dict(TG.NSa)


def _alg(precision, monkeypatch, it0=30008):
    monkeypatch.setattr(SF, "_DEFER_AUTOTUNE", False)
    alg = get_algorithm(argparse.Namespace(**NSa, read_rows_precision=precision), vit.vit_small_patch2_32)
    alg.model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_params(alg.model.names_shapes, 0).items()})
    alg.model.seed = 4321
    alg.it = it0
    alg.optimizer.sched_step = it0
    return alg


def test_bf16x3_touches_exactly_the_read_columns(monkeypatch):
    """One training step with the mode off and one with it on, same state, same batch, same DropPath: the gradient columns and the deferred ones
    are bit for bit the same, the unread columns _Plan moved into the read launch as well (their own bf16 launch, same kernels), the read
    columns are not."""
    cfg = V.VitCfg(num_classes=100, **V.VIT_SMALL_P2_32)
    b = synth.synth_batch(101, 8, 8, 32, 100, 50000)
    dps = [torch.from_numpy(synth.synth_droppath(700 + k, V.drop_path_probs(cfg), 24)) for k in range(9)]
    res = {}
    for prec in ("bf16", "bf16x3"):
        alg = _alg(prec, monkeypatch)
        assert alg.read_rows_precision == prec
        alg.inject_droppath = dps
        alg.trace = {}
        alg.train_step(**alg.process_batch(**{k: torch.from_numpy(v) for k, v in b.items()}))
        torch.cuda.synchronize()
        assert alg.trace["K"] == 8
        pl = next(iter(alg._plans.values()))
        res[prec] = (alg.trace["logits"].reshape(-1, 100).clone(), alg.trace["feats"].reshape(-1, 384).clone(), pl)
    (L0, F0, p0), (L1, F1, p1) = res["bf16"], res["bf16x3"]
    assert p0.x3_cols is None and p1.x3_cols is not None
    Bt, nl, nu = 24, 8, 8
    read = torch.tensor([k * Bt + j for k in range(9) for j in range(nl, nl + nu)], device=DEV)
    assert torch.equal(torch.sort(p1.x3_cols).values, read)
    assert p1.mix_cols.numel() > 0, "the plan of the reference batch moves unread columns into the read launch"
    same = torch.cat([p1.grad_cols, p1.mix_cols, p1.rest_cols])
    assert torch.equal(L1[same], L0[same]) and torch.equal(F1[same], F0[same])
    d = (L1[read] - L0[read]).abs().amax(dim=1)
    assert bool((d > 0).all()), "every read column runs the bf16x3 chain"
    assert rel(L1[read], L0[read]) < 2e-2


def test_bf16x3_captured_step_replays_the_eager_step(monkeypatch):
    """core/stepgraph.py with the mode on: from the eager step's state the replayed step's features, masks and FlexMatch table are the eager
    step's bit for bit (the assertions of test_graph_replay_equals_eager_steps)."""
    monkeypatch.setenv("SR_READ_ROWS_PRECISION", "bf16x3")
    it0, n = 30008, 8
    a0, _ = TG._make(False, it0, monkeypatch)
    a1, sg = TG._make(True, it0, monkeypatch)
    assert a0.read_rows_precision == a1.read_rows_precision == "bf16x3"
    batches = [a0.process_batch(**{k: torch.from_numpy(v) for k, v in synth.synth_batch(700 + i, 8, 8, 32, 100, 50000).items()}) for i in range(n)]
    for i in range(n):
        before = a0.model.flat.clone()
        x, y = TG._one_step(a0, None, batches[i]), TG._one_step(a1, sg, batches[i])
        upd = float((x["flat"] - before).abs().max())
        assert torch.equal(x["feat"], y["feat"]), i
        np.testing.assert_allclose(y["loss"], x["loss"], rtol=1e-5, atol=1e-6, err_msg="step %d" % i)
        assert torch.equal(x["sel"], y["sel"]) and torch.equal(x["acc"], y["acc"]), i
        assert float((x["flat"] - y["flat"]).abs().max()) <= 2.1 * upd, i
        assert float((x["flat"] - y["flat"]).abs().mean()) <= 1e-2 * upd, i
        TG._copy_state(a1, a0)
    assert len(sg.graphs) >= 1 and sg.replays >= 1, (len(sg.graphs), sg.replays, sg.eager_steps)
