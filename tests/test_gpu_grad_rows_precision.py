"""grad_rows_precision = bf16x3 on the GPU: the split-bf16 backward kernels (csrc/x3.hip) against fp64, the ViT backward of the
gradient rows against fp32 autograd, the reference step traces with both options on, and the captured step."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_srflexmatch as TS                                         # noqa: E402  (make_args, samp_of)
import test_gpu_stepgraph as TG                                           # noqa: E402  (the captured-step helpers)
from oracle import hooks_ref as Hr                                        # noqa: E402
from oracle import semireward_ref as S                                    # noqa: E402
from oracle import vit_ref as V                                           # noqa: E402
from oracle.gen_golden import TRACE, TRACE_C100, TRACE_FIX, TRACE_FREE, TRACE_SOFT   # noqa: E402
from semireward_amd import ops                                            # noqa: E402
from semireward_amd.algorithms import get_algorithm                       # noqa: E402
from semireward_amd.nets import vit                                       # noqa: E402
from semireward_amd.utils import synth                                    # noqa: E402

DEV = "cuda:0"
KERNEL_REL = 2e-5         # a bf16x3 product (chain) against fp64; the forward x3 kernels reach 4.4e-6
GAIN = 100                # x3 against the same product on bf16 operands


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def _randn(*shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _bf(t):
    return t.to(torch.bfloat16).double()


def _gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v / 2 ** 0.5))


def _dgelu(v):
    return 0.5 * (1.0 + torch.erf(v / 2 ** 0.5)) + v * torch.exp(-0.5 * v * v) / (2 * np.pi) ** 0.5


# ---- kernels ----------------------------------------------------------------------------------------------------------------------------
# token counts of the gradient rows: 16 images of 257 / 197 / 37 / 17 tokens, and a few images of each -- none a multiple of 32
TN_TOKENS = [16 * 257, 16 * 197, 16 * 37, 16 * 17, 3 * 257, 5 * 37, 17]


@pytest.mark.parametrize("K", TN_TOKENS)
def test_dw_db_grouped_against_fp64(K):
    """dW += dY^T X and db += colsum dY for the four block products of a ViT-S layer (+ a tiny one) in ONE launch, ragged token tails."""
    D = 384
    shapes = [(D, 4 * D), (4 * D, D), (D, D), (3 * D, D), (128, 512)]
    probs, refs = [], []
    for i, (M, N) in enumerate(shapes):
        dy, x = _randn(K, M, seed=10 * i + K, scale=0.1), _randn(K, N, seed=10 * i + 1 + K)
        c0, b0 = _randn(M, N, seed=10 * i + 2, scale=0.5), _randn(M, seed=10 * i + 3)
        c, b = c0.clone(), b0.clone()
        probs.append((dy, x, c, b, M, N, K))
        refs.append((c0.double() + dy.double().t() @ x.double(), b0.double() + dy.double().sum(0), _bf(dy).t() @ _bf(x) + c0.double()))
    desc, n, tiles, flops, nbytes = ops.make_group_tn_x3_desc(probs, DEV)
    ops.gemm_tn_x3_grouped(desc, n, tiles)
    for (dy, x, c, b, M, N, _), (rc, rb, rc_bf) in zip(probs, refs):
        e, eb = rel(c, rc), rel(rc_bf, rc)
        assert e < KERNEL_REL, (M, N, K, e)
        assert e * GAIN < eb, (M, N, K, e, eb)
        assert rel(b, rb) < 1e-6, (M, K, rel(b, rb))


@pytest.mark.parametrize("M,N,K", [(16 * 257, 1536, 384), (16 * 37, 3072, 768), (16 * 17, 512, 128), (5 * 197, 1536, 384)])
def test_dgelu_and_gelu_pre_epilogues(M, N, K):
    """fc1 of a saved forward (GELU + fp32 pre-activation, NT) and the input gradient through fc2 (acc * gelu'(pre), NN)."""
    A, W, bias = _randn(M, K, seed=1), _randn(N, K, seed=2, scale=K ** -0.5), _randn(N, seed=3, scale=0.1)
    h, pre = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
    ops.gemm_x3(ops.X3B_NT, ops.X3B_EPI_GELU_PRE, A, W, h, M, N, K, bias=bias, aux_out=pre, ldaux=N)
    rpre = A.double() @ W.double().t() + bias.double()
    assert rel(pre, rpre) < KERNEL_REL and rel(h, _gelu(rpre)) < KERNEL_REL
    # dpre = (g . W2) * gelu'(pre): W2 [K, N] read as stored ([out, in] of fc2 = [D, Hd])
    g, W2 = _randn(M, K, seed=4, scale=0.1), _randn(K, N, seed=5, scale=N ** -0.5)
    dpre = torch.empty(M, N, device=DEV)
    ops.gemm_x3(ops.X3B_NN, ops.X3B_EPI_DGELU, g, W2, dpre, M, N, K, aux=pre, ldaux=N)
    ref = (g.double() @ W2.double()) * _dgelu(pre.double())
    ref_bf = (_bf(g) @ _bf(W2)) * _dgelu(pre.double())
    e, eb = rel(dpre, ref), rel(ref_bf, ref)
    assert e < KERNEL_REL and e * GAIN < eb, (e, eb)


@pytest.mark.parametrize("M,N,K", [(16 * 257, 384, 1536), (16 * 197, 384, 1152), (16 * 37, 768, 768), (16 * 17, 128, 384), (37, 384, 384)])
def test_nn_input_gradient_against_fp64(M, N, K):
    """dX = dY . W with W [K, N] as the parameter block stores it (no transposed copy): plain and accumulating epilogues."""
    dy, W = _randn(M, K, seed=M, scale=0.1), _randn(K, N, seed=K, scale=K ** -0.5)
    ref = dy.double() @ W.double()
    C = torch.empty(M, N, device=DEV)
    ops.gemm_x3(ops.X3B_NN, ops.X3B_EPI_F32, dy, W, C, M, N, K)
    e, eb = rel(C, ref), rel(_bf(dy) @ _bf(W), ref)
    assert e < KERNEL_REL and e * GAIN < eb, (e, eb)
    C0 = _randn(M, N, seed=9)
    C2 = C0.clone()
    ops.gemm_x3(ops.X3B_NN, ops.X3B_EPI_ACC, dy, W, C2, M, N, K)
    assert rel(C2, C0.double() + ref) < KERNEL_REL


def _attn_ref(qkv, dout, B, N, H):
    D = H * 64
    q, k, v = qkv.double().view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4).unbind(0)
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o = torch.softmax((q @ k.transpose(-1, -2)) * 64 ** -0.5, -1) @ v
    o.backward(dout.double().view(B, N, H, 64).permute(0, 2, 1, 3))
    dq = torch.stack([t.grad.permute(0, 2, 1, 3).reshape(B * N, D) for t in (q, k, v)], 1).reshape(B * N, 3 * D)
    return o.detach().permute(0, 2, 1, 3).reshape(B * N, D), dq


@pytest.mark.parametrize("N", [17, 37, 197, 257])
@pytest.mark.parametrize("H", [2, 6, 12])
def test_attention_backward_against_fp64(N, H):
    B = 3
    D = H * 64
    qkv = _randn(B * N, 3 * D, seed=N * H, scale=1.5)
    dout = _randn(B * N, D, seed=N + H, scale=0.1)
    out, lse = torch.empty(B * N, D, device=DEV), torch.empty(B, H, N, device=DEV)
    ops.attn_fwd_x3_lse(qkv, out, lse, B, N, H, 64 ** -0.5)
    o_ref, d_ref = _attn_ref(qkv, dout, B, N, H)
    assert rel(out, o_ref) < KERNEL_REL
    s = (qkv.double().view(B, N, 3, H, 64)[:, :, 0].permute(0, 2, 1, 3) @ qkv.double().view(B, N, 3, H, 64)[:, :, 1].permute(0, 2, 3, 1)) * 64 ** -0.5
    assert rel(lse, torch.logsumexp(s, -1)) < 3e-6                  # (measured <= 1.5e-6: the x3 scores' own error)
    dqkv, delta = torch.full((B * N, 3 * D), float("nan"), device=DEV), torch.empty(B, H, N, device=DEV)
    ops.attn_bwd_x3(qkv, out, dout, lse, dqkv, delta, B, N, H, 64 ** -0.5)
    assert torch.isfinite(dqkv).all()                   # every element written
    for j, nm in enumerate(("dq", "dk", "dv")):
        e = rel(dqkv[:, j * D:(j + 1) * D], d_ref[:, j * D:(j + 1) * D])
        assert e < 5e-5, (nm, e)
    # the bf16 kernel on the same inputs
    qb, ob, dob = qkv.to(torch.bfloat16), torch.empty(B * N, D, dtype=torch.bfloat16, device=DEV), dout.to(torch.bfloat16)
    lb = torch.empty(B, H, N, device=DEV)
    ops.attn_fwd(qb, ob, lb, B, N, H, 64 ** -0.5)
    db = torch.empty(B * N, 3 * D, dtype=torch.bfloat16, device=DEV)
    ops.attn_bwd(qb, ob, dob, lb, db, torch.empty(B, H, N, device=DEV), B, N, H, 64 ** -0.5)
    assert rel(dqkv, d_ref) * GAIN < rel(db.float(), d_ref), (rel(dqkv, d_ref), rel(db.float(), d_ref))


@pytest.mark.parametrize("D", [128, 384, 768])
def test_layernorm_backward_fp32_dy(D):
    """fp32 dy, DropPath-scaled fp32 copy of the updated dx, LN_REP partial copies of dgamma / dbeta."""
    B, N = 5, 37
    M = B * N
    x, gamma, beta = _randn(M, D, seed=1), 1 + _randn(D, seed=2, scale=0.1), _randn(D, seed=3, scale=0.1)
    dy, dx0 = _randn(M, D, seed=4, scale=0.1), _randn(M, D, seed=5, scale=0.1)
    mean, rstd, y = torch.empty(M, device=DEV), torch.empty(M, device=DEV), torch.empty(M, D, device=DEV)
    ops.layernorm_fwd_f32(x, gamma, beta, 1e-6, y, mean, rstd, M, D)
    sc = torch.tensor([1.25, 0.0, 1.25, 1.25, 0.0], device=DEV)
    part = torch.zeros(16, 2, D, device=DEV)
    dx, out = dx0.clone(), torch.empty(M, D, device=DEV)
    ops.layernorm_bwd_part_f32(dy, x, mean, rstd, gamma, dx, part, 16, out, sc, N, M, D)
    xd, gd, bd = (t.double().clone().requires_grad_(True) for t in (x, gamma, beta))
    torch.nn.functional.layer_norm(xd, (D,), gd, bd, 1e-6).backward(dy.double())
    assert rel(dx, dx0.double() + xd.grad) < 1e-6
    assert rel(out, (dx0.double() + xd.grad) * sc.double().repeat_interleave(N)[:, None]) < 1e-6
    assert rel(part[:, 0].sum(0), gd.grad) < 1e-6 and rel(part[:, 1].sum(0), bd.grad) < 1e-6


# ---- backbone -----------------------------------------------------------------------------------------------------------------------------
CONFIGS = {"tiny": (vit.vit_tiny_test, V.VIT_TINY_TEST, 10, 8), "small_p2_32": (vit.vit_small_patch2_32, V.VIT_SMALL_P2_32, 100, 4),
           "small_p16_224": (vit.vit_small_patch16_224, V.VIT_SMALL_P16_224, 100, 2), "base_p16_96": (vit.vit_base_patch16_96, V.VIT_BASE_P16_96, 10, 4)}
# worst parameter tensor against fp32 autograd, measured on MI355X: 1.6e-5 (tiny), 2.2e-5 (ViT-S/2@32), 2.1e-5 (ViT-S/16@224),
# 1.8e-5 (ViT-B/16@96); bound = 1.5 x the worst.  The bf16 path on the same check: 2e-2 .. 4e-2 (test_vit_backward_matches_oracle_fp32_on_bf16_weights
# bounds it by 4e-2 on bf16-rounded weights)
BWD_REL = 3.3e-5
LOGIT_REL = 1e-4          # read_rows_precision's FWD_REL (measured 1.0e-5 .. 1.1e-5)


@pytest.mark.parametrize("tag", list(CONFIGS))
def test_vit_backward_x3_matches_fp32_autograd(tag):
    builder, cdict, C, B = CONFIGS[tag]
    model = builder(num_classes=C, device=DEV)
    with pytest.raises(AssertionError):                 # not opted in: no fp32 context is allocated behind the user's back
        model.forward_features(torch.zeros(1, 3, cdict["img_size"], cdict["img_size"], device=DEV), None, None, save=True, precision="bf16x3")
    model.grad_rows_precision = "bf16x3"
    cfg = V.VitCfg(num_classes=C, **cdict)
    P = {k: torch.from_numpy(v) for k, v in synth.synth_params(V.param_shapes(cfg), 5).items()}
    model.load_state_dict(P)
    rng = np.random.Generator(np.random.PCG64(6))
    x = torch.from_numpy(rng.standard_normal((B, 3, cfg.img_size, cfg.img_size)).astype(np.float32))
    y = torch.from_numpy(rng.integers(0, C, size=(B,), dtype=np.int64))
    dp = torch.from_numpy(synth.synth_droppath(7, V.drop_path_probs(cfg), B))
    assert (dp == 0).any() and (dp > 1).any()           # dropped and kept paths
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    o = V.vit_forward(Pg, x, cfg, dp)
    Hr.ce_loss_mean(o["logits"], y).backward()
    lg, ft, ctx = model.forward_features(x.to(DEV), None, dp.to(DEV), save=True, precision="bf16x3")
    assert ctx.precision == "bf16x3"
    el = rel(lg, o["logits"].detach())
    assert el < LOGIT_REL, el
    loss, dl = torch.empty(1, device=DEV), torch.empty(B, C, device=DEV)
    ops.masked_ce(lg, y.to(DEV), None, None, 1.0, loss, dl, B, C)
    model.zero_grad()
    model.backward(ctx, dl)
    g1 = model.grad.clone()
    worst = []
    D = cfg.embed_dim
    for n, gr in model.named_grads():
        ref = Pg[n].grad
        if n.endswith("attn.qkv.bias"):           # K-third is analytically zero (pure round-off in the reference)
            e = max(rel(gr[:D], ref[:D]), rel(gr[2 * D:], ref[2 * D:]))
        else:
            e = rel(gr, ref)
        worst.append((e, n))
    worst.sort(reverse=True)
    print("\n%s: logits %.2e, worst gradient tensors %s" % (tag, el, ["%s %.2e" % (n, e) for e, n in worst[:3]]))
    assert worst[0][0] < BWD_REL, worst[:5]
    # linear in dlogits: grads(2 dl) = 2 grads(dl)
    model.zero_grad()
    model.backward(ctx, 2 * dl)
    assert rel(model.grad, 2 * g1) < 1e-6
    # the bf16 context of the same model is untouched by the mode (and still is the default)
    _, _, c0 = model.forward_features(x.to(DEV), None, dp.to(DEV), save=True)
    assert c0.precision == "bf16" and c0 is not ctx
    model.zero_grad()
    model.backward(c0, dl)
    assert torch.isfinite(model.grad).all() and float(model.grad.abs().max()) > 0
    # ... and the bf16 forward and backward in between left the bf16x3 context and its backward plan as they were
    model.zero_grad()
    model.backward(ctx, dl)
    assert rel(model.grad, g1) < 1e-6


# ---- steps ---------------------------------------------------------------------------------------------------------------------------------
# per-iteration step-gradient rel-L2 against the reference's autograd: measured <= 1.66e-5 (srflexmatch_trace) / 2.12e-5 (c100); the bf16
# path's bound in test_sr_train_step_trace is 2.5e-2 (measured 0.005-0.010)
GRAD_STEP_REL = 3.2e-5
# sampled parameters after the engine's AdamW steps, every iteration against the reference's: measured <= 5.8e-6 / 6.0e-6 after 12 steps.
# One bound for all steps (the bf16 path widens its feature tolerance by 1.5e-2 per full-lr step taken)
PARAM_REL = 9e-6


@pytest.mark.parametrize("name,tr", [("srflexmatch_trace", TRACE), ("srflexmatch_c100_trace", TRACE_C100), ("srfixmatch_trace", TRACE_FIX),
                                     ("srfreematch_trace", TRACE_FREE), ("srsoftmatch_trace", TRACE_SOFT)])
def test_step_trace_with_both_options(golden, name, tr, monkeypatch):
    """The reference traces of test_sr_train_step_trace (12 iterations, the engine's own AdamW) with read_rows_precision and
    grad_rows_precision both bf16x3: every mask and pseudo label of every pass equals the reference's, the gradients follow its autograd,
    and the parameters stay within a bound that does not grow with the steps taken."""
    from oracle.gen_golden import trace_vit_params
    monkeypatch.setenv("SR_READ_ROWS_PRECISION", "bf16x3")
    monkeypatch.setenv("SR_GRAD_ROWS_PRECISION", "bf16x3")
    g = golden(name)
    flex = tr["algorithm"] == "srflexmatch"
    fix = tr["algorithm"] in ("srfixmatch", "srfreematch", "srsoftmatch")
    free, soft = tr["algorithm"] == "srfreematch", tr["algorithm"] == "srsoftmatch"
    C, Bl, Bu, seed = tr["C"], tr["Bl"], tr["Bu"], tr["seed"]
    cfg = V.VitCfg(num_classes=C, **V.VIT_TINY_TEST)
    extra = dict(ema_p=tr["ema_p"], use_quantile=tr["use_quantile"], clip_thresh=tr["clip_thresh"], ent_loss_ratio=tr["ent_loss_ratio"]) if free else {}
    if soft:
        extra = dict(ema_p=tr["ema_p"], n_sigma=tr["n_sigma"], dist_uniform=tr["dist_uniform"], dist_align=True, per_class=False)
    alg = get_algorithm(TS.make_args(algorithm=tr["algorithm"], p_cutoff=tr["p_cutoff"], num_classes=C, ulb_dest_len=tr["ulb_dest_len"],
                                     lr=tr.get("lr", 5e-4), **extra), vit.vit_tiny_test)
    assert alg.read_rows_precision == alg.grad_rows_precision == "bf16x3"
    T = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}   # noqa: E731
    alg.model.load_state_dict(T(trace_vit_params(cfg, seed, tr.get("head_gain", 1.0), tr.get("hot_classes", 0), tr.get("cold_scale", 0.25))))
    alg.rewarder.load_state_dict(T(synth.synth_params(S.rewarder_shapes(cfg.embed_dim, C), seed + 1)))
    alg.generator.load_state_dict(T(synth.synth_params(S.generator_shapes(cfg.embed_dim), seed + 2)))
    grad_rels, param_rels = [], []
    for n, it in enumerate(tr["its"]):
        p = f"it{it}"
        alg.it = it
        alg.optimizer.sched_step = it
        K = int(g[f"{p}/K"])
        b = synth.synth_batch(seed + 10 + n, Bl, Bu, cfg.img_size, C, tr["ulb_dest_len"])
        alg.inject_droppath = [torch.from_numpy(synth.synth_droppath(seed + 1000 * (n + 1) + k, V.drop_path_probs(cfg), Bl + 2 * Bu))
                               for k in range(K + 1)]
        alg.trace = {}
        out, log = alg.train_step(**alg.process_batch(**{k: torch.from_numpy(v) for k, v in b.items()}))
        alg.out_dict, alg.log_dict = out, log
        if flex:
            num = den = 0.0
            for nme, gv in alg.model.named_grads():
                gs = g.samp(f"{p}/grad/{nme}")
                a = TS.samp_of(gv.cpu().numpy(), gs).astype(np.float64)
                num += float(((a - gs["sample"]) ** 2).sum()); den += float((gs["sample"].astype(np.float64) ** 2).sum())
            grad_rels.append((num / max(den, 1e-30)) ** 0.5)
        alg.call_hook("after_train_step")
        masks = np.stack([m.cpu().numpy() for m in alg.trace["masks"]])
        want = g[f"{p}/masks"]
        if soft:
            np.testing.assert_allclose(masks, want, rtol=0.0, atol=1e-3)
        else:
            assert np.array_equal(masks, want), p
        if flex:
            assert np.array_equal(alg.trace["pseudo"].cpu().numpy().reshape(want.shape), g[f"{p}/pseudo_label"]), p
            num = den = 0.0
            for nme, v in alg.model.named_parameters():
                gs = g.samp(f"{p}/param/{nme}")
                a = TS.samp_of(v.detach().cpu().numpy(), gs).astype(np.float64)
                num += float(((a - gs["sample"]) ** 2).sum()); den += float((gs["sample"].astype(np.float64) ** 2).sum())
            param_rels.append((num / max(den, 1e-30)) ** 0.5)
        if not fix:
            sel = alg.hooks_dict["MaskingHook"].selected_label.cpu().numpy()
            nz = np.nonzero(sel != -1)[0]
            assert np.array_equal(nz, g[f"{p}/sel_idx"]) and np.array_equal(sel[nz], g[f"{p}/sel_val"]), p
            acc = alg.hooks_dict["MaskingHook"].classwise_acc.cpu().numpy()
            assert np.array_equal(acc.view(np.uint32), g[f"{p}/accs"][-1].view(np.uint32)), p
    if flex:
        print("\n%s: grad rel-L2 per iteration %s; parameter rel-L2 per iteration %s" % (
            name, ["%.2e" % r for r in grad_rels], ["%.2e" % r for r in param_rels]))
        assert max(grad_rels) < GRAD_STEP_REL, grad_rels
        assert max(param_rels) < PARAM_REL, param_rels


# worst step-gradient tensor at full size: measured 1.01e-4 (pos_embed, it = 1000) / 4.6e-5 (it = 30000); bf16 path: WORST_TENSOR_REL = 0.12,
# measured 0.062
FULL_WORST_TENSOR_REL = 1.5e-4


def test_full_size_trace_with_both_options(golden, monkeypatch):
    """srflexmatch_full_trace.npz (ViT-S/2, 100 classes, 8 / 8 / 8, two single steps from a mid-training state) with both options bf16x3:
    masks, pseudo labels and the FlexMatch table of the batch are the reference's, and every gradient tensor follows its autograd."""
    from oracle.gen_golden import FULL, full_hook_state, trace_vit_params
    monkeypatch.setenv("SR_READ_ROWS_PRECISION", "bf16x3")
    monkeypatch.setenv("SR_GRAD_ROWS_PRECISION", "bf16x3")
    g = golden("srflexmatch_full_trace")
    tr = FULL
    C, Bl, Bu = tr["C"], tr["Bl"], tr["Bu"]
    cfg = V.VitCfg(num_classes=C, **V.VIT_SMALL_P2_32)
    T_ = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}   # noqa: E731
    P0 = trace_vit_params(cfg, tr["seed"], tr["head_gain"])
    b = synth.synth_batch(int(g["meta/bseed"]), Bl, Bu, cfg.img_size, C, tr["ulb_dest_len"])
    sel0, acc0 = full_hook_state(b["idx_ulb"])
    for it in [int(i) for i in g["meta/its"]]:
        p = f"it{it}"
        K = int(g[f"{p}/K"])
        alg = get_algorithm(TS.make_args(algorithm="srflexmatch", num_classes=C, num_train_iter=tr["num_train_iter"], ulb_dest_len=tr["ulb_dest_len"],
                                         start_timing=tr["start_timing"], feature_dim=cfg.embed_dim, num_warmup_iter=tr["num_warmup_iter"],
                                         p_cutoff=tr["p_cutoff"], N_k=tr["N_k"], lr=tr["lr"]), vit.vit_small_patch2_32)
        assert alg.grad_rows_precision == "bf16x3"
        alg.model.load_state_dict(T_(P0))
        alg.rewarder.load_state_dict(T_(synth.synth_params(S.rewarder_shapes(cfg.embed_dim, C), tr["seed"] + 1)))
        alg.generator.load_state_dict(T_(synth.synth_params(S.generator_shapes(cfg.embed_dim), tr["seed"] + 2)))
        h = alg.hooks_dict["MaskingHook"]
        h.selected_label = torch.from_numpy(sel0.copy())
        h.classwise_acc = torch.from_numpy(acc0.copy()).to(DEV)
        alg.it = it
        alg.optimizer.sched_step = it
        alg.inject_droppath = [torch.from_numpy(synth.synth_droppath(int(g[f"{p}/dp_seed0"]) + k, V.drop_path_probs(cfg), Bl + 2 * Bu))
                               for k in range(K + 1)]
        alg.trace = {}
        out, log = alg.train_step(**alg.process_batch(**{k: torch.from_numpy(v) for k, v in b.items()}))
        torch.cuda.synchronize()
        want = g[f"{p}/masks"]
        masks = np.stack([m.cpu().numpy() for m in alg.trace["masks"]])
        assert np.array_equal(masks, want), p
        assert np.array_equal(alg.trace["pseudo"].cpu().numpy().reshape(want.shape), g[f"{p}/pseudo_label"]), p
        assert np.array_equal(h.selected_label.cpu().numpy()[b["idx_ulb"]], g[f"{p}/sel_after_batch"])
        assert np.array_equal(h.classwise_acc.cpu().numpy().view(np.uint32), g[f"{p}/accs"][-1].view(np.uint32))
        worst = (0.0, None)
        for nme, gv in alg.model.named_grads():
            gs = g.samp(f"{p}/grad/{nme}")
            a = TS.samp_of(gv.cpu().numpy(), gs).astype(np.float64)
            e2, n2 = float(((a - gs["sample"]) ** 2).sum()), float((gs["sample"].astype(np.float64) ** 2).sum())
            if n2 > 0 and not nme.endswith("attn.qkv.bias") and nme != "cls_token":
                worst = max(worst, ((e2 / n2) ** 0.5, nme))
        print("\nfull trace %s with both options: worst gradient tensor %.2e (%s)" % (p, worst[0], worst[1]))
        assert worst[0] < FULL_WORST_TENSOR_REL, (p, worst)


# ---- graph ---------------------------------------------------------------------------------------------------------------------------------
def test_captured_step_replays_the_eager_step_with_both_options(monkeypatch):
    """core/stepgraph.py with both options on: the replayed step's features, masks and FlexMatch table are the eager step's bit for bit."""
    monkeypatch.setenv("SR_READ_ROWS_PRECISION", "bf16x3")
    monkeypatch.setenv("SR_GRAD_ROWS_PRECISION", "bf16x3")
    it0, n = 30008, 8
    a0, _ = TG._make(False, it0, monkeypatch)
    a1, sg = TG._make(True, it0, monkeypatch)
    assert a0.grad_rows_precision == a1.grad_rows_precision == "bf16x3"
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
