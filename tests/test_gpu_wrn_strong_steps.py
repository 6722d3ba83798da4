"""SRFixMatch / SRFlexMatch / SRFreeMatch / SRSoftMatch on the WideResNet (classic_cv) against traces of the reference's own train_step
(tests/golden/sr{fix,flex,free,soft}match_wrn_trace.npz, tools/gen_wrn_strong_traces.py): every one of the K + 1 model() calls of a step
forwards cat(x_lb, x_ulb_w, x_ulb_s) in training mode -- one BatchNorm statistics group each, each moving the running statistics.
Modelled on tests/test_gpu_wrn.py::test_srpseudolabel_wrn_trace, with its bounds."""
import argparse
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import semireward_ref as S        # noqa: E402
from oracle import wrn_ref as W               # noqa: E402
from oracle.gen_golden import synth_wrn_params   # noqa: E402
from semireward_amd.algorithms import get_algorithm   # noqa: E402
from semireward_amd.nets import wrn           # noqa: E402
from semireward_amd.utils import synth        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _traces():
    spec = importlib.util.spec_from_file_location("gen_wrn_strong_traces", os.path.join(ROOT, "tools", "gen_wrn_strong_traces.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def make_args(tr, Fd, **kw):
    d = dict(algorithm=tr["algorithm"], num_classes=tr["C"], num_train_iter=tr["num_train_iter"], epoch=1, ema_m=tr["ema_m"], ulb_loss_ratio=1.0,
             use_cat=True, amp=False, optim="SGD", lr=tr["lr"], momentum=tr["momentum"], weight_decay=tr["weight_decay"], layer_decay=1.0,
             num_warmup_iter=tr["num_warmup_iter"], p_cutoff=tr["p_cutoff"], N_k=tr["N_k"], start_timing=tr["start_timing"], feature_dim=Fd,
             sr_lr=5e-4, sr_ema=False, sr_ema_m=0.99, gpu=0, rank=0, world_size=1, distributed=False, T=0.5, hard_label=True,
             thresh_warmup=True, ulb_dest_len=tr["ulb_dest_len"])
    if tr["algorithm"] == "srfreematch":
        d.update(ema_p=tr["ema_p"], use_quantile=tr["use_quantile"], clip_thresh=tr["clip_thresh"], ent_loss_ratio=tr["ent_loss_ratio"])
    if tr["algorithm"] == "srsoftmatch":
        d.update(ema_p=tr["ema_p"], n_sigma=tr["n_sigma"], dist_uniform=tr["dist_uniform"], dist_align=True, per_class=False)
    d.update(kw)
    return argparse.Namespace(**d)


@pytest.mark.parametrize("algo", ["srfixmatch", "srflexmatch", "srfreematch", "srsoftmatch"])
def test_strong_view_wrn_trace(golden, algo):
    """Bounds of test_srpseudolabel_wrn_trace: zero mask flips (the fixture keeps every thresholded max-prob > 1e-2 from its threshold),
    running_var 1e-3, running_mean 5e-2 + 3e-2 n, losses 6e-2, final parameters 3e-2, the EMA as there; num_batches_tracked advances by K + 1
    per step.  SoftMatch's masks are continuous weights: the tolerance of test_sr_train_step_trace[srsoftmatch_trace] (6e-2 absolute,
    util_ratio 4e-2).

    No bound is wider than that.  The trace has the three iterations that cover the regimes of a step (it0: K = 0; it1: K = 0 and the stage-1
    rewarder update; it110: K = 19 and the N_k update): every SGD step at lr 0.03 moves a trajectory with bf16 convolution operands further
    from the fp32 one (gradients go through LeakyReLU kinks), and a fixture is kept only if the REFERENCE's own run with bf16-rounded
    convolution operands on the CPU stays inside these bounds and flips no mask (tools/gen_wrn_strong_traces.py: bf16_inside_bounds;
    tests/test_cpu_wrn_strong_steps.py asserts it on the fixture)."""
    mod = _traces()
    tr = mod.TRACES[algo]
    g = golden(algo + "_wrn_trace")
    flex, free, soft = algo == "srflexmatch", algo == "srfreematch", algo == "srsoftmatch"
    C, Bl, Bu, seed = tr["C"], tr["Bl"], tr["Bu"], tr["seed"]
    assert (int(g["meta/seed"]), float(g["meta/p_cutoff"]), float(g["meta/head_gain"])) == (seed, tr["p_cutoff"], tr["head_gain"])
    wcfg = W.WrnCfg(num_classes=C, **W.WRN_TINY_TEST)
    Fd = W.channels(wcfg)[3]
    alg = get_algorithm(make_args(tr, Fd), wrn.wrn_tiny_test)
    Tn = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}   # noqa: E731
    P0 = mod.wrn_params(wcfg, tr)
    alg.model.load_state_dict(Tn(P0))
    assert alg.ema_m == 0.999 and alg.ema_model is not alg.model
    alg.ema_model.load_state_dict(Tn(P0))
    alg.rewarder.load_state_dict(Tn(synth.synth_params(S.rewarder_shapes(Fd, C), seed + 1)))
    alg.generator.load_state_dict(Tn(synth.synth_params(S.generator_shapes(Fd), seed + 2)))
    flips = total = nbt = 0
    for n, it in enumerate(tr["its"]):
        p = f"it{it}"
        alg.it = it
        alg.optimizer.sched_step = it
        K = int(g[f"{p}/K"])
        b = synth.synth_batch(seed + 10 + n, Bl, Bu, tr["img"], C, tr["ulb_dest_len"])
        alg.trace = {}
        before = alg.rewarder.flat.clone()
        out, log = alg.train_step(**alg.process_batch(**{k: torch.from_numpy(v) for k, v in b.items()}))
        alg.out_dict, alg.log_dict = out, log
        assert alg.optimizer.lr_factor() == pytest.approx(float(g[f"{p}/lr_factor"]), rel=1e-9, abs=1e-12)
        alg.call_hook("after_train_step")
        assert alg.trace["K"] == K
        masks = np.stack([m.cpu().numpy() for m in alg.trace["masks"]])
        want = g[f"{p}/masks"]
        assert masks.shape == want.shape == (K + 1, Bu)
        mpv = alg.trace["max_probs"].cpu().numpy().reshape(masks.shape)
        print(p, "K", K, "max |max-prob - reference|", float(np.abs(mpv - g[f"{p}/mask_probs"]).max()),
              "losses", [float(log["train/" + k_]) for k_ in ("sup_loss", "unsup_loss", "total_loss")],
              [float(g[f"{p}/log/{k_}"]) for k_ in ("sup_loss", "unsup_loss", "total_loss")])
        if soft:
            np.testing.assert_allclose(masks, want, rtol=0.0, atol=6e-2)
            assert float(log["train/util_ratio"]) == pytest.approx(float(g[f"{p}/log/util_ratio"]), abs=4e-2)
            bad = np.zeros(masks.shape, bool)
        else:
            assert float(np.abs(g[f"{p}/mask_probs"] - g[f"{p}/mask_thr"]).min()) > 1e-2
            if flex:
                assert float(np.abs(g[f"{p}/mask_probs"] - tr["p_cutoff"]).min()) > 1e-2
            bad = masks != want
            flips += int(bad.sum()); total += bad.size
            assert not bad.any(), (p, mpv[bad], g[f"{p}/mask_probs"][bad], g[f"{p}/mask_thr"][bad])
            # (pseudo labels where they count and where the reference's own runner-up class is further than the margin: elsewhere a near tie)
            sel = (want > 0) & (g[f"{p}/label_gap"] > 1e-2)
            assert np.array_equal(alg.trace["pseudo"].cpu().numpy().reshape(want.shape)[sel], g[f"{p}/pseudo_label"][sel]), p
        for k_, v in alg.model.buffers.items():                      # every one of the K + 1 calls moves them, momentum 0.001
            if not k_.endswith("num_batches_tracked"):
                d = rel(v.cpu(), g[f"{p}/buf/{k_}"])
                assert d < (5e-2 + 3e-2 * n if k_.endswith("running_mean") else 1e-3), (p, k_, d)
        nbt += K + 1
        assert int(g[f"{p}/num_batches_tracked"]) == nbt
        assert all(int(v) == nbt for k_, v in alg.model.buffers.items() if k_.endswith("num_batches_tracked")), p
        assert int(not torch.equal(before, alg.rewarder.flat)) == int(g[f"{p}/rewarder_updated"]), p
        for k_ in ("sup_loss", "unsup_loss", "total_loss"):
            assert float(log["train/" + k_]) == pytest.approx(float(g[f"{p}/log/{k_}"]), rel=6e-2, abs=5e-3), (p, k_)
        for k_ in ("x_lb", "x_ulb_w", "x_ulb_s"):
            assert rel(out["feat"][k_].cpu(), g[f"{p}/feat/{k_}"]) < 5e-2 + 3e-2 * n, (p, k_)
        mr = float(g[f"{p}/max_reward"])
        assert (np.isinf(mr) and np.isinf(float(alg.max_reward))) or float(alg.max_reward) == pytest.approx(mr, rel=1e-2), p
        h = alg.hooks_dict["MaskingHook"]
        if flex:
            sel = h.selected_label.cpu().numpy()
            nz = np.nonzero(sel != -1)[0]
            assert np.array_equal(nz, g[f"{p}/sel_idx"]) and np.array_equal(sel[nz], g[f"{p}/sel_val"]), p
            assert np.array_equal(h.classwise_acc.cpu().numpy().view(np.uint32), g[f"{p}/classwise_acc"].view(np.uint32)), p
        if free:
            assert float(h.time_p) == pytest.approx(float(g[f"{p}/time_p"]), rel=2e-2)
            assert rel(h.p_model.cpu(), g[f"{p}/p_model"]) < 2e-2
            assert rel(h.label_hist.cpu(), g[f"{p}/label_hist"]) < 2e-2
        if soft:
            da = alg.hooks_dict["DistAlignHook"]
            assert float(h.prob_max_mu_t) == pytest.approx(float(g[f"{p}/mu"]), rel=2e-2)
            assert float(h.prob_max_var_t) == pytest.approx(float(g[f"{p}/var"]), rel=5e-2)
            assert rel(da.p_model.cpu(), g[f"{p}/p_model"]) < 2e-2
            assert rel(da.p_target.cpu(), g[f"{p}/p_target"]) < 2e-2
    assert flips == 0 and (soft or total > 0), (flips, total)
    worst = 0.0
    last = f"it{tr['its'][-1]}"
    for nme, v in alg.model.named_parameters():
        gs = g.samp(f"{last}/param/{nme}")
        a = v.reshape(-1).cpu().numpy()[::gs["stride"]]
        worst = max(worst, float(np.abs(a - gs["sample"]).max()))
    print("worst parameter deviation", worst)
    assert worst < 3e-2, worst
    for nme, v in alg.ema_model.named_parameters():
        gs = g.samp(f"{last}/ema/{nme}")
        a = v.reshape(-1).cpu().numpy()[::gs["stride"]]
        assert float(np.abs(a - gs["sample"]).max()) < 1e-5 + 6e-3 * worst, nme
        m_ = alg.model.view(nme).reshape(-1).cpu().numpy()[::gs["stride"]]
        assert float(np.abs(a - m_).max()) > 0.0 or float(np.abs(m_).max()) == 0.0, nme
    for k_, v in alg.model.buffers.items():
        if not k_.endswith("num_batches_tracked"):
            assert torch.equal(alg.ema_model.buffers[k_], v), k_


def test_full_width_step_properties_wrn_28_2():
    """SRFlexMatch on wrn_28_2, 100 classes, 8 labelled + 16 + 16 unlabelled 32 x 32 images, K = sr_decay() = 8: finite losses,
    num_batches_tracked += 9, and every pass's logits bit-equal to pass 0's -- the network has no stochastic layer and the batch statistics do
    not read the running ones, so a difference would mean the statistics groups of the shared launches are not independent."""
    C, Bl, Bu = 100, 8, 16
    wcfg = W.WrnCfg(num_classes=C, **W.WRN_28_2)
    Fd = W.channels(wcfg)[3]
    tr = dict(algorithm="srflexmatch", C=C, num_train_iter=2000, ema_m=0.999, lr=0.03, momentum=0.9, weight_decay=1e-3, num_warmup_iter=0,
              p_cutoff=0.05, N_k=10, start_timing=100, ulb_dest_len=256)
    alg = get_algorithm(make_args(tr, Fd), wrn.wrn_28_2)
    sd = {k: torch.from_numpy(v) for k, v in synth_wrn_params(wcfg, 5).items()}
    alg.model.load_state_dict(sd)
    alg.ema_model.load_state_dict(sd)
    alg.it = 1001                                   # sr_decay() = max(8, 1 + 2000 / 1001) = 8; not a rewarder-update step
    alg.optimizer.sched_step = alg.it
    b = synth.synth_batch(300, Bl, Bu, 32, C, 256)
    alg.trace = {}
    nbt0 = int(alg.model.buffers["bn1.num_batches_tracked"])
    run0 = alg.model.buffers["bn1.running_mean"].clone()
    out, log = alg.train_step(**alg.process_batch(**{k: torch.from_numpy(v) for k, v in b.items()}))
    torch.cuda.synchronize()
    assert alg.trace["K"] == 8
    for k_ in ("sup_loss", "unsup_loss", "total_loss"):
        assert np.isfinite(float(log["train/" + k_])), k_
    assert all(int(v) == nbt0 + 9 for k_, v in alg.model.buffers.items() if k_.endswith("num_batches_tracked"))
    assert not torch.equal(run0, alg.model.buffers["bn1.running_mean"])
    L = alg.trace["logits"]
    assert L.shape == (9, Bl + 2 * Bu, C)
    for p_ in range(1, 9):
        assert torch.equal(L[p_], L[0]), p_
    assert torch.isfinite(alg.model.grad).all() and float(alg.model.grad.abs().max()) > 0
