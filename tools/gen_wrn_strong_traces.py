"""tests/golden/sr{fix,flex,free,soft}match_wrn_trace.npz: the reference's four strong-view SemiReward train_steps on the WideResNet.

TEST INFRASTRUCTURE (build container only: it RUNS THE REFERENCE through oracle/_ref_import.py, like oracle/gen_golden.py whose helpers it
calls).  classic_cv flavour, in the style of TRACE_PL_WRN: WRN_TINY_TEST (depth 10) on 8 x 8 images, SGD + Nesterov 0.03 / 0.9 / 1e-3, no
warm-up, ema_m 0.999, use_cat True -- every one of the K + 1 model() calls of a step forwards cat(x_lb, x_ulb_w, x_ulb_s) in training mode, so
every call is one BatchNorm statistics group over Bl + 2 Bu images and moves the running statistics and num_batches_tracked (no Bn_Controller
here: srfixmatch/fixmatch.py:62-146).  Iterations 0 (K = 0), 1 (K = 0, stage-1 rewarder update), 110 (K = 19, N_k update): the regimes of a
step and nothing more -- every further SGD step at lr 0.03 only adds trajectory drift between fp32 and bf16-operand arithmetic (the gradients
go through LeakyReLU kinks), which is not what the trace pins.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_wrn_strong_traces.py            # writes the four fixtures from TRACES below
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_wrn_strong_traces.py --search   # screens seed / p_cutoff / head gain ON THE REFERENCE ALONE

Screening (search(), on the reference alone): a candidate is acceptable when no hard decision of any pass of any iteration sits within
MIN_MARGIN of its threshold and the masks are mixed.  The hard decisions: the max-prob against the fixed cut-off, against FlexMatch's
class-wise threshold and cut-off, against FreeMatch's time_p * p_model / max p_model; and the pseudo label (an argmax) of every row that
reaches the loss against its runner-up class (`label_gap`, recorded per row) -- a near tie there hands the strong row another target.
SoftMatch's weights are continuous and positive: no threshold, and the label gap of EVERY row is its screened quantity.  TRACES holds, per
algorithm, the acceptable candidate with the widest smallest margin at the LOWEST head gain of GAINS that has one among SEEDS x CUTS (the
gradients of a step grow with the gain, and with them the drift), provided the CPU model below stays inside the GPU test's bounds on it.

CPU model: the same reference run with only its convolutions taking bf16-rounded operands (bf16_conv_model), the number formats of an engine
with bf16 matrix units.  Its deviation from the fixture is stored under bf16dev/; a fixture is written only if that model stays inside the
bounds the GPU test sets and flips no mask (bf16_inside_bounds).  The fixtures hold arrays only.
"""
import argparse
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as G  # noqa: E402

MIN_MARGIN = 1.02e-2       # (the tests assert > 1e-2 on the fixture)
_WRN = dict(backbone="wrn", lr=0.03, momentum=0.9, weight_decay=1e-3, img=8, num_warmup_iter=0, ema_m=0.999, its=[0, 1, 110])
TRACES = {
    "srfixmatch": dict(G._TRACE_BASE, **_WRN, algorithm="srfixmatch", seed=300, p_cutoff=0.25, head_gain=1.0),
    "srflexmatch": dict(G._TRACE_BASE, **_WRN, algorithm="srflexmatch", Bu=8, ulb_dest_len=16, seed=249, p_cutoff=0.4, head_gain=2.0),
    "srfreematch": dict(G._TRACE_BASE, **_WRN, algorithm="srfreematch", seed=298, head_gain=1.0, ema_p=0.9, use_quantile=True, clip_thresh=False,
                        ent_loss_ratio=0.05, p_cutoff=0.0),
    "srsoftmatch": dict(G._TRACE_BASE, **_WRN, algorithm="srsoftmatch", seed=257, head_gain=1.5, ema_p=0.9, n_sigma=2, dist_uniform=False,
                        p_cutoff=0.0),
}
META = ("seed", "p_cutoff", "head_gain", "Bl", "Bu", "C", "ulb_dest_len", "img", "lr", "momentum", "weight_decay", "ema_m", "num_train_iter",
        "start_timing", "N_k", "num_warmup_iter")


def wrn_params(wcfg, tr):
    p = G.synth_wrn_params(wcfg, tr["seed"])
    p["classifier.weight"] = (p["classifier.weight"] * np.float32(tr["head_gain"])).astype(np.float32)      # spreads the max-probs
    return p


class _Bf16Conv(torch.autograd.Function):
    """A convolution with bf16-ROUNDED OPERANDS and fp32 accumulation, forward and backward: activation, filter and the upstream gradient are
    rounded to bf16 before every product -- the number formats of an engine that runs its convolutions on bf16 matrix units.  Everything else
    (BatchNorm, LeakyReLU, pooling, classifier, losses, SGD) stays the reference's fp32."""

    @staticmethod
    def forward(ctx, x, w, b, stride, padding):
        xr, wr = x.bfloat16().float(), w.bfloat16().float()
        ctx.save_for_backward(xr, wr)
        ctx.cfg = (stride, padding, b is not None)
        return torch.nn.functional.conv2d(xr, wr, b, stride, padding)

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        stride, padding, has_b = ctx.cfg
        dyr = dy.bfloat16().float()
        dx = torch.nn.grad.conv2d_input(xr.shape, wr, dyr, stride, padding)
        dw = torch.nn.grad.conv2d_weight(xr, wr.shape, dyr, stride, padding)
        return dx, dw, (dy.sum((0, 2, 3)) if has_b else None), None, None


def bf16_conv_model(model):
    """The reference model with every Conv2d computing through _Bf16Conv (a CPU model of bf16 convolution operands)."""
    for m_ in model.modules():
        if isinstance(m_, torch.nn.Conv2d):
            m_.forward = (lambda x, _m=m_: _Bf16Conv.apply(x, _m.weight, _m.bias, _m.stride, _m.padding))
    return model


def run(tr, bf16_convs=False):
    """The reference's train_step (+ backward, SGD, scheduler, EMA) over tr['its'] -> (fixture dict, stats).  ``bf16_convs``: the same run with
    the convolutions of the reference model computing on bf16-rounded operands (bf16_conv_model)."""
    R, W, S, synth, T = G.R, G.W, G.S, G.synth, G.T
    algo = tr["algorithm"]
    flex, free, soft = algo == "srflexmatch", algo == "srfreematch", algo == "srsoftmatch"
    C, Bl, Bu, seed = tr["C"], tr["Bl"], tr["Bu"], tr["seed"]
    wcfg = W.WrnCfg(num_classes=C, **W.WRN_TINY_TEST)
    Fd = W.channels(wcfg)[3]
    bu = R.mod("semilearn.core.utils.build")
    misc = R.mod("semilearn.core.utils.misc")
    model = G.build_ref_wrn(wcfg, wrn_params(wcfg, tr))
    if bf16_convs:
        bf16_conv_model(model)
    model.train()
    alg = G.build_headless_srflexmatch(model, C, Fd, tr)
    G.load_module_params(alg.rewarder, synth.synth_params(S.rewarder_shapes(Fd, C), seed + 1))
    G.load_module_params(alg.generator, synth.synth_params(S.generator_shapes(Fd), seed + 2))
    # the reference's classic_cv optimizer in place of the headless object's AdamW
    alg.optimizer = bu.get_optimizer(model, "SGD", tr["lr"], tr["momentum"], tr["weight_decay"], 1.0)
    alg.scheduler = bu.get_cosine_schedule_with_warmup(alg.optimizer, tr["num_train_iter"], num_warmup_steps=tr["num_warmup_iter"])
    ema = misc.EMA(model, tr["ema_m"])
    ema.register()
    ema_model = copy.deepcopy(model)
    bns = [(nme, dict(model.named_modules())[nme]) for nme, _, _ in W.bn_names(wcfg)]
    out, prev_it, margin, gap = {}, -1, 1.0, 1.0
    for n, it in enumerate(tr["its"]):
        for _ in range(it - prev_it - 1):
            alg.scheduler.step()
        prev_it = it
        alg.it = it
        K = 0 if it <= tr["start_timing"] else int(max(8, 1 + tr["num_train_iter"] / it))
        b = synth.synth_batch(seed + 10 + n, Bl, Bu, tr["img"], C, tr["ulb_dest_len"])
        alg.model = G._CountingModel(model)
        rec = dict(mask=[], probs=[], thr=[], pl=[], gap=[])
        mh = alg.hooks_dict["MaskingHook"]
        orig = mh.masking

        def wrapped(algorithm, *a, _orig=orig, _rec=rec, **k):
            lg = k["logits_x_ulb"].detach()
            probs = torch.softmax(lg, dim=-1) if k.get("softmax_x_ulb", True) else lg
            mp, mi = probs.max(dim=-1)
            top2 = probs.topk(2, dim=-1)[0]
            _rec["gap"].append((top2[:, 0] - top2[:, 1]).numpy().copy())       # the argmax is a hard decision too: how far the runner-up is
            thr = None
            if flex:          # utils.py:47-53: the class-wise threshold from the state BEFORE the call
                acc = mh.classwise_acc[mi]
                thr = (algorithm.p_cutoff * (acc / (2.0 - acc))).numpy().copy()
            m = _orig(algorithm, *a, **k)
            if free:          # freematch/utils.py:60-62: time_p * p_model / max p_model, the state the call itself just moved
                thr = (mh.time_p * (mh.p_model / mh.p_model.max())[mi]).numpy().copy()
            if thr is None:
                thr = np.full(mp.shape, tr["p_cutoff"], np.float32)
            _rec["mask"].append(m.numpy().copy()); _rec["probs"].append(mp.numpy().copy()); _rec["pl"].append(mi.numpy().copy())
            _rec["thr"].append(thr.astype(np.float32))
            return m
        mh.masking = wrapped
        nbt0 = int(bns[0][1].num_batches_tracked)
        rbefore = {k_: v.detach().clone() for k_, v in alg.rewarder.named_parameters()}
        if flex:
            o, log = alg.train_step(T(b["x_lb"]), T(b["y_lb"]), T(b["idx_ulb"]), T(b["x_ulb_w"]), T(b["x_ulb_s"]))
        else:
            o, log = alg.train_step(T(b["x_lb"]), T(b["y_lb"]), T(b["x_ulb_w"]), T(b["x_ulb_s"]))
        mh.masking = orig
        assert alg.model.calls == K + 1, (alg.model.calls, K)
        assert all(int(m_.num_batches_tracked) == nbt0 + K + 1 for _, m_ in bns)
        o["loss"].backward()
        p = f"it{it}"
        for nme, prm in model.named_parameters():
            G.flat(f"{p}/grad/{nme}", G.samp(prm.grad.numpy() if prm.grad is not None else np.zeros(tuple(prm.shape), np.float32), 64), out)
        out[f"{p}/lr_factor"] = np.float64(alg.scheduler.get_last_lr()[-1] / tr["lr"])
        alg.optimizer.step(); alg.scheduler.step(); model.zero_grad()
        ema.update()
        ema_model.load_state_dict(model.state_dict())
        ema_model.load_state_dict(ema.shadow, strict=False)
        for nme, prm in ema_model.named_parameters():
            G.flat(f"{p}/ema/{nme}", G.samp(prm.detach().numpy(), 64), out)
        for k_, v in log.items():
            out[f"{p}/log/{k_.split('/')[-1]}"] = np.float64(v)
        out[f"{p}/K"], out[f"{p}/calls"] = np.int64(K), np.int64(alg.model.calls)
        out[f"{p}/masks"], out[f"{p}/mask_probs"] = np.stack(rec["mask"]), np.stack(rec["probs"])
        out[f"{p}/mask_thr"], out[f"{p}/pseudo_label"] = np.stack(rec["thr"]), np.stack(rec["pl"])
        out[f"{p}/label_gap"] = np.stack(rec["gap"])
        used = out[f"{p}/masks"] > 0            # rows whose pseudo label reaches the loss (SoftMatch: every row, its weights are positive)
        if used.any():
            gap = min(gap, float(out[f"{p}/label_gap"][used].min()))
        if not soft:
            margin = min(margin, float(np.abs(out[f"{p}/mask_probs"] - out[f"{p}/mask_thr"]).min()))
        if flex:
            margin = min(margin, float(np.abs(out[f"{p}/mask_probs"] - tr["p_cutoff"]).min()))
        for k_ in ("x_lb", "x_ulb_w", "x_ulb_s"):
            out[f"{p}/feat/{k_}"] = o["feat"][k_].detach().numpy()
        out[f"{p}/rewarder_updated"] = np.int64(any(not torch.equal(rbefore[k_], v.detach()) for k_, v in alg.rewarder.named_parameters()))
        for k_, v in alg.rewarder.named_parameters():
            G.flat(f"{p}/rewarder/{k_}", G.samp(v.detach().numpy(), 64), out)
        for nme, prm in model.named_parameters():
            G.flat(f"{p}/param/{nme}", G.samp(prm.detach().numpy(), 64), out)
        out[f"{p}/max_reward"] = np.float64(float(alg.max_reward))
        for nme, m_ in bns:
            out[f"{p}/buf/{nme}.running_mean"], out[f"{p}/buf/{nme}.running_var"] = m_.running_mean.numpy().copy(), m_.running_var.numpy().copy()
        out[f"{p}/num_batches_tracked"] = np.int64(int(bns[0][1].num_batches_tracked))
        if flex:
            sel = mh.selected_label.numpy(); nz = np.nonzero(sel != -1)[0]
            out[f"{p}/sel_idx"], out[f"{p}/sel_val"] = nz.astype(np.int64), sel[nz]
            out[f"{p}/classwise_acc"] = mh.classwise_acc.numpy().copy()
        if free:
            out[f"{p}/time_p"], out[f"{p}/p_model"] = np.float32(mh.time_p), mh.p_model.numpy().copy()
            out[f"{p}/label_hist"] = mh.label_hist.numpy().copy()
        if soft:
            dh = alg.hooks_dict["DistAlignHook"]
            out[f"{p}/mu"], out[f"{p}/var"] = np.float32(mh.prob_max_mu_t), np.float32(mh.prob_max_var_t)
            out[f"{p}/p_model"], out[f"{p}/p_target"] = dh.p_model.numpy().copy(), dh.p_target.numpy().copy()
    out["meta/its"] = np.array(tr["its"], dtype=np.int64)
    for k_ in META:
        out[f"meta/{k_}"] = np.float64(tr[k_])
    allm = np.concatenate([out[f"it{it}/masks"].ravel() for it in tr["its"]])
    return out, dict(mask_mean=float(allm.mean()), margin=margin, label_gap=gap)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def bf16_deviation(tr, out):
    """How far the SAME reference run moves when only its convolutions take bf16-rounded operands: per iteration, the deviation of every
    quantity the GPU test bounds, from the fp32 fixture ``out``.  A step's gradients go through LeakyReLU kinks, so rounding the operands does
    not perturb the trajectory smoothly: it is the size of these deviations, measured here on the CPU and on the reference alone, that says
    what an engine with bf16 convolution operands can be held to on this trace.  Stored in the fixture under bf16dev/."""
    o2, _ = run(tr, bf16_convs=True)
    dev = {}
    for it in tr["its"]:
        p = f"it{it}"
        for k_ in ("sup_loss", "unsup_loss", "total_loss", "util_ratio"):
            dev[f"bf16dev/{p}/log/{k_}"] = np.float64(abs(float(o2[f"{p}/log/{k_}"]) - float(out[f"{p}/log/{k_}"])))
        for k_ in ("x_lb", "x_ulb_w", "x_ulb_s"):
            dev[f"bf16dev/{p}/feat/{k_}"] = np.float64(rel(o2[f"{p}/feat/{k_}"], out[f"{p}/feat/{k_}"]))
        bm = [rel(o2[k_], out[k_]) for k_ in out if k_.startswith(f"{p}/buf/") and k_.endswith("running_mean")]
        bv = [rel(o2[k_], out[k_]) for k_ in out if k_.startswith(f"{p}/buf/") and k_.endswith("running_var")]
        dev[f"bf16dev/{p}/running_mean"], dev[f"bf16dev/{p}/running_var"] = np.float64(max(bm)), np.float64(max(bv))
        dev[f"bf16dev/{p}/masks"] = np.float64(np.abs(o2[f"{p}/masks"] - out[f"{p}/masks"]).max())
        dev[f"bf16dev/{p}/mask_probs"] = np.float64(np.abs(o2[f"{p}/mask_probs"] - out[f"{p}/mask_probs"]).max())
        for k_ in ("time_p", "mu", "var"):
            if f"{p}/{k_}" in out:
                dev[f"bf16dev/{p}/{k_}"] = np.float64(abs(float(o2[f"{p}/{k_}"]) - float(out[f"{p}/{k_}"])) / abs(float(out[f"{p}/{k_}"])))
        for k_ in ("p_model", "p_target", "label_hist"):
            if f"{p}/{k_}" in out:
                dev[f"bf16dev/{p}/{k_}"] = np.float64(rel(o2[f"{p}/{k_}"], out[f"{p}/{k_}"]))
        mr, mr2 = float(out[f"{p}/max_reward"]), float(o2[f"{p}/max_reward"])
        dev[f"bf16dev/{p}/max_reward"] = np.float64(0.0 if np.isinf(mr) else abs(mr2 - mr) / abs(mr))
    last = f"it{tr['its'][-1]}"
    dev["bf16dev/param"] = np.float64(max(float(np.abs(o2[k_] - out[k_]).max()) for k_ in out if k_.startswith(f"{last}/param/") and k_.endswith("/sample")))
    return dev


def bf16_inside_bounds(tr, out, dev):
    """Does the CPU model with bf16 convolution operands stay inside the bounds the GPU test sets (those of test_srpseudolabel_wrn_trace and,
    for SoftMatch's weights, of the srsoftmatch_trace test)?  A trace on which that model itself leaves them -- or flips a mask -- measures
    the drift of an SGD trajectory, not an engine: such a candidate is not kept.  Returns the list of what is outside."""
    soft, bad = tr["algorithm"] == "srsoftmatch", []
    for n, it in enumerate(tr["its"]):
        p, d = f"it{it}", (lambda k_: float(dev[f"bf16dev/it{it}/{k_}"]))
        if d("masks") > (6e-2 if soft else 0.0):
            bad.append((p, "masks", d("masks")))
        if soft and d("log/util_ratio") > 4e-2:
            bad.append((p, "util_ratio", d("log/util_ratio")))
        for k_ in ("sup_loss", "unsup_loss", "total_loss"):
            if d("log/" + k_) > max(5e-3, 6e-2 * abs(float(out[f"{p}/log/{k_}"]))):
                bad.append((p, k_, d("log/" + k_)))
        for k_ in ("feat/x_lb", "feat/x_ulb_w", "feat/x_ulb_s", "running_mean"):
            if d(k_) >= 5e-2 + 3e-2 * n:
                bad.append((p, k_, d(k_)))
        if d("running_var") >= 1e-3:
            bad.append((p, "running_var", d("running_var")))
        for k_, b_ in (("time_p", 2e-2), ("p_model", 2e-2), ("label_hist", 2e-2), ("mu", 2e-2), ("var", 5e-2), ("p_target", 2e-2), ("max_reward", 1e-2)):
            if f"bf16dev/{p}/{k_}" in dev and d(k_) >= b_:
                bad.append((p, k_, d(k_)))
    if float(dev["bf16dev/param"]) >= 3e-2:
        bad.append(("final", "param", float(dev["bf16dev/param"])))
    return bad


def acceptable(tr, st):
    if tr["algorithm"] == "srsoftmatch":      # (no threshold: the pseudo labels are its hard decisions)
        return st["label_gap"] >= MIN_MARGIN
    return min(st["margin"], st["label_gap"]) >= MIN_MARGIN and 0.15 < st["mask_mean"] < 0.95


GAINS = (1.0, 1.5, 2.0)      # lowest first: the gradients of a step, and with them the drift of a bf16-operand trajectory, grow with the gain
SEEDS = range(201, 321)
CUTS = {"srfixmatch": [0.14, 0.16, 0.18, 0.2, 0.22, 0.25, 0.3], "srflexmatch": [0.12, 0.14, 0.16, 0.18, 0.2, 0.25, 0.3, 0.4]}


def _screen_one(tr):
    torch.set_num_threads(1)
    _, st = run(tr)
    return tr, st


def search(algo, workers=8):
    """The rule TRACES follows: at the LOWEST head gain of GAINS that has an acceptable candidate among SEEDS x CUTS, the candidate whose
    smallest margin (thresholds and label gaps) is widest and on which the CPU model with bf16 convolution operands stays inside the GPU
    test's bounds.  Everything here runs the reference alone."""
    import multiprocessing
    base = TRACES[algo]
    for gain in GAINS:
        cand = [dict(base, seed=seed, head_gain=gain, p_cutoff=pc) for seed in SEEDS for pc in CUTS.get(algo, [0.0])]
        with multiprocessing.get_context("fork").Pool(workers) as pool:
            res = [(min(st["margin"], st["label_gap"]), tr, st) for tr, st in pool.imap(_screen_one, cand, chunksize=4) if acceptable(tr, st)]
        res.sort(key=lambda r: -r[0])
        print(algo, "head_gain", gain, ":", len(res), "of", len(cand), "candidates acceptable", flush=True)
        for q, tr, st in res:
            out, _ = run(tr)
            bad = bf16_inside_bounds(tr, out, bf16_deviation(tr, out))
            print(algo, "seed", tr["seed"], "head_gain", gain, "p_cutoff", tr["p_cutoff"], st, "bf16 CPU model outside:", bad, flush=True)
            if not bad:
                return tr
    print(algo, "no candidate")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--search", action="store_true")
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    for algo, tr in TRACES.items():
        if a.only and a.only != algo:
            continue
        if a.search:
            search(algo)
            continue
        out, st = run(tr)
        print(algo, st)
        assert acceptable(tr, st), (algo, st)
        dev = bf16_deviation(tr, out)
        for it in tr["its"]:
            print("  bf16-operand CPU model, it%d:" % it, {k_.split("/", 2)[2]: float("%.3g" % v) for k_, v in dev.items() if k_.startswith("bf16dev/it%d/" % it)})
        print("  bf16-operand CPU model, final parameters:", float(dev["bf16dev/param"]))
        bad = bf16_inside_bounds(tr, out, dev)
        assert not bad, (algo, bad)
        out.update(dev)
        np.savez_compressed(os.path.join(G.OUT, "%s_wrn_trace.npz" % algo), **out)
