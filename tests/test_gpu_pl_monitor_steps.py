"""``monitor_pseudo_labels: True`` through the algorithms: four steps across start_timing (K = 0 and K > 0) on every algorithm and backbone
family.  The monitor's window equals the restatement of tests/_pl_monitor_cases.py applied to each step's trace, summed; from equal
states a step computes what it computes with the key off (everything deterministic bit for bit, the parameters to the engine's own run-to-run
round-off; see the test's docstring); the log line gains exactly the eight keys; with the key off nothing is launched."""
import argparse
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _pl_monitor_cases as PC                                  # noqa: E402
from semireward_amd import ops                                 # noqa: E402
from semireward_amd.algorithms import get_algorithm            # noqa: E402
from semireward_amd.algorithms import srflexmatch as SF        # noqa: E402
from semireward_amd.core.pl_monitor import LOG_KEYS, PlMonitor  # noqa: E402
from semireward_amd.nets import bert, vit, wrn                 # noqa: E402
from semireward_amd.utils import synth                         # noqa: E402

C, BL, BU, N_ULB, IMG = 10, 4, 6, 64, 8
ITS = (1, 2, 3, 4)                     # start_timing 2: K = 0, 0, then sr_decay() = 9 and 8 data_generator passes (num_train_iter 24)
OLD_KEYS = ["train/sup_loss", "train/unsup_loss", "train/total_loss", "train/util_ratio"]
SUM_BOUND = 2.0 ** -39                 # tests/test_gpu_pl_monitor.py: the kernel's fp64 sums against the restatement's


def _targets():
    rng = np.random.Generator(np.random.PCG64(77))
    t = rng.integers(0, C, size=N_ULB).astype(np.int64)
    t[rng.random(N_ULB) < 0.2] = -1
    return t


def _args(algorithm, backbone, **kw):
    d = dict(algorithm=algorithm, num_classes=C, num_train_iter=24, epoch=1, ema_m=0.0, ulb_loss_ratio=1.0, use_cat=backbone != "bert", amp=False,
             lr=5e-4, weight_decay=5e-4, layer_decay=0.5, num_warmup_iter=0, optim="AdamW", T=0.5, p_cutoff=0.12, hard_label=True,
             thresh_warmup=True, ulb_dest_len=N_ULB, N_k=10, start_timing=2, feature_dim=128, sr_lr=5e-4, sr_ema=False, sr_ema_m=0.99, gpu=0,
             rank=0, world_size=1, distributed=False, unsup_warm_up=0.4, ema_p=0.5, use_quantile=False, clip_thresh=False, ent_loss_ratio=0.01,
             n_sigma=2, dist_uniform=True, dist_align=True, per_class=False)
    if backbone == "wrn":
        d.update(optim="SGD", lr=0.03, momentum=0.9, weight_decay=1e-3, layer_decay=1.0)
    d.update(kw)
    return argparse.Namespace(**d)


BUILDERS = {"vit": vit.vit_tiny_test, "bert": bert.bert_tiny_test, "wrn": wrn.wrn_tiny_test}
CONFIGS = [("srflexmatch", "vit"), ("srfixmatch", "vit"), ("srfreematch", "vit"), ("srsoftmatch", "vit"), ("srpseudolabel", "vit"),
           ("srsoftmatch", "bert"), ("srpseudolabel", "wrn")]


def _batch(backbone, n):
    """Step n's batch as a loader hands it over (CPU tensors, idx_ulb included whatever the algorithm's train_step takes)."""
    b = {k: torch.from_numpy(v) for k, v in synth.synth_batch(900 + n, BL, BU, IMG, C, N_ULB).items()}
    if backbone == "bert":
        g = torch.Generator().manual_seed(400 + n)

        def tokens(rows, L):
            ids = torch.randint(1, 120, (rows, L), generator=g)
            am = torch.ones(rows, L, dtype=torch.int64)
            am[0, L - 3:] = 0                                   # a padded row
            return {"input_ids": ids * am, "attention_mask": am}
        b.update(x_lb=tokens(BL, 12 + n), x_ulb_w=tokens(BU, 15), x_ulb_s=tokens(BU, 10 + 2 * n))
    return b


def _copy_state(dst, src):
    """Everything a step reads, through the project's checkpoint (resume is exact, tests/test_gpu_resume.py): parameters, BatchNorm buffers,
    optimizer moments, rewarder / generator and their optimizer, the thresholding hooks' state, the counter-based RNG position."""
    buf = io.BytesIO()
    torch.save(src.get_save_dict(), buf)
    buf.seek(0)
    dst.load_model(buf)
    assert torch.equal(dst.model.flat, src.model.flat) and torch.equal(dst.rewarder.flat, src.rewarder.flat)


def _step(alg, backbone, n, it, trace):
    """Step n at iteration ``it``: (log_dict, trace or None, idx_ulb)."""
    alg.model.train()
    alg.it = it
    alg.optimizer.sched_step = it
    b = _batch(backbone, n)
    alg.trace = {} if trace else None
    alg.out_dict, alg.log_dict = alg.train_step(**alg.process_batch(**b))
    alg.call_hook("after_train_step")
    return alg.log_dict, alg.trace, b["idx_ulb"].numpy()


def _run(alg, backbone, trace):
    out = [_step(alg, backbone, n, it, trace) for n, it in enumerate(ITS)]
    torch.cuda.synchronize()
    ops.check_label_errors()
    return out


def _case_of(trace, idx, targets):
    K = int(trace["K"])
    nu = idx.shape[0]
    h = lambda t: None if t is None else t.detach().cpu().numpy().reshape(-1)       # noqa: E731
    return dict(P=K + 1, nu=nu, C=C, n_ulb=targets.shape[0], pseudo=h(trace["pseudo"]), masks=[h(m) for m in trace["masks"]],
                mask2=h(trace["mask2"]), reward=h(trace["reward"]), idx_ulb=idx, targets=targets)


def _same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a):
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
    return a == b


@pytest.mark.parametrize("algorithm,backbone", CONFIGS, ids=["%s+%s" % c for c in CONFIGS])
def test_window_equals_the_restated_traces_and_the_step_is_unchanged(algorithm, backbone, monkeypatch):
    """Two algorithm objects, the key on and off.  The monitored run is free-running; before every step the other one takes over its whole
    state (a checkpoint round trip), so that each of its steps is THE SAME step without the monitor.

    Why from equal states per step and not two free runs: the engine's backward adds weight gradients with fp32 atomics (see
    profiles/run_to_run_distance.txt and tests/test_gpu_stepgraph.py), so two free runs with the key OFF already end apart in their
    parameters after these four steps -- measured on one MI355X, max |difference|: 1.2e-10 .. 2.3e-10 on the tiny ViT (all five
    algorithms), 5.9e-04 on the tiny BERT, 0 on the tiny WideResNet -- and a free-running on / off pair measures the same noise: 5.96e-08
    (srflexmatch), 1.46e-10 (srfixmatch), 1.56e-06 (srfreematch), 1.75e-10 (srsoftmatch), 1.16e-10 (srpseudolabel) on the tiny ViT,
    1.30e-04 on the tiny BERT, 0 on the tiny WideResNet: a bit-for-bit comparison of two free runs fails with the key off on both sides.
    From equal states
    everything the engine computes deterministically must agree bit for bit -- every traced quantity of every pass (logits, features, max
    probabilities, pseudo labels, masks, rewards, mask2), the returned features, the four log values; on the WideResNet (no atomics on this
    path) the parameters too -- and the parameters behind an atomics-summed gradient agree to the round-off of one optimizer step, the
    rewarder (its embedding gradient is an atomic scatter) to 1e-5: the bounds tests/test_gpu_stepgraph.py puts on its eager / replayed
    pair.  Those two bounds are loose against a monitor that wrote into the parameters; what pins that down is that every forward quantity
    of the NEXT step still agrees bit for bit (the monitored object free-runs) and the sentinel words of tests/test_gpu_pl_monitor.py."""
    monkeypatch.setattr(SF, "_DEFER_AUTOTUNE", False)
    targets = _targets()
    on = get_algorithm(_args(algorithm, backbone, monitor_pseudo_labels=True, ulb_targets=targets), BUILDERS[backbone])
    off = get_algorithm(_args(algorithm, backbone), BUILDERS[backbone])
    assert isinstance(on.pl_monitor, PlMonitor) and not hasattr(off, "pl_monitor")
    want = PC.empty_state(C)
    Ks, logs_on = [], []
    for n, it in enumerate(ITS):
        _copy_state(off, on)
        before = on.model.flat.clone()
        log_on, tr_on, idx = _step(on, backbone, n, it, trace=True)
        log_off, tr_off, _ = _step(off, backbone, n, it, trace=True)
        torch.cuda.synchronize()
        logs_on.append(log_on)
        Ks.append(int(tr_on["K"]))
        want = PC.add_states(want, PC.restate(_case_of(tr_on, idx, targets)))
        # ---- the log line: the four old keys in their order and with the values of the step without the monitor, then exactly the eight new ones
        assert list(log_off) == OLD_KEYS and list(log_on) == OLD_KEYS + ["train/" + k for k in LOG_KEYS]
        old = [(float(log_on[k]), float(log_off[k])) for k in OLD_KEYS]
        assert all(a == b for a, b in old), (it, old)
        # ---- the step computes what it computes with the key off
        assert sorted(tr_on) == sorted(tr_off)
        for k in tr_on:
            a, b = tr_on[k], tr_off[k]
            if k in ("logits", "feats") and not on.use_cat and a.shape[0] > 1:
                # use_cat False: the labelled rows of the passes 1 .. K are never computed (srflexmatch._Plan.cat_passes): unwritten memory
                assert _same_bits(a[0], b[0]), (it, k)
                a, b = a[1:, BL:], b[1:, BL:]
            assert _same_bits(a, b), (it, k)
        for k, v in on.out_dict["feat"].items():
            assert _same_bits(v, off.out_dict["feat"][k]), (it, k)
        upd = float((on.model.flat - before).abs().max())
        d = (on.model.flat - off.model.flat).abs()
        dr = float((on.rewarder.flat - off.rewarder.flat).abs().max())
        print("%s+%s it %d (K = %d): parameters on vs off max |diff| %.3e mean %.3e (largest update %.3e), rewarder %.3e" % (
            algorithm, backbone, it, Ks[-1], float(d.max()), float(d.mean()), upd, dr))
        assert upd > 0.0
        if backbone == "wrn":
            assert torch.equal(on.model.flat, off.model.flat), it
        else:
            assert float(d.max()) <= 2.1 * upd and float(d.mean()) <= 1e-2 * upd, (it, float(d.max()), float(d.mean()), upd)
        assert dr <= 1e-5, (it, dr)
    ops.check_label_errors()
    assert Ks[0] == Ks[1] == 0 and Ks[2] > 0 and Ks[3] > 0, Ks
    # ---- the window: every step's trace through the restatement, summed
    got = on.pl_monitor.read(reset=False)
    diff = PC.state_equal_ints(got, want)
    assert not diff, {k: (got[k], want[k]) for k in diff}
    assert got["steps"] == 4 and got["rows"] + got["rows_unknown"] == 4 * BU and got["gen_rows"] > 0 and got["hist"].sum() == got["gen_rows"]
    for name, g, w in (("sum_w", got["sum_w"], want["sum_w"]), ("sum_w_correct", got["sum_w_correct"], want["sum_w_correct"]),
                       ("sum_r[0]", got["sum_r"][0], want["sum_r"][0]), ("sum_r[1]", got["sum_r"][1], want["sum_r"][1])):
        print("%s+%s %s: %.17g (restatement %.17g)" % (algorithm, backbone, name, g, w))
        assert abs(g - w) <= SUM_BOUND * abs(w), (name, g, w)
    assert not want["flag"] and got["rows"] > 0 and got["reward_bad"] == 0
    # ---- the last step's log values describe the whole window (nobody read before), from ONE copy that starts the next window
    m = PlMonitor.metrics_from_state(want)
    for k in LOG_KEYS:
        v = float(logs_on[-1]["train/" + k])
        assert (np.isnan(v) and np.isnan(m[k])) or v == pytest.approx(m[k], rel=1e-9), (k, v, m[k])
    assert not on.pl_monitor.block.any()
    # an older line read after a newer one reads nan and leaves the running window alone
    on.pl_monitor.accumulate(0, [torch.ones(BU, device=on.device)], torch.zeros(BU, dtype=torch.int64, device=on.device), None, None,
                             torch.arange(BU, device=on.device))
    assert np.isnan(float(logs_on[0]["train/pl_acc"])) and on.pl_monitor.read(reset=False)["steps"] == 1


def test_key_off_launches_nothing(monkeypatch):
    """ops.pl_monitor raises: a run with the key off never reaches it, a run with the key on does."""
    monkeypatch.setattr(SF, "_DEFER_AUTOTUNE", False)

    def boom(*a, **k):
        raise AssertionError("ops.pl_monitor was called")
    monkeypatch.setattr(ops, "pl_monitor", boom)
    off = get_algorithm(_args("srfixmatch", "vit"), BUILDERS["vit"])
    steps = _run(off, "vit", trace=False)
    assert all(list(log) == OLD_KEYS and np.isfinite(float(log["train/total_loss"])) for log, _, _ in steps)
    on = get_algorithm(_args("srfixmatch", "vit", monitor_pseudo_labels=True, ulb_targets=_targets()), BUILDERS["vit"])
    with pytest.raises(AssertionError, match="ops.pl_monitor was called"):
        _run(on, "vit", trace=False)
    torch.cuda.synchronize()


def test_unread_log_values_copy_nothing_and_a_batch_without_idx_ulb_is_refused(monkeypatch):
    monkeypatch.setattr(SF, "_DEFER_AUTOTUNE", False)
    on = get_algorithm(_args("srfixmatch", "vit", monitor_pseudo_labels=True, ulb_targets=_targets()), BUILDERS["vit"])
    reads = []
    real = on.pl_monitor.read
    monkeypatch.setattr(on.pl_monitor, "read", lambda reset=True: (reads.append(reset), real(reset))[1])
    steps = _run(on, "vit", trace=False)
    assert reads == []                                           # four steps, nobody read a monitor value: no copy
    assert float(steps[1][0]["train/select_ratio"]) >= 0.0 and reads == [True]
    float(steps[1][0]["train/pl_acc"])
    assert reads == [True]                                       # the same line: the same copy
    assert on.pl_monitor.read(reset=False)["steps"] == 0
    b = _batch("vit", 0)
    del b["idx_ulb"]
    on.it = 1
    with pytest.raises(ValueError, match="idx_ulb"):
        on.train_step(**on.process_batch(**b))
    torch.cuda.synchronize()


def test_example_prints_the_monitor_keys(monkeypatch, capsys):
    """examples/train_synthetic_cifar.py --monitor-pseudo-labels: the synthetic set's labels go in, every log line shows the eight keys."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic_cifar as ex
    monkeypatch.setattr(sys, "argv", ["train_synthetic_cifar.py", "--steps", "31", "--monitor-pseudo-labels"])
    ex.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("it ")]
    assert len(lines) == 4
    for ln in lines:
        f = ln.split()
        assert all(k in f for k in LOG_KEYS), ln
    last = dict(zip(lines[-1].split()[2::2], lines[-1].split()[3::2]))
    assert 0.0 <= float(last["pl_acc"]) <= 1.0 and 0.0 <= float(last["reward_auc"]) <= 1.0       # it 30 > start_timing 20: rewards were scored
    first = dict(zip(lines[0].split()[2::2], lines[0].split()[3::2]))
    assert first["reward_auc"] == "nan" and first["select_ratio"] == "1.000"                      # K = 0, thresh_warmup: every row kept
