"""``device_eval: True`` and ``run_hooks: True`` on the GPU: SRFlexMatch with ViT-S/2 fed by the device loaders (10 classes, 12 labelled,
40 unlabelled, 10 evaluation images, batch 4, uratio 2).  (a) evaluate() on the device accumulators against today's path on the same
weights; (b) a 6-step run with the reference's evaluation / checkpoint / logging hooks; (c) a run resumed from the file CheckpointHook
wrote against the run that never stopped; (d) without the keys train() writes and prints nothing."""
import argparse
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import synth_image                              # noqa: E402
from semireward_amd.algorithms import get_algorithm                    # noqa: E402
from semireward_amd.nets import vit                                    # noqa: E402

F64_BOUND = 2e-6          # fp32 against float64, relative (tests/test_gpu_criterions.py)


def _flex_args(dd, **kw):
    d = dict(algorithm="srflexmatch", num_classes=10, num_train_iter=6, epoch=2, ema_m=0.0, ulb_loss_ratio=1.0, use_cat=True, amp=False, lr=5e-4,
             weight_decay=5e-4, layer_decay=0.5, num_warmup_iter=0, optim="AdamW", T=0.5, p_cutoff=0.95, hard_label=True, thresh_warmup=True, N_k=2,
             start_timing=2, feature_dim=384, sr_lr=5e-4, sr_ema=False, sr_ema_m=0.99, num_eval_iter=0, num_log_iter=3, gpu=0, rank=0, world_size=1,
             distributed=False, dataset="cifar100", img_size=32, crop_ratio=0.875, batch_size=4, uratio=2, eval_batch_size=4,
             train_sampler="RandomSampler", seed=5, device_data=True, dataset_dict=dd)
    d.update(kw)
    return argparse.Namespace(**d)


def _dict_datasets(H0, n_lb=12, n_ulb=40, n_ev=10, C=10):
    rng = np.random.Generator(np.random.PCG64(H0))
    mk = lambda n, s: np.stack([synth_image(s + t, H0, H0, t % 3) for t in range(n)])      # noqa: E731
    return {"train_lb": {"data": mk(n_lb, 1000), "targets": rng.integers(0, C, size=n_lb)}, "train_ulb": {"data": mk(n_ulb, 2000), "targets": None},
            "eval": {"data": mk(n_ev, 3000), "targets": rng.integers(0, C, size=n_ev)}}


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, s):
        self.lines.append(s)


def _build(log=None, **kw):
    return get_algorithm(_flex_args(_dict_datasets(64), **kw), vit.vit_small_patch2_32, None, log)


METRICS = ("top-1-acc", "balanced_acc", "precision", "recall", "F1")


def test_device_eval_equals_todays_evaluate_on_the_same_weights():
    base, log = _build(), _Log()
    dev = _build(log, device_eval=True)
    dev.model.load_state_dict(base.model.state_dict())
    dev.model.refresh_operands()
    assert list(dev.hooks_dict) == list(base.hooks_dict)                     # the key alone registers no hook
    log.lines.clear()
    a, b = base.evaluate("eval", return_logits=True), dev.evaluate("eval", return_logits=True)
    assert set(a) == set(b) == {"eval/loss", "eval/logits"} | {"eval/" + k for k in METRICS}
    for k in METRICS:
        assert a["eval/" + k] == b["eval/" + k], k
    assert np.array_equal(a["eval/logits"], b["eval/logits"]) and b["eval/logits"].shape == (10, 10)
    # both losses are fp32 row arithmetic, each within F64_BOUND of the float64 value (today's path also adds the batches in fp32)
    print("eval/loss: today's %.9g, device_eval %.9g" % (a["eval/loss"], b["eval/loss"]))
    assert abs(a["eval/loss"] - b["eval/loss"]) <= 2 * F64_BOUND * abs(a["eval/loss"])
    z = a["eval/logits"].astype(np.float64)
    y = np.asarray(dev.args.dataset_dict["eval"]["targets"])
    want = float((np.log(np.exp(z - z.max(1, keepdims=True)).sum(1)) + z.max(1) - z[np.arange(10), y]).reshape(-1).sum())
    assert abs(b["eval/loss"] * 10 - want) <= F64_BOUND * abs(want)           # (no -1 labels: mean per batch times its rows == the plain sum)
    # the confusion matrix goes through print_fn as the reference's does (algorithmbase.py:426-427)
    assert len(log.lines) == 1 and log.lines[0].startswith("confusion matrix:\n[[")
    assert dev.model.training == base.model.training
    # evaluation over host tensors and an explicit loader: the same result
    host = [{k: v.cpu() for k, v in bt.items()} for bt in dev.loader_dict["eval"]]
    assert dev.evaluate("eval", loader=host) == {k: v for k, v in b.items() if k != "eval/logits"}


NUM = r"(-?\d+\.\d{4}|-?inf|nan)"                                           # "{:.4f}"
LOG_LINE = r"%d iteration USE_EMA: False, (\S+: " + NUM + r", )*\S+: " + NUM + r" $"
EVAL_LINE = r"%d iteration, USE_EMA: False, (\S+: " + NUM + r", )*\S+: " + NUM + r" BEST_EVAL_ACC: (?P<acc>\d\.\d{4}), at (?P<it>\d+) iters$"


def test_run_hooks_evaluate_checkpoint_and_log_a_six_step_run(tmp_path):
    log = _Log()
    alg = _build(log, run_hooks=True, device_eval=True, num_eval_iter=3, num_log_iter=2, save_dir=str(tmp_path), save_name="r")
    assert list(alg.hooks_dict)[:4] == ["ParamUpdateHook", "EMAHook", "EvaluationHook", "CheckpointHook"] and list(alg.hooks_dict)[-1] == "LoggingHook"
    evals, real = [], alg.evaluate
    alg.evaluate = lambda *a, **k: (evals.append(alg.it), real(*a, **k))[1]
    log.lines.clear()
    alg.train()
    torch.cuda.synchronize()
    assert alg.it == 6 and evals == [2, 5]                                                   # exactly two evaluations
    d = tmp_path / "r"
    assert (d / "latest_model.pth").exists()
    assert (d / "model_best.pth").exists() == (alg.best_eval_metric > 0)
    assert set(alg.results_dict) == {"eval/best_acc", "eval/best_it"}
    assert alg.results_dict == {"eval/best_acc": alg.best_eval_metric, "eval/best_it": alg.best_it} and alg.best_it in (0, 2, 5)
    ck = torch.load(str(d / "latest_model.pth"), map_location="cpu")
    assert ck["it"] == 6 + 1 and ck["best_eval_acc"] == alg.best_eval_metric                # after_run's save: ``it`` has advanced past the last step
    its = [l for l in log.lines if re.match(r"\d+ iteration", l)]
    assert [int(l.split()[0]) for l in its] == [2, 3, 4, 6], its
    assert re.match(LOG_LINE % 2, its[0]) and re.match(LOG_LINE % 4, its[2]), its
    for n, l in ((3, its[1]), (6, its[3])):
        m = re.match(EVAL_LINE % n, l)
        assert m, l
        if n == 3:                                                                           # the first evaluation is the best so far, unless it scored 0
            assert int(m.group("it")) == (3 if float(m.group("acc")) > 0 else 1), l
        else:
            assert int(m.group("it")) == alg.best_it + 1 and m.group("acc") == "%.4f" % alg.best_eval_metric, l
        assert "eval/top-1-acc: " in l and "eval/loss: " in l and "lr: " in l and "train/run_time: " in l
    assert "eval/top-1-acc" not in its[0] and "lr: " in its[0] and "train/total_loss: " in its[0]
    assert log.lines.count("validating...") == 2 and sum(l.startswith("confusion matrix:\n") for l in log.lines) == 2
    assert alg.model.training is True


def _params(alg):
    return alg.model.flat.detach().double().cpu()


def test_resume_through_the_checkpoint_hooks_file(tmp_path):
    """Run B is a 6-step run stopped after 3 steps: built like run A (same schedule, same loaders) with ``num_train_iter`` then lowered to 3,
    so that step 3 is the last iteration and CheckpointHook writes there.  A fresh instance C loads that file and runs to 6.
      * after ``load_model`` every piece of state of C equals B's bit for bit (``state_of`` of tests/test_gpu_resume.py);
      * C against B simply continuing in place to 6 (the run that never stopped, from the same state): parameters within the 1e-6 relative L2
        of tests/test_gpu_resume.py (the backward's fp32 atomics);
      * C against run A, an independent 6-step run, is printed and not asserted: two independent runs of this engine are not bit-equal, and
        their distance was seen to exceed the bound without a checkpoint being involved (profiles/run_to_run_distance.txt).
    The file is the one the hook writes inside the loop: ``after_run`` then overwrites latest_model.pth with ``it`` advanced by one, as the
    reference does (configs/README.md)."""
    from test_gpu_resume import state_of
    kw = dict(run_hooks=True, num_log_iter=0, num_eval_iter=3)               # every run evaluates after steps 3 and 6, as the others do
    a = _build(_Log(), save_dir=str(tmp_path / "a"), **kw)
    a.train()
    b = _build(_Log(), save_dir=str(tmp_path / "b"), **kw)
    b.num_train_iter = 3
    f = tmp_path / "hook_latest.pth"
    real = b.save_model

    def saving(name, path):
        real(name, path)
        if name == "latest_model.pth" and b.it == 2:
            shutil.copy(os.path.join(path, name), str(f))
    b.save_model = saving
    b.train()
    assert b.it == 3 and (tmp_path / "b" / "run" / "latest_model.pth").exists()
    assert torch.load(str(f), map_location="cpu")["it"] == 3
    c = _build(_Log(), save_dir=str(tmp_path / "c"), **kw)
    c.load_model(str(f))
    assert c.it == 3 and c.start_epoch == 1 and (c.best_eval_metric, c.best_it) == (b.best_eval_metric, b.best_it)
    sb, sc = state_of(b), state_of(c)
    assert set(sb) == set(sc)
    for k in sb:
        assert torch.equal(sb[k], sc[k]), k
    start = _params(b)
    c.train()
    b.num_train_iter, b.start_epoch = 6, 1                                   # B keeps going: the second epoch, steps 4 .. 6
    b.train()
    torch.cuda.synchronize()
    assert c.it == b.it == a.it == 6
    pa, pb, pc = _params(a), _params(b), _params(c)
    err = float((pb - pc).norm() / pb.norm())
    print("resume through CheckpointHook: resumed vs continued in place %.3e, resumed vs an independent run %.3e, steps 4 .. 6 moved %.3e" % (
        err, float((pa - pc).norm() / pa.norm()), float((pb - start).norm() / pb.norm())))
    assert err <= 1e-6, err
    assert float((pb - start).norm()) > 0                                    # and steps 4 .. 6 did move the parameters


def test_without_the_keys_train_writes_and_prints_nothing(tmp_path):
    log = _Log()
    alg = _build(log, save_dir=str(tmp_path), num_eval_iter=3, num_log_iter=2)
    assert not {"EvaluationHook", "CheckpointHook", "LoggingHook"} & set(alg.hooks_dict)
    log.lines.clear()
    alg.train()
    torch.cuda.synchronize()
    assert alg.it == 6 and log.lines == [] and list(tmp_path.iterdir()) == [] and not hasattr(alg, "results_dict")
