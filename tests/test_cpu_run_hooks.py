"""``run_hooks: True`` and ``device_eval: True``, host side (no GPU): the metrics computed from the confusion counts alone against sklearn
and against ``classification_metrics``; EvaluationHook / CheckpointHook / LoggingHook (semilearn/core/hooks/evaluation.py, checkpoint.py,
logging.py) on a stub algorithm -- cadence, strict best-model tracking, save order, rank gating, after_run, the exact log lines; and the
registration order on the base class (algorithmbase.py:270-276), which without the key stays today's list."""
import argparse
import os

import numpy as np
import pytest

from semireward_amd.core.algorithmbase import AlgorithmBase
from semireward_amd.core.hooks import (CheckpointHook, DistSamplerSeedHook, EMAHook, EvaluationHook, Hook, LoggingHook, ParamUpdateHook,
                                       TimerHook)
from semireward_amd.nets import vit


# ---- 1. metrics_from_confusion ----------------------------------------------------------------------------------------------------------
def _confusion(yt, yp, C):
    cm = np.zeros((C + 1, C), dtype=np.int32)
    np.add.at(cm, (np.where(yt < 0, C, yt), yp), 1)
    return cm


def _cases():
    rng = np.random.Generator(np.random.PCG64(5))
    out = []
    for C, n in [(10, 200), (100, 300), (3, 7), (2, 50)]:
        yt, yp = rng.integers(0, C, n), rng.integers(0, C, n)
        yp[: n // 3] = yt[: n // 3]
        out.append(("plain", C, yt, yp))
    yt, yp = rng.integers(0, 10, 200), rng.integers(0, 10, 200)
    yt[yt == 4] = 5                                      # class 4 absent from y_true, present in y_pred
    yt[yt == 7], yp[yp == 7] = 6, 6                      # class 7 absent from both
    out.append(("absent", 10, yt, yp))
    out.append(("absent_100", 100, rng.integers(0, 30, 300), rng.integers(20, 60, 300)))
    yt, yp = rng.integers(0, 10, 200), rng.integers(0, 10, 200)
    yp[:70] = yt[:70]
    yt[::9] = -1                                         # ignore_index rows: one more class of y_true, never predicted
    out.append(("ignored", 10, yt, yp))
    out.append(("all_ignored_but_one", 3, np.array([-1, -1, 2, -1]), np.array([0, 2, 2, 1])))
    return out


@pytest.mark.parametrize("name,C,yt,yp", _cases(), ids=lambda v: v if isinstance(v, str) else None)
def test_metrics_from_confusion_match_sklearn_and_classification_metrics(name, C, yt, yp):
    from sklearn.metrics import accuracy_score, balanced_accuracy_score, f1_score, precision_score, recall_score
    import warnings
    m = AlgorithmBase.metrics_from_confusion(_confusion(yt, yp, C))
    assert m == AlgorithmBase.classification_metrics(yt, yp)                 # exactly: same label set, same order of the sums
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                      # (y_pred contains classes not in y_true)
        assert m["top-1-acc"] == pytest.approx(accuracy_score(yt, yp))
        assert m["balanced_acc"] == pytest.approx(balanced_accuracy_score(yt, yp))
        assert m["precision"] == pytest.approx(precision_score(yt, yp, average="macro", zero_division=0))
        assert m["recall"] == pytest.approx(recall_score(yt, yp, average="macro", zero_division=0))
        assert m["F1"] == pytest.approx(f1_score(yt, yp, average="macro", zero_division=0))


def test_present_confusion_is_sklearns_matrix():
    from sklearn.metrics import confusion_matrix
    _, C, yt, yp = _cases()[-2]
    assert np.array_equal(AlgorithmBase._present_confusion(_confusion(yt, yp, C)), confusion_matrix(yt, yp))
    _, C, yt, yp = _cases()[4]
    assert np.array_equal(AlgorithmBase._present_confusion(_confusion(yt, yp, C)), confusion_matrix(yt, yp))


# ---- 2. hook logic on a stub ------------------------------------------------------------------------------------------------------------
class _Tb:
    def __init__(self):
        self.calls = []

    def update(self, d, it):
        self.calls.append((dict(d), it))


class _Stub:
    """What the three hooks touch on an algorithm, recording."""

    def __init__(self, accs=(), num_eval_iter=3, num_log_iter=2, num_train_iter=7, rank=0, distributed=False, test=False, save_dir="/nowhere",
                 tb=False):
        self.it, self.epoch, self.epochs = 0, 0, 1
        self.num_train_iter, self.num_eval_iter, self.num_log_iter = num_train_iter, num_eval_iter, num_log_iter
        self.log_dict = {}
        self.best_eval_metric, self.best_it = 0.0, 0
        self.ema_m = 0.0
        self.rank, self.distributed, self.ngpus_per_node = rank, distributed, 8
        self.save_dir, self.save_name = save_dir, "run"
        self.loader_dict = {"eval": [], **({"test": []} if test else {})}
        self.tb_log = _Tb() if tb else None
        self.accs = list(accs)
        self.events, self.lines = [], []

    def print_fn(self, s):
        self.lines.append(s)

    def evaluate(self, dest="eval"):
        self.events.append(("evaluate", dest, self.it))
        acc = self.accs.pop(0) if dest == "eval" else 0.625
        return {dest + "/loss": 1.5, dest + "/top-1-acc": acc}

    def save_model(self, name, path):
        self.events.append(("save", name, path, self.it))

    def load_model(self, path):
        self.events.append(("load", path))


def _run(stub, hooks, steps=None):
    for it in range(stub.num_train_iter if steps is None else steps):
        stub.it = it
        stub.log_dict = {"train/sup_loss": 0.25 + it}
        for h in hooks:
            h.after_train_step(stub)


def test_hook_base_helpers():
    h, s = Hook(), _Stub()
    s.it, s.epoch, s.epochs = 6, 1, 2
    assert h.is_last_iter(s) and h.is_last_epoch(s) and h.every_n_epochs(s, 2) and not h.every_n_epochs(s, 0) and not h.every_n_epochs(s, 3)
    s.it, s.epoch = 5, 0
    assert not h.is_last_iter(s) and not h.is_last_epoch(s) and h.every_n_iters(s, 3) and not h.every_n_iters(s, 0)


@pytest.mark.parametrize("n,expected", [(0, [6]), (3, [2, 5, 6])])
def test_evaluation_and_checkpoint_cadence(n, expected):
    s = _Stub(accs=[0.0] * 7, num_eval_iter=n)
    _run(s, [EvaluationHook(), CheckpointHook()])
    assert [e[2] for e in s.events if e[0] == "evaluate"] == expected
    assert [e[3] for e in s.events if e[0] == "save" and e[1] == "latest_model.pth"] == expected
    assert s.lines == ["validating..."] * len(expected)


def test_best_metric_needs_strict_improvement_and_saves_latest_then_best():
    s = _Stub(accs=[0.5, 0.5, 0.75], num_eval_iter=3, save_dir="/ckpt")
    _run(s, [EvaluationHook(), CheckpointHook()])
    path = os.path.join("/ckpt", "run")
    assert s.events == [("evaluate", "eval", 2), ("save", "latest_model.pth", path, 2), ("save", "model_best.pth", path, 2),
                        ("evaluate", "eval", 5), ("save", "latest_model.pth", path, 5),                   # 0.5 again: not an improvement
                        ("evaluate", "eval", 6), ("save", "latest_model.pth", path, 6), ("save", "model_best.pth", path, 6)]
    assert (s.best_eval_metric, s.best_it) == (0.75, 6)
    assert s.log_dict["eval/top-1-acc"] == 0.75 and s.log_dict["eval/loss"] == 1.5 and s.log_dict["train/sup_loss"] == 6.25   # merged
    # an evaluation that never beats 0 never becomes "best" -- except that best_it starts at 0, as in the reference: a save at it == 0 is "best"
    z = _Stub(accs=[0.0] * 3, num_eval_iter=3)
    _run(z, [EvaluationHook(), CheckpointHook()])
    assert (z.best_eval_metric, z.best_it) == (0.0, 0) and not [e for e in z.events if e[1] == "model_best.pth"]


def test_non_leading_rank_saves_and_prints_nothing():
    s = _Stub(accs=[0.5, 0.6, 0.7], rank=3, distributed=True, tb=True)
    _run(s, [EvaluationHook(), CheckpointHook(), LoggingHook()])
    EvaluationHook().after_run(s)
    assert not [e for e in s.events if e[0] == "save"] and [e[2] for e in s.events if e[0] == "evaluate"] == [2, 5, 6]
    assert s.lines == ["validating..."] * 3 and len(s.tb_log.calls) == 4          # it evaluates and feeds its tb_log, it does not write
    lead = _Stub(accs=[0.5, 0.6, 0.7], rank=8, distributed=True)                   # first rank of the second node
    _run(lead, [EvaluationHook(), CheckpointHook()])
    assert len([e for e in lead.events if e[0] == "save"]) == 6


def test_after_run_results(tmp_path):
    s = _Stub(save_dir=str(tmp_path))
    s.best_eval_metric, s.best_it, s.it = 0.75, 5, 7
    EvaluationHook().after_run(s)
    assert s.events == [("save", "latest_model.pth", os.path.join(str(tmp_path), "run"), 7)]
    assert s.results_dict == {"eval/best_acc": 0.75, "eval/best_it": 5}
    # a test loader and a model_best.pth: loaded, evaluated on 'test'
    t = _Stub(save_dir=str(tmp_path), test=True)
    t.best_eval_metric, t.best_it = 0.75, 5
    os.makedirs(tmp_path / "run")
    best = tmp_path / "run" / "model_best.pth"
    best.write_bytes(b"")
    EvaluationHook().after_run(t)
    assert t.events[1:] == [("load", str(best)), ("evaluate", "test", 0)]
    assert t.results_dict == {"eval/best_acc": 0.75, "eval/best_it": 5, "test/best_acc": 0.625}
    # ... and without the file: one line, no load, no test/best_acc
    best.unlink()
    m = _Stub(save_dir=str(tmp_path), test=True)
    EvaluationHook().after_run(m)
    assert [e[0] for e in m.events] == ["save"] and m.results_dict == {"eval/best_acc": 0.0, "eval/best_it": 0}
    assert len(m.lines) == 1 and "model_best.pth" in m.lines[0]


def test_logging_lines_are_the_references():
    class _Lazy:                                                       # a deferred log scalar: only __format__ / __float__
        def __format__(self, spec): return format(0.123456, spec)
        def __float__(self): return 0.123456

    s = _Stub(num_eval_iter=3, num_log_iter=2, tb=True)
    s.ema_m = 0.999
    s.best_eval_metric, s.best_it = 0.5, 2
    h = LoggingHook()
    fixed = {"train/sup_loss": 1.0, "train/util_ratio": _Lazy(), "lr": 0.00049999, "eval/top-1-acc": 0.5}
    for it in range(4):
        s.it, s.log_dict = it, dict(fixed)
        h.after_train_step(s)
    body = "train/sup_loss: 1.0000, train/util_ratio: 0.1235, lr: 0.0005, eval/top-1-acc: 0.5000 "
    assert s.lines == ["2 iteration USE_EMA: True, " + body,
                       "3 iteration, USE_EMA: True, " + body + "BEST_EVAL_ACC: 0.5000, at 3 iters",
                       "4 iteration USE_EMA: True, " + body]
    assert [it for _, it in s.tb_log.calls] == [1, 2, 3]
    assert s.tb_log.calls[0][0] == {"train/sup_loss": 1.0, "train/util_ratio": 0.123456, "lr": 0.00049999, "eval/top-1-acc": 0.5}
    assert all(type(v) is float for v in s.tb_log.calls[0][0].values())
    # no cadence, no line; ema_m == 0 prints False
    q = _Stub(num_eval_iter=0, num_log_iter=0)
    _run(q, [h])
    assert q.lines == []
    q = _Stub(num_eval_iter=0, num_log_iter=7)
    _run(q, [h])
    assert q.lines == ["7 iteration USE_EMA: False, train/sup_loss: 6.2500 "]


# ---- 3. registration --------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    d = dict(algorithm="hostonly", num_classes=10, num_train_iter=6, epoch=2, ema_m=0.0, ulb_loss_ratio=1.0, use_cat=True, amp=False, lr=5e-4,
             num_eval_iter=0, num_log_iter=0, gpu=None, rank=0, world_size=1, distributed=False, dataset=None, num_labels=12, batch_size=4,
             uratio=2, eval_batch_size=4, img_size=8, data_functions=(None, None))
    d.update(kw)
    return argparse.Namespace(**d)


class _HostOnly(AlgorithmBase):
    """The base class's wiring with a backbone that is never launched (CPU device) and no optimizer."""

    def set_model(self):
        return vit.VisionTransformer(vit.VitConfig(img_size=8, patch_size=2, embed_dim=128, depth=2, num_heads=2, num_classes=self.num_classes),
                                     device="cpu")

    def set_ema_model(self):
        return self.model

    def set_optimizer(self):
        return None, None

    def train_step(self, x_lb, y_lb, idx_ulb, x_ulb_w, x_ulb_s):
        raise AssertionError("not stepped")


def test_registration_order_and_defaults():
    for kw in (dict(), dict(run_hooks=False), dict(device_eval=True)):
        alg = _HostOnly(_args(**kw), None)
        assert list(alg.hooks_dict) == ["ParamUpdateHook", "EMAHook", "TimerHook"]
        assert alg.run_hooks is False and alg.device_eval is bool(kw.get("device_eval", False))
    alg = _HostOnly(_args(run_hooks=True), None)
    assert [type(h) for h in alg.hooks_dict.values()] == [ParamUpdateHook, EMAHook, EvaluationHook, CheckpointHook, TimerHook, LoggingHook]
    assert list(alg.hooks_dict) == ["ParamUpdateHook", "EMAHook", "EvaluationHook", "CheckpointHook", "TimerHook", "LoggingHook"]
    assert alg.device_eval is False and alg.ngpus_per_node >= 1
    # independent of device_data: its DistSamplerSeedHook (NORMAL) goes between the HIGH and the LOWEST hooks, as in the reference
    rng = np.random.Generator(np.random.PCG64(2))
    mk = lambda n: rng.integers(0, 256, size=(n, 8, 8, 3)).astype(np.uint8)      # noqa: E731
    dd = {"train_lb": {"data": mk(12), "targets": rng.integers(0, 10, size=12)}, "train_ulb": {"data": mk(40), "targets": None},
          "eval": {"data": mk(6), "targets": rng.integers(0, 10, size=6)}, "test": None}
    alg = _HostOnly(_args(run_hooks=True, device_data=True, dataset="eurosat", dataset_dict=dd, train_sampler="RandomSampler", crop_ratio=0.875,
                          seed=3), None)
    assert [type(h) for h in alg.hooks_dict.values()] == [ParamUpdateHook, EMAHook, EvaluationHook, CheckpointHook, DistSamplerSeedHook,
                                                          TimerHook, LoggingHook]
