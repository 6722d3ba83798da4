"""The pseudo-label monitor's host side without a GPU: the C ABI and its documented state layout, the option checks, that the key absent
changes nothing, the metrics derived from the counts (against brute force over rows), reward_auc from the histograms, empty denominators, and
that the numpy restatement the GPU tests trust tells three planted faults apart."""
import argparse
import math
import os
import re

import numpy as np
import pytest
import torch

import _pl_monitor_cases as PC
from semireward_amd import _lib, ops
from semireward_amd.core.algorithmbase import AlgorithmBase, DeferredScalar
from semireward_amd.core.pl_monitor import HEADER, LOG_KEYS, PlMonitor
from semireward_amd.nets import vit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_TEXT = open(os.path.join(ROOT, "include", "srhip.h")).read()


# ---- 1. ABI -------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_documents_the_state():
    m = re.search(r"int srhip_pl_monitor\(([^;]*)\);", HEADER_TEXT)
    assert m, "srhip_pl_monitor is not declared in include/srhip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 14 and params[-1] == "void* stream"
    assert [p.split()[-1].lstrip("*") for p in params[:7]] == ["pseudo", "mask0", "mask_kept", "mask2", "reward", "idx_ulb", "ulb_targets"]
    doc = HEADER_TEXT[:m.start()].rsplit("/*", 1)[1]
    assert "istate int64 [16 + 2 * C + 64]" in doc and "fstate double [4]" in doc
    for i, name in enumerate(HEADER):                      # every header word is documented at the index the host reads it from
        assert "[%d] %s" % (i, name) in doc, (i, name)
    for word in ("sel_by_class", "sel_correct_by_class", "hist[0]", "hist[1]", "sum_w_correct", "sum_r[0]", "sum_r[1]", "reward_bad", "bit 5",
                 "SR_EINVAL"):
        assert word in doc, word
    assert HEADER == PC.COUNTS


def test_signature_table_and_wrapper():
    res, args = _lib.SIGNATURES["srhip_pl_monitor"]
    assert res is _lib.I and len(args) == 14
    assert args[7] is _lib.c_longlong and args[8:11] == [_lib.I] * 3 and all(a is _lib.P for a in args[:7] + args[11:])
    assert callable(ops.pl_monitor)
    assert ops.pl_monitor_words(10) == 16 + 20 + 64 and (ops.PL_HEADER_WORDS, ops.PL_BINS, ops.PL_SUMS) == (16, 32, 4)
    assert len(HEADER) <= ops.PL_HEADER_WORDS
    assert any("monitor" in m for m in ops._LABEL_ERR) and len(ops._LABEL_ERR) == 6          # bit 5 of the label-error word


# ---- 2. options ---------------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    d = dict(algorithm="hostonly", num_classes=10, num_train_iter=6, epoch=2, ema_m=0.0, ulb_loss_ratio=1.0, use_cat=True, amp=False, lr=5e-4,
             num_eval_iter=0, num_log_iter=0, gpu=None, rank=0, world_size=1, distributed=False, dataset=None, num_labels=12, batch_size=4,
             uratio=2, eval_batch_size=4, img_size=8, data_functions=(None, None), ulb_dest_len=40)
    d.update(kw)
    return argparse.Namespace(**d)


class _HostOnly(AlgorithmBase):
    """The base class's wiring with a backbone that is never launched and no optimizer."""

    def set_model(self):
        return vit.VisionTransformer(vit.VitConfig(img_size=8, patch_size=2, embed_dim=128, depth=2, num_heads=2, num_classes=self.num_classes),
                                     device="cpu")

    def set_ema_model(self):
        return self.model

    def set_optimizer(self):
        return None, None

    def train_step(self, x_lb, y_lb, x_ulb_w, x_ulb_s):
        raise AssertionError("not stepped")


def test_option_validation():
    with pytest.raises(ValueError, match="ulb_targets"):
        _HostOnly(_args(monitor_pseudo_labels=True), None)
    with pytest.raises(ValueError, match="ulb_targets"):
        _HostOnly(_args(monitor_pseudo_labels=True, ulb_targets=None), None)
    with pytest.raises(ValueError, match="39 entries.*40"):
        _HostOnly(_args(monitor_pseudo_labels=True, ulb_targets=np.zeros(39, np.int64)), None)
    with pytest.raises(ValueError, match="int array"):
        _HostOnly(_args(monitor_pseudo_labels=True, ulb_targets=np.zeros(40, np.float32)), None)
    t = np.arange(40) % 10
    t[3] = -1
    for given in (t, t.astype(np.int32), list(t), torch.from_numpy(t)):
        alg = _HostOnly(_args(monitor_pseudo_labels=True, ulb_targets=given), None)
        mon = alg.pl_monitor
        assert isinstance(mon, PlMonitor) and mon.targets.dtype == torch.int64 and mon.targets.tolist() == t.tolist()
        assert mon.block.dtype == torch.int64 and mon.block.numel() == 16 + 20 + 64 + 4 and not mon.block.any()
        assert mon.istate.data_ptr() == mon.block.data_ptr() and mon.fstate.dtype == torch.float64 and mon.fstate.numel() == 4
        assert mon.fstate.data_ptr() == mon.block.data_ptr() + 8 * 100


def test_a_batch_without_idx_ulb_is_refused_and_idx_ulb_is_kept_aside():
    t = np.arange(40) % 10
    alg = _HostOnly(_args(monitor_pseudo_labels=True, ulb_targets=t), None)
    x = torch.zeros(2, 3)
    out = alg.process_batch(x_lb=x, y_lb=torch.zeros(2, dtype=torch.int64), x_ulb_w=x, x_ulb_s=x, idx_ulb=torch.tensor([5, 7]))
    assert "idx_ulb" not in out and alg._monitor_idx_ulb.tolist() == [5, 7]          # train_step does not take it: the filter dropped it
    alg.process_batch(x_lb=x, y_lb=torch.zeros(2, dtype=torch.int64), x_ulb_w=x, x_ulb_s=x)
    assert alg._monitor_idx_ulb is None
    with pytest.raises(ValueError, match="idx_ulb"):
        alg.monitor_step(0, [x[:, 0]], torch.zeros(2, dtype=torch.int64), None, None)


def test_key_absent_adds_nothing(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the monitor was touched with the key off")
    monkeypatch.setattr(PlMonitor, "__init__", boom)
    monkeypatch.setattr(PlMonitor, "check_targets", staticmethod(boom))
    monkeypatch.setattr(ops, "pl_monitor", boom)
    ref = set(vars(_HostOnly(_args(), None)))
    for kw in (dict(), dict(monitor_pseudo_labels=False), dict(ulb_targets=np.zeros(40, np.int64)), dict(monitor_pseudo_labels=False, ulb_targets=None)):
        alg = _HostOnly(_args(**kw), None)
        assert not hasattr(alg, "pl_monitor") and not hasattr(alg, "_monitor_idx_ulb")
        assert set(vars(alg)) == ref                                              # no attribute at all
        x = torch.zeros(2, 3)
        out = alg.process_batch(x_lb=x, y_lb=torch.zeros(2, dtype=torch.int64), x_ulb_w=x, x_ulb_s=x, idx_ulb=torch.tensor([5, 7]))
        assert sorted(out) == ["x_lb", "x_ulb_s", "x_ulb_w", "y_lb"] and not hasattr(alg, "_monitor_idx_ulb")


# ---- 3. metrics from the counts -------------------------------------------------------------------------------------------------------------
def brute(case, fault=None):
    """Row by row in plain Python, with optional planted faults: the metrics and the state's integers, no numpy reductions."""
    P, nu, C, K = case["P"], case["nu"], case["C"], case["P"] - 1
    pseudo, idx, tg = case["pseudo"].reshape(P, nu), case["idx_ulb"], case["targets"]
    n = dict(rows=0, rows_correct=0, sel=0, sel_correct=0, conf_sel=0, conf_sel_correct=0, m2=0, m2_correct=0, rows_unknown=0, reward_bad=0)
    sum_w = sum_wc = 0.0
    hist = [[0] * 32, [0] * 32]
    rs = [[], []]
    for j in range(nu):
        y = int(tg[idx[j]])
        if y < 0:
            n["rows_unknown"] += 1
            continue
        pl = int(pseudo[0 if fault == "pass0_labels" else K, j])
        w = np.float32(case["masks"][K][j])
        if K > 0 and fault != "ignore_mask2":
            w = np.float32(w * np.float32(case["mask2"][(K - 1) * nu + j]))
        n["rows"] += 1
        n["rows_correct"] += pl == y
        n["sel"] += bool(w > 0)
        n["sel_correct"] += bool(w > 0) and pl == y
        sum_w += float(w)
        sum_wc += float(w) if pl == y else 0.0
        if case["masks"][0][j] > 0:
            n["conf_sel"] += 1
            n["conf_sel_correct"] += int(pseudo[0, j]) == y
        for g in range(K):
            r, ok = np.float32(case["reward"][g * nu + j]), int(pseudo[g + 1, j]) == y
            if case["mask2"][g * nu + j] > 0:
                n["m2"] += 1
                n["m2_correct"] += ok
            if not (r >= 0 and r <= 1):
                n["reward_bad"] += 1
                continue
            b = min(int(r * np.float32(32.0)) + (1 if fault == "bin_plus_one" else 0), 31)
            hist[ok][b] += 1
            rs[ok].append(float(r))
    return n, sum_w, sum_wc, hist, rs


def pair_auc(right, wrong):
    """P(right > wrong) + 0.5 P(right == wrong) over every pair, exactly."""
    if not right or not wrong:
        return float("nan")
    s = sum((a > b) + 0.5 * (a == b) for a in right for b in wrong)
    return s / (len(right) * len(wrong))


CPU_SHAPES = [(1, 7, 10), (3, 5, 4), (9, 56, 100), (2, 300, 10)]


@pytest.mark.parametrize("P,nu,C", CPU_SHAPES)
@pytest.mark.parametrize("soft", [False, True])
def test_metrics_from_state_against_brute_force(P, nu, C, soft):
    case = PC.make_case(P, nu, C, seed=3, soft=soft)
    st = PC.restate(case)
    n, sum_w, sum_wc, hist, rs = brute(case)
    assert not st["flag"] and all(st[k] == v for k, v in n.items()), {k: (st[k], v) for k, v in n.items() if st[k] != v}
    assert st["hist"].tolist() == hist and st["sel_by_class"].sum() == st["sel"] and st["sel_correct_by_class"].sum() == st["sel_correct"]
    m = PlMonitor.metrics_from_state(st)
    assert tuple(m) == LOG_KEYS
    rat = lambda a, b: a / b if b else float("nan")      # noqa: E731
    centre = lambda v: (min(int(np.float32(v) * np.float32(32.0)), 31) + 0.5) / 32.0      # noqa: E731
    want = dict(pl_acc=rat(n["rows_correct"], n["rows"]), select_ratio=rat(sum_w, n["rows"]), select_acc=rat(sum_wc, sum_w),
                conf_select_acc=rat(n["conf_sel_correct"], n["conf_sel"]), reward_filter_acc=rat(n["m2_correct"], n["m2"]),
                reward_mean_correct=rat(sum(rs[1]), len(rs[1])), reward_mean_wrong=rat(sum(rs[0]), len(rs[0])),
                reward_auc=pair_auc([centre(v) for v in rs[1]], [centre(v) for v in rs[0]]))
    for k in LOG_KEYS:
        if math.isnan(want[k]):
            assert math.isnan(m[k]), k
        else:
            assert m[k] == pytest.approx(want[k], rel=1e-12, abs=1e-15), k
    if (P - 1) * nu >= 200:                              # (smaller cases hold little beside the planted edge values)
        assert m["reward_mean_correct"] > m["reward_mean_wrong"] and m["reward_auc"] > 0.5         # the cases separate right from wrong


def test_reward_auc_equals_the_pairwise_auc_on_bin_centres():
    rng = np.random.Generator(np.random.PCG64(11))
    for trial in range(6):
        nr, nw = int(rng.integers(1, 400)), int(rng.integers(1, 400))
        br = np.minimum((rng.beta(3, 2, size=nr) * 32).astype(np.int64), 31)
        bw = np.minimum((rng.beta(2, 3, size=nw) * 32).astype(np.int64), 31)
        if trial == 0:
            br[:], bw[:] = 31, 0                                                     # perfectly separated
        if trial == 1:
            br[:] = bw[:1]
            bw[:] = bw[0]                                                            # one bin: 0.5
        st = PC.empty_state(4)
        np.add.at(st["hist"][1], br, 1)
        np.add.at(st["hist"][0], bw, 1)
        got = PlMonitor.metrics_from_state(st)["reward_auc"]
        want = pair_auc(list((br + 0.5) / 32.0), list((bw + 0.5) / 32.0))
        assert abs(got - want) <= 1e-12, (trial, got, want)
        if trial == 0:
            assert got == 1.0
        if trial == 1:
            assert got == 0.5


def test_empty_denominators_give_nan():
    m = PlMonitor.metrics_from_state(PC.empty_state(5))
    assert tuple(m) == LOG_KEYS and all(math.isnan(v) for v in m.values())
    st = PC.restate(PC.make_case(3, 9, 4, seed=1, unknown=1.0))                     # every row unknown
    assert st["rows_unknown"] == 9 and st["rows"] == 0 and st["gen_rows"] == 0
    assert all(math.isnan(v) for v in PlMonitor.metrics_from_state(st).values())
    st = PC.restate(PC.make_case(1, 30, 4, seed=2))                                 # K = 0: nothing about rewards
    m = PlMonitor.metrics_from_state(st)
    assert not math.isnan(m["pl_acc"]) and not math.isnan(m["select_acc"])
    assert all(math.isnan(m[k]) for k in ("reward_filter_acc", "reward_mean_correct", "reward_mean_wrong", "reward_auc"))
    st = PC.empty_state(3)
    st["hist"][1][4] = 7                                                            # right rows only: no pair
    st["sum_r"][1] = 1.0
    m = PlMonitor.metrics_from_state(st)
    assert math.isnan(m["reward_auc"]) and math.isnan(m["reward_mean_wrong"]) and m["reward_mean_correct"] == 1.0 / 7


def test_state_words_round_trip():
    C = 6
    st = PC.restate(PC.make_case(4, 33, C, seed=5, soft=True))
    W = ops.pl_monitor_words(C)
    h = np.zeros(W + 4, np.int64)
    for i, k in enumerate(HEADER):
        h[i] = st[k]
    h[16:16 + C], h[16 + C:16 + 2 * C], h[16 + 2 * C:W] = st["sel_by_class"], st["sel_correct_by_class"], st["hist"].reshape(-1)
    h[W:] = np.array([st["sum_w"], st["sum_w_correct"], st["sum_r"][0], st["sum_r"][1]]).view(np.int64)
    back = PlMonitor.state_from_words(h, C)
    assert not PC.state_equal_ints(back, st)
    assert (back["sum_w"], back["sum_w_correct"]) == (st["sum_w"], st["sum_w_correct"]) and back["sum_r"].tolist() == st["sum_r"].tolist()


# ---- 4. lazy log values -----------------------------------------------------------------------------------------------------------------------
def test_log_values_share_one_read_per_step(monkeypatch):
    mon = PlMonitor(np.zeros(8, np.int64), 3, "cpu", 8)
    reads = []

    def fake_read(reset=True):
        reads.append(reset)
        return {"metrics": {k: float(len(reads)) for k in LOG_KEYS}}
    monkeypatch.setattr(mon, "read", fake_read)
    a = mon.log_values(7)
    assert tuple(a) == LOG_KEYS and all(isinstance(v, DeferredScalar) for v in a.values()) and reads == []      # nobody read: no copy
    assert [float(v) for v in a.values()] == [1.0] * 8 and reads == [True]
    assert "%.2f" % a["pl_acc"] == "1.00" and a["reward_auc"] + 1 == 2.0 and reads == [True]
    again = mon.log_values(7)                                                         # the same step index: the same copy
    assert float(again["select_acc"]) == 1.0 and reads == [True]
    skipped = mon.log_values(8)                                                       # a step nobody reads
    b = mon.log_values(9)
    assert float(b["pl_acc"]) == 2.0 and float(b["reward_auc"]) == 2.0 and reads == [True, True]
    # an older line read after a newer one: its steps went into that one's window; it reads nan and does not touch the running window
    assert all(math.isnan(float(v)) for v in skipped.values()) and math.isnan(float(mon.log_values(3)["pl_acc"])) and reads == [True, True]
    assert float(mon.log_values(9)["pl_acc"]) == 2.0 and reads == [True, True]
    mon.restart()                                                                     # (load_model: a resumed run may step back)
    assert float(mon.log_values(3)["pl_acc"]) == 3.0 and reads == [True, True, True]


# ---- 5. the restatement tells planted faults apart ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", ["ignore_mask2", "pass0_labels", "bin_plus_one"])
def test_restatement_rejects_planted_faults(fault):
    hit = 0
    for P, nu, C in [(3, 5, 4), (9, 56, 100), (2, 300, 10)]:
        case = PC.make_case(P, nu, C, seed=3)
        st = PC.restate(case)
        n, sum_w, sum_wc, hist, _ = brute(case)
        assert all(st[k] == v for k, v in n.items()) and st["hist"].tolist() == hist and abs(st["sum_w"] - sum_w) <= 1e-9
        n, sum_w, sum_wc, hist, _ = brute(case, fault)
        differs = any(st[k] != v for k, v in n.items()) or st["hist"].tolist() != hist or abs(st["sum_w"] - sum_w) > 1e-9
        assert differs, (fault, P, nu, C)
        hit += differs
    assert hit == 3
