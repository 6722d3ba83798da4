"""What tests/_rewarder_cases.py promises about its inputs, asserted on the float64 reference (no GPU): the attention softmax is peaked, the
rewards and generated labels differ between rows, no ReLU input of a backward case sits near its kink -- and the bounds that
tests/test_gpu_rewarder_kernels.py commits are 8 times the float32 oracle's own deviation from float64, measured afresh here."""
import ast
import os
import re

import numpy as np
import pytest
import torch

import _rewarder_cases as RC
from oracle import semireward_ref as S

IDS = lambda cs: [c["id"] for c in cs]  # noqa: E731


@pytest.mark.parametrize("c", RC.FORWARD + RC.BACKWARD, ids=IDS(RC.FORWARD) + ["bwd_" + i for i in IDS(RC.BACKWARD)])
def test_rewarder_inputs_exercise_the_softmax(c):
    inp = RC.rewarder_inputs(c)
    B = c["B"]
    for g, m in enumerate(RC.forward_ref(c, inp)):
        lab = inp["labels"][g * B:(g + 1) * B]
        std = float(np.std(m["logits"], ddof=1))
        peak = float(m["alpha"].max()) * 2 * B
        print("%s group %d: logit std %.2f, max(alpha) * 2B %.2f, rewards %.3f .. %.3f" % (c["id"], g, std, peak, m["reward"].min(), m["reward"].max()))
        if c["sat"]:
            assert std >= 40.0
            assert np.abs(m["logits"]).max() > 104.0         # float32 exp() of the raw logit overflows, or underflows to 0: needs the max-subtraction
        else:
            assert 1.5 <= std <= 4.0
            # max(alpha) * 2B cannot exceed 2B: below B = 3 the same peakedness reads "one row holds 85 % of the weight"
            assert peak >= min(5.0, 0.85 * 2 * B)
        if B >= 8 and not c["same_labels"]:              # (rows differ only through their labels: equal labels, equal rewards)
            assert m["reward"].min() <= 0.2 and m["reward"].max() >= 0.8
        if c["same_labels"]:
            assert len(set(lab.tolist())) == 1
        assert 0 <= lab.min() and lab.max() < c["C"]
    if c["G"] > 1:                                       # groups get different features and labels
        assert not np.array_equal(inp["feats"][:B], inp["feats"][B:2 * B]) and not np.array_equal(inp["labels"][:B], inp["labels"][B:2 * B])
    t = inp["target"]
    assert set(t.tolist()) <= {0.5, 1.0} and (B == 1 or set(t.tolist()) == {0.5, 1.0})


@pytest.mark.parametrize("c", RC.BACKWARD, ids=IDS(RC.BACKWARD))
def test_backward_inputs_stay_off_the_relu_kinks(c):
    """Every float64 ReLU input (mlp_fc1, ffn_fc1) at least KINK_FACTOR times as far from 0 as the float32 oracle strays from float64 on those
    tensors: a float32 kernel cannot land on the other side, so no gradient element needs an exclusion."""
    closest, dev = RC.kink_margin(c, RC.rewarder_inputs(c))
    print("%s: closest ReLU input %.3e, float32 deviation %.3e, ratio %.0f" % (c["id"], closest, dev, closest / dev))
    assert dev > 0.0 and closest >= RC.KINK_FACTOR * dev


@pytest.mark.parametrize("c", RC.GENERATOR, ids=IDS(RC.GENERATOR))
def test_generator_inputs_give_distinct_labels(c):
    out, pre = RC.generator_ref(c, RC.generator_inputs(c))
    print("%s: outputs %s" % (c["id"], np.array2string(out, precision=3)))
    assert len(set(np.floor(out).tolist())) >= (4 if c["B"] >= 8 else 2)
    assert (out == 0.0).any()                            # a ReLU-clamped row
    # distance to the nearest integer, taken before the last ReLU so that the clamped rows count too (they sit below -1e-3, not at 0)
    assert np.abs(pre - np.round(pre)).min() >= 1e-3
    assert np.array_equal(out, np.maximum(pre, 0.0))


def test_oracle_intermediates_are_the_forward():
    """rewarder_forward is rewarder_intermediates' reward bit for bit, and the named stages are consistent with each other."""
    c = RC.by_id(RC.FORWARD, "F100_C100_B13_G1")
    inp = RC.rewarder_inputs(c)
    p = {k: torch.from_numpy(v) for k, v in inp["params"].items()}
    x, y = torch.from_numpy(inp["feats"]), torch.from_numpy(inp["labels"])
    m = S.rewarder_intermediates(p, x, y)
    assert torch.equal(S.rewarder_forward(p, x, y), m["reward"])
    assert torch.equal(m["z"], torch.cat((m["h"], m["e"]))) and torch.equal(m["u"], m["ctx"].unsqueeze(0) + m["e"])
    assert torch.equal(m["m1"], torch.relu(m["m1_pre"])) and torch.equal(m["f1"], torch.relu(m["f1_pre"]))
    assert abs(float(m["alpha"].sum()) - 1.0) < 1e-6
    pre = x @ p["feature_fc.weight"].t() + p["feature_fc.bias"]
    var = pre.double().var(dim=1, unbiased=False)
    np.testing.assert_allclose(m["rstd"][:13].numpy(), (1.0 / torch.sqrt(var + 1e-5)).numpy(), rtol=1e-5)
    np.testing.assert_allclose(m["xhat"][:13].numpy(), ((pre - pre.mean(1, keepdim=True)) * m["rstd"][:13, None]).numpy(), rtol=1e-4, atol=1e-6)


def _docstring_table():
    """{row: (floor, bound)} as written in the module docstring of tests/test_gpu_rewarder_kernels.py"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_rewarder_kernels.py")
    with open(path) as f:
        doc = ast.get_docstring(ast.parse(f.read()))
    rows = re.findall(r"^\s*([a-z_0-9/]+)\s+([0-9.]+e-[0-9]+)\s+([0-9.]+e-[0-9]+)\s", doc, flags=re.M)
    return {k: (float(a), float(b)) for k, a, b in rows}


def test_committed_bounds_are_eight_float32_floors():
    """The committed floors are the float32 oracle's deviation as measured here, within FLOOR_HEADROOM from both sides; every bound is exactly
    8 times its floor (at least 1e-7); the docstring table of the GPU tests states the same figures."""
    floors = RC.float32_floors()
    table = _docstring_table()
    for k in sorted(floors):
        print("%-14s measured %.3e   floor %.2e   bound %.2e" % (k, floors[k], RC.FLOORS.get(k, float("nan")), RC.BOUNDS.get(k, float("nan"))))
    assert set(floors) == set(RC.FLOORS) == set(RC.BOUNDS) == set(table)
    for k, f in RC.FLOORS.items():
        assert f * (1.0 - RC.FLOOR_HEADROOM) <= floors[k] <= f * (1.0 + RC.FLOOR_HEADROOM), (k, floors[k], f)
        assert RC.BOUNDS[k] == max(8.0 * f, 1e-7), k
        assert table[k] == (float("%.2e" % f), float("%.2e" % RC.BOUNDS[k])), (k, table[k])
