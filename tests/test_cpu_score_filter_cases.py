"""What tests/_score_filter_cases.py promises about its cases, asserted on the float64 restatements (no GPU): every stride, cap and reduction path of
csrc/score_filter.hip that the cases are there for is reached (derived from B, C and n_all), both lerp branches of the quantile occur, the planted
conditions hold, no row sits near a threshold -- and the bounds that tests/test_gpu_score_filter_kernels.py commits are 8 times the float32
evaluation's own deviation from float64, measured afresh here, and reject every wrong version of _score_filter_cases.WRONG."""
import ast
import os
import re

import numpy as np
import pytest
import torch

import _score_filter_cases as SC

F32, F64 = np.float32, np.float64
IDS = lambda cs: [c["id"] for c in cs]  # noqa: E731


def _any(cases, f):
    return any(f(c) for c in cases)


def test_cases_reach_every_stride_cap_and_path():
    """The launch geometry of csrc/score_filter.hip, restated: 256 threads, 4 waves of 64, one wave per row; freematch_stats one thread per
    class on ceil(C / 256) workgroups; caps srt[1024], pred[1024] / rowloss[1024], g[2048]; masked_ce's other reduction from B = 1025 on;
    reward_mask2 left to right up to 64 rows, per-lane partials above."""
    for cases in (SC.ROWS, SC.STATS, SC.FREEMATCH, SC.ENTROPY, SC.DISTALIGN, SC.MASKED_CE):
        cs = {c["C"] for c in cases}
        assert {1, 2, 63, 64, 65, 256, 257, 1000, 2048} <= cs, (cases[0]["id"], sorted(cs))          # idle lanes; one-wave boundary; `c += 256`; caps
        assert _any(cases, lambda c: c["B"] < 4) and _any(cases, lambda c: c["B"] == 1)                # fewer rows than waves
    for cases in (SC.ROWS, SC.STATS, SC.FREEMATCH, SC.ENTROPY, SC.DISTALIGN, SC.SOFTMATCH, SC.MASKED_CE):
        bs = {c["B"] for c in cases}
        assert {1, 3, 5, 64, 65, 257, 1024} <= bs, (cases[0]["id"], sorted(bs))
    big = [c for cases in (SC.ROWS, SC.STATS, SC.FREEMATCH, SC.ENTROPY, SC.DISTALIGN, SC.MASKED_CE) for c in cases]
    assert max(c["B"] * c["C"] for c in big) <= 65 * 256                                               # the large shapes are not crossed
    # the second workgroup of freematch_stats, the second `c += 256` stride of update / entropy / distalign
    for cases in (SC.STATS, SC.FREEMATCH, SC.ENTROPY, SC.DISTALIGN):
        assert _any(cases, lambda c: c["C"] == 256) and _any(cases, lambda c: c["C"] > 256)
    assert _any(SC.ENTROPY, lambda c: c["C"] == 2048) and _any(SC.ENTROPY, lambda c: c["B"] == 1024) and max(c["C"] for c in SC.ENTROPY) <= 2048
    # masked_ce: rowloss[] filled to its cap, and the per-wave acc / part[4] path past it
    assert _any(SC.MASKED_CE, lambda c: c["B"] == 1024) and _any(SC.MASKED_CE, lambda c: c["B"] == 1025)
    assert all(c["B"] <= 1024 for cases in (SC.FREEMATCH, SC.ENTROPY) for c in cases)
    for k in (0, 1, 2):
        assert _any(SC.MASKED_CE, lambda c: c["masks"] == k)
    # n_all != B: 4 B and an odd multiple; the srt[] cap; every quantile size the issue names
    for cases in (SC.FREEMATCH, SC.SOFTMATCH):
        assert _any(cases, lambda c: c["ranks"] == 4) and _any(cases, lambda c: c["ranks"] > 1 and c["ranks"] % 2 == 1)
    assert _any(SC.DISTALIGN, lambda c: c["ranks"] == 4) and _any(SC.DISTALIGN, lambda c: c["ranks"] == 3)
    qn = {c["n_all"] for c in SC.FREEMATCH if c["uq"]}
    assert {1, 2, 3, 4, 6, 11, 257, 1024} <= qn and max(c["n_all"] for c in SC.FREEMATCH) == 1024
    assert _any(SC.FREEMATCH, lambda c: c["uq"] and c["n_all"] == 1024 and c["B"] == 256)
    assert _any(SC.FREEMATCH, lambda c: not c["uq"] and c["ranks"] > 1) and _any(SC.FREEMATCH, lambda c: c["clip"])
    # momentum 0 and 0.5 beside the configs' value; one sequence of 3 to 4 calls at 0.5
    for cases in (SC.FREEMATCH, SC.DISTALIGN, SC.SOFTMATCH):
        assert {0.0, 0.5, SC.CONFIG_M} <= {c["m"] for c in cases}
        assert _any(cases, lambda c: c["m"] == 0.5 and 3 <= c["steps"] <= 4)
    assert _any(SC.DISTALIGN, lambda c: c["model"]) and _any(SC.DISTALIGN, lambda c: not c["model"]) and all(c["steps"] >= 2 for c in SC.DISTALIGN)
    # reward_mask2: both summation orders, mean_in and ragged on each
    for pick in (lambda c: c["mean_in"], lambda c: c["total"] != c["groups"] * c["Bg"], lambda c: not c["mean_in"]):
        assert _any(SC.REWARD, lambda c: pick(c) and c["Bg"] <= 64) and _any(SC.REWARD, lambda c: pick(c) and c["Bg"] > 64)
    assert {1, 64, 65, 257} <= {c["Bg"] for c in SC.REWARD}
    rag = [c for c in SC.REWARD if c["total"] != c["groups"] * c["Bg"]]
    assert _any(rag, lambda c: c["Bg"] > 64 and SC.group_rows(c, c["groups"] - 1) <= 64)               # a last group on the other path than its peers
    assert _any(SC.ENTROPY, lambda c: c["acc"] and c["gs"] != 1.0) and _any(SC.MASKED_CE, lambda c: c["gs"] != 1.0)


def test_both_lerp_branches_and_integral_ranks_occur():
    ws = {c["n_all"]: SC.lerp_weight(c["n_all"]) for c in SC.FREEMATCH if c["uq"]}
    print(ws)
    assert ws[2] >= 0.5 and ws[3] >= 0.5 and 0.0 < ws[4] < 0.5 and ws[1] == 0.0 and ws[6] == 0.0 and ws[11] == 0.0
    assert 0.5 <= ws[257] < 1.0 and 0.0 < ws[1024] < 0.5
    x = np.array([0.1, 0.2, 0.4, 0.8, 0.9], F64)
    assert abs(SC.quantile64(x) - float(torch.quantile(torch.from_numpy(x), 0.8))) < 1e-15 and abs(SC.quantile64(x[:4]) - np.quantile(x[:4], 0.8)) < 1e-15


def _no_near(what, near):
    assert int(np.sum(near)) == 0, "%s: %d rows within %g of their threshold" % (what, int(np.sum(near)), SC.NEAR)


def _mixed(mask):
    return 0.0 < float(np.mean(mask)) < 1.0


@pytest.mark.parametrize("c", SC.ROWS, ids=IDS(SC.ROWS))
def test_row_cases(c):
    inp = SC.row_inputs(c)
    ref = SC.row_ref(c, inp)
    _no_near(c["id"], SC.argmax_near(ref["gap"]))
    if c["B"] >= 8:
        pl = inp["planted"]
        assert set(pl) == set(SC.PLANTS if c["C"] >= 3 else [p for p in SC.PLANTS if p != "tie_three"])
        assert ref["gap"][pl["tie_first_last"]] == 0.0 and ref["idx"][pl["tie_first_last"]] == 0          # a tie for the maximum: the first index
        assert ref["maxp"][pl["onehot_pos"]] == 1.0 and ref["maxp"][pl["onehot_neg"]] == 1.0             # saturated rows
        assert np.ptp(ref["probs"][pl["all_equal"]]) == 0.0 and ref["idx"][pl["all_equal"]] == 0
    assert c["rpg"] < c["B"] or c["B"] <= 5                   # the strided form has more than one group
    assert c["pad"] > 0


@pytest.mark.parametrize("c", SC.FREEMATCH, ids=IDS(SC.FREEMATCH))
def test_freematch_cases(c):
    inp = SC.freematch_inputs(c)
    ref = SC.freematch_ref(c, inp)
    for t, r in enumerate(ref):
        _no_near("%s step %d" % (c["id"], t), r["near"])
        x = inp["steps"][t]["maxp_all"]
        if c["plant"] == "ones_block":                        # 12 max-probs of exactly 1.0f, ranks 28 .. 39, around rank 0.8 * 39 = 31.2
            assert (np.sort(x)[28:] == 1.0).all() and np.sort(x)[27] < 1.0 and 28 <= int(np.floor(0.8 * (c["n_all"] - 1))) < 39
            assert r["stat"] == 1.0
        if c["C"] == 1:
            assert (x == 1.0).all() and r["stat"] == 1.0      # all max-probs equal
        if c["B"] >= 8 and c["C"] > 1:
            assert _mixed(r["mask"]), c["id"]
        if c["ranks"] > 1:                                    # the statistics of all ranks differ from those of the local rows
            loc = SC.freematch_ref(c, inp, wrong="local_rows_only")[t]
            assert abs(loc["stat"] - r["stat"]) > 1e-4 and np.abs(loc["p_model"] - r["p_model"]).max() > 1e-4 * r["p_model"].max()
    if c["m"] == 0 and not c["uq"] and c["n_all"] == 1:       # the exact tie: kept, and by equality
        assert ref[0]["exact"].all() and ref[0]["mask"].all() and ref[0]["thr"][0] == ref[0]["conf"][0]
    if c["m"] == 0 and not c["clip"]:
        assert ref[0]["time_p"] == ref[0]["stat"]             # at m == 0 the state after one call IS the batch statistic
    if c["clip"] and c["plant"]:
        assert ref[0]["time_p"] == SC.CLIP_HI < ref[0]["stat"]


@pytest.mark.parametrize("c", SC.ENTROPY, ids=IDS(SC.ENTROPY))
def test_entropy_cases(c):
    inp = SC.entropy_inputs(c)
    ref = SC.entropy_ref(c, inp)
    sel = inp["mask"] != 0
    _no_near(c["id"], SC.argmax_near(ref["gap"]))
    assert int(sel.sum()) == {"all": c["B"], "none": 0, "one": 1}.get(c["sel"], int(sel.sum()))
    if c["sel"] == "some":
        assert 0 < sel.sum() < c["B"]
    if c["sel"] == "none":
        assert ref["loss"] == 0.0 and not ref["grad"].any()
        return
    if c["unpredicted"]:                                      # classes that rows predict, but no SELECTED row: h == 0, a = 0, mean_c > 0
        assert len(inp["dropped"]) == c["unpredicted"] and all((ref["pred"] == k).any() and not (ref["pred"][sel] == k).any() for k in inp["dropped"])
        assert (ref["h"][inp["dropped"]] == 0).all()
    if c["C"] > c["B"]:
        assert (ref["h"] == 0).any()
    assert int((inp["label_hist"] == 0).sum()) == c["lh_zeros"]
    if c["acc"]:
        assert c["gs"] != 1.0 and np.abs(inp["d0"]).max() > 0 and np.abs(inp["d0"]).max() < 10 * max(np.abs(ref["grad"]).max(), 1e-3)
    # the analytic form against float64 autograd of the oracle's loss (whose 1e-12 is a double: the loss moves by 4e-9 where a q_c is 0)
    loss, grad = SC.entropy_autograd(c, inp)
    assert abs(loss - ref["loss"]) <= 1e-8 * max(1.0, abs(loss)), (loss, ref["loss"])
    assert np.abs(grad - ref["grad"]).max() <= 1e-9 * max(np.abs(grad).max(), 1e-30), c["id"]
    if c["B"] >= 5 and c["sel"] != "one":
        assert np.abs(ref["grad"]).max() > 0.0


@pytest.mark.parametrize("c", SC.DISTALIGN, ids=IDS(SC.DISTALIGN))
def test_distalign_cases(c):
    ref = SC.distalign_ref(c, SC.distalign_inputs(c))
    for t, r in enumerate(ref):
        _no_near("%s step %d" % (c["id"], t), SC.argmax_near(r["gap"]))
        assert np.abs(r["aligned"].sum(axis=1) - 1.0).max() < 1e-12
    if c["model"]:
        assert np.abs(ref[-1]["p_target"] - 1.0 / c["C"]).max() > 0 or c["C"] == 1
    if c["C"] > 1:
        assert np.abs(ref[1]["p_model"] - ref[0]["p_model"]).max() > 0 or c["m"] == 1


@pytest.mark.parametrize("c", SC.SOFTMATCH, ids=IDS(SC.SOFTMATCH))
def test_softmatch_cases(c):
    inp = SC.softmatch_inputs(c)
    for x, r in zip(inp["steps"], SC.softmatch_ref(c, inp)):
        _no_near(c["id"], np.abs(x[: c["B"]].astype(F64) - r["mu"]) <= SC.NEAR)
        assert r["weight"].min() > 1e-30 and np.isfinite(r["var"])             # no float32 underflow: the exponent measure stays defined
    if c["m"] == 0 and c["B"] >= 64:                          # the weights span well below 1 and exactly 1
        w = SC.softmatch_ref(c, inp)[0]["weight"]
        assert w.min() < 0.1 and (w == 1.0).any() and ((w > 0.1) & (w < 0.9)).any()


@pytest.mark.parametrize("c", SC.MASKED_CE, ids=IDS(SC.MASKED_CE))
def test_ce_cases(c):
    inp = SC.ce_inputs(c)
    ref = SC.ce_ref(c, inp)
    if c["masks"] and c["B"] > 1:
        assert _mixed(ref["w"] != 0)
    if c["B"] >= 8 and c["C"] >= 3:
        assert ref["loss"] * c["B"] > 100.0                  # the saturated row with its target on a -80 logit is in the mean
    z = torch.from_numpy(inp["z"]).double().requires_grad_(True)
    t = lambda a: None if a is None else torch.from_numpy(a).double()  # noqa: E731
    loss = SC.H.consistency_loss(z, torch.from_numpy(inp["y"]), t(inp["mask"]), t(inp["mask2"]))
    (loss * c["gs"]).backward()
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-12 * max(1.0, ref["loss"]) and np.abs(z.grad.numpy() - ref["dlogits"]).max() <= 1e-14


@pytest.mark.parametrize("c", SC.REWARD, ids=IDS(SC.REWARD))
def test_reward_cases(c):
    inp = SC.reward_inputs(c)
    ref = SC.reward_ref(c, inp)
    _no_near(c["id"], ref["near"])
    valid = ~np.isnan(ref["mask"])
    assert int(valid.sum()) == c["total"] and np.isnan(inp["reward"][c["total"]:]).all() and not np.isnan(inp["reward"][: c["total"]]).any()
    r, Bg = inp["reward"].astype(F64), c["Bg"]
    if c["plant"] == "all_equal":
        assert ref["mask"][valid].all() and all(np.ptp(r[g * Bg:(g + 1) * Bg]) == 0 for g in range(c["groups"]))
    elif c["plant"] == "one_at_mean":
        for g in range(c["groups"]):
            x = r[g * Bg:(g + 1) * Bg]
            assert ref["mean"][g] == 0.5 and (x == 0.5).sum() == 2 and (x < 0.5).any() and ref["mask"][g * Bg:(g + 1) * Bg][x == 0.5].all()
            assert float(np.cumsum(x.astype(F32), dtype=F32)[-1]) == x.sum()      # exact in float32 as well
    elif c["Bg"] >= 3:
        assert _mixed(ref["mask"][valid])


def _docstring_table():
    """{row: (floor, bound)} as written in the module docstring of tests/test_gpu_score_filter_kernels.py"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_score_filter_kernels.py")
    with open(path) as f:
        doc = ast.get_docstring(ast.parse(f.read()))
    rows = re.findall(r"^\s*([a-z_0-9/]+)\s+([0-9.]+e-[0-9]+)\s+([0-9.]+e-[0-9]+)\s", doc, flags=re.M)
    return {k: (float(a), float(b)) for k, a, b in rows}


def test_committed_bounds_are_eight_float32_floors():
    """The committed floors are the float32 evaluation's deviation as measured here, within FLOOR_HEADROOM from both sides; every bound is exactly
    8 times its floor (at least 1e-7); the docstring table of the GPU tests states the same figures."""
    floors = SC.float32_floors()
    table = _docstring_table()
    for k in sorted(floors):
        print("%-15s measured %.3e   floor %.2e   bound %.2e" % (k, floors[k], SC.FLOORS.get(k, float("nan")), SC.BOUNDS.get(k, float("nan"))))
    assert set(floors) == set(SC.FLOORS) == set(SC.BOUNDS) == set(table)
    for k, f in SC.FLOORS.items():
        assert f * (1.0 - SC.FLOOR_HEADROOM) <= floors[k] <= f * (1.0 + SC.FLOOR_HEADROOM), (k, floors[k], f)
        assert SC.BOUNDS[k] == max(8.0 * f, 1e-7), k
        assert table[k] == (float("%.2e" % f), float("%.2e" % SC.BOUNDS[k])), (k, table[k])


# ---- power: the committed bounds reject every wrong version ------------------------------------------------------------------------------------------
def _over(errors):
    return any(not v <= SC.BOUNDS[k] for k, v in errors.items())


def _flips(got, ref, near):
    return bool(((np.asarray(got) != np.asarray(ref)) & ~np.asarray(near)).any())


def _rejected(op, wrong):
    """ids of the committed cases on which the wrong version, put in the kernel's place, would fail the GPU test's comparisons"""
    hit = []
    if op == "stats":
        for c in SC.STATS:
            inp = SC.stats_inputs(c)
            r, w = SC.stats_ref(c, inp), SC.stats_ref(c, inp, wrong)
            if _over(SC.stats_errors(c, w, r)) or not np.array_equal(w["hist"], r["hist"]):
                hit.append(c["id"])
    elif op == "freematch":
        for c in SC.FREEMATCH:
            inp = SC.freematch_inputs(c)
            for r, w in zip(SC.freematch_ref(c, inp), SC.freematch_ref(c, inp, wrong)):
                if _over(SC.freematch_errors(c, w, r)) or _flips(w["mask"], r["mask"], r["near"]):
                    hit.append(c["id"])
                    break
    elif op == "entropy":
        for c in SC.ENTROPY:
            inp = SC.entropy_inputs(c)
            r, w = SC.entropy_ref(c, inp), SC.entropy_ref(c, inp, wrong)
            if c["sel"] != "none" and _over(SC.entropy_errors(w["loss"], w["out"], r)):
                hit.append(c["id"])
    elif op == "distalign":
        for c in SC.DISTALIGN:
            inp = SC.distalign_inputs(c)
            for r, w in zip(SC.distalign_ref(c, inp), SC.distalign_ref(c, inp, wrong)):
                if _over(SC.distalign_errors(c, w, r)) or _flips(w["idx"], r["idx"], SC.argmax_near(r["gap"])):
                    hit.append(c["id"])
                    break
    elif op == "softmatch":
        for c in SC.SOFTMATCH:
            inp = SC.softmatch_inputs(c)
            for r, w in zip(SC.softmatch_ref(c, inp), SC.softmatch_ref(c, inp, wrong)):
                if _over(SC.softmatch_errors(w, r)):
                    hit.append(c["id"])
                    break
    elif op == "ce":
        for c in SC.MASKED_CE:
            inp = SC.ce_inputs(c)
            if _over(SC.ce_errors(c, SC.ce_ref(c, inp, wrong), SC.ce_ref(c, inp))):
                hit.append(c["id"])
    elif op == "reward":
        for c in SC.REWARD:
            inp = SC.reward_inputs(c)
            r, w = SC.reward_ref(c, inp), SC.reward_ref(c, inp, wrong)
            valid = ~np.isnan(r["mask"])
            if _over(SC.reward_errors(w, r)) or _flips(w["mask"][valid], r["mask"][valid], r["near"][valid]):
                hit.append(c["id"])
    return hit


@pytest.mark.parametrize("op,wrong", [(op, w) for op, ws in SC.WRONG.items() for w in ws])
def test_bounds_reject_the_wrong_version(op, wrong):
    hit = _rejected(op, wrong)
    print("%s / %s: rejected on %d cases: %s" % (op, wrong, len(hit), hit[:6]))
    assert hit, (op, wrong)


def test_the_restatements_themselves_pass():
    """the same machinery finds nothing wrong with the right version"""
    for op in SC.WRONG:
        assert _rejected(op, None) == [], op
