"""srhip_score_rows / srhip_score_commit without a GPU: the float64 restatement of tests/_score_rows_cases.py against torch's CPU softmax /
argmax and the oracle's hook formulas, the checker against planted faults, every SR_EINVAL refusal, PseudoLabelTable on host arrays, and
the near-threshold condition of the case table."""
import os

import numpy as np
import pytest
import torch

import _score_rows_cases as SC
from oracle import hooks_ref as H

F32 = np.float32
SPECS = SC.case_table()
_CASES = {}


def case_and_ref(spec):
    """A case and its restatement, computed once and shared (read-only)."""
    if spec not in _CASES:
        case = SC.make_case(*spec)
        _CASES[spec] = (case, SC.restate_rows(case))
    return _CASES[spec]


def test_case_table_covers_what_it_claims():
    assert {s[0] for s in SPECS} == set(SC.CS) and {s[1] for s in SPECS} == set(SC.BS) and {s[2] for s in SPECS} == set(SC.MODES)
    assert {s[3] for s in SPECS} == {0, 3} and {s[4] for s in SPECS} == {0, 1} and {s[5] for s in SPECS} == set(SC.IDX_KINDS)
    for mode in SC.MODES:                             # every mode on both sides of the register / re-read switch
        assert {s[0] for s in SPECS if s[2] == mode} >= {SC.REG_COLS, SC.REG_COLS + 1}, mode
    planted = set()
    for s in SPECS:
        case, _ = case_and_ref(s)
        planted |= set(case["planted"])
        row_cols = np.zeros(case["buf"].size, bool)
        for b in range(case["B"]):
            row_cols[case["off"] + b * case["ld"]: case["off"] + b * case["ld"] + case["C"]] = True
        assert np.isnan(case["buf"][~row_cols]).all() and not np.isnan(case["buf"][row_cols]).any()      # NaN sentinels around every row
    assert planted == {"tie_first_last", "tie_three", "tie_second", "onehot_pos", "onehot_neg", "all_equal"}


@pytest.mark.parametrize("spec", SPECS, ids=SC.case_id)
def test_restatement_agrees_with_torch_and_the_oracle_hooks(spec):
    case, ref = case_and_ref(spec)
    B, C, st, mode = case["B"], case["C"], case["state"], case["mode"]
    probs = torch.softmax(torch.from_numpy(case["logits"]), dim=-1)
    if mode == "soft_da1":                            # hooks/dist_align.py with momentum 1: the state stays, the rows are aligned
        da = H.DistAlignState(C, momentum=1.0)
        da.p_model, da.p_target = torch.from_numpy(st["da_p_model"].copy()), torch.from_numpy(st["da_p_target"].copy())
        probs = da.dist_align(probs)
        assert np.array_equal(da.p_model.numpy(), st["da_p_model"])
    p = probs.numpy()
    sure = (ref["margin"] == 0.0) | (ref["margin"] > SC.NEAR)
    assert np.array_equal(probs.argmax(dim=-1).numpy()[sure], ref["label"][sure])
    np.testing.assert_allclose(p.max(axis=1), ref["conf"], rtol=0, atol=SC.margin_bound(C))
    assert np.isfinite(ref["entropy"]).all() and (ref["entropy"] >= 0).all() and (ref["entropy"] <= np.log(C) + 1e-12).all()
    t = torch.from_numpy(p.astype(np.float64))
    np.testing.assert_allclose(ref["entropy"], torch.special.entr(t).sum(dim=-1).numpy(), rtol=0, atol=SC.entropy_bound(C))
    if C > 1:
        top2 = torch.topk(probs, 2, dim=-1).values.numpy()
        np.testing.assert_allclose(ref["margin"], top2[:, 0].astype(np.float64) - top2[:, 1], rtol=0, atol=SC.margin_bound(C))
    else:
        assert np.array_equal(ref["margin"], ref["conf"])
    # the oracle's hook formulas on the same probabilities, state frozen by momentum 1
    pc = st["p_cutoff"]
    if mode == "fixed":
        w = H.fixed_threshold_mask(p, pc)
    elif mode == "flex":
        fm = H.FlexMatchState(4 * B, C)
        fm.classwise_acc = st["classwise_acc"].copy()
        w = fm.masking(p, np.arange(B), pc)            # the mask is taken before the update (srflexmatch/utils.py:53)
    elif mode == "free":
        fr = H.FreeMatchState(C, momentum=1.0, use_quantile=False)
        fr.p_model, fr.time_p = torch.from_numpy(st["p_model"].copy()), torch.tensor(float(st["time_p"][0]))
        w = fr.masking(probs).numpy()
        assert np.array_equal(fr.p_model.numpy(), st["p_model"])
    else:
        if B < 2:
            return                                    # torch.var of one value is nan: the oracle's update cannot be frozen
        sm = H.SoftMatchState(C, n_sigma=st["n_sigma"], momentum=1.0)
        sm.mu, sm.var = torch.tensor(float(st["mu_var"][0])), torch.tensor(float(st["mu_var"][1]))
        w = sm.masking(probs).numpy()
        np.testing.assert_allclose(w, ref["weight"], rtol=0, atol=ref["soft_tol"])
        return
    keep = ~ref["near"] & sure
    assert np.array_equal(np.asarray(w, np.float64)[keep], ref["weight"][keep])


@pytest.mark.parametrize("spec", SPECS, ids=SC.case_id)
def test_near_threshold_rows_are_rare(spec):
    """The exclusion the GPU test may use, on the float64 restatement alone: at most 2 % of a case's rows within 1e-6 of their threshold."""
    case, ref = case_and_ref(spec)
    assert ref["near"].sum() <= SC.NEAR_SHARE * case["B"], (int(ref["near"].sum()), case["B"])


# ---- the checker against planted faults ---------------------------------------------------------------------------------------------
def emulate(case, fault=None):
    """The five columns in fp32 numpy, the way a correct kernel forms them -- or with one fault planted."""
    z, st, mode, C = case["logits"], case["state"], case["mode"], case["C"]
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = (e / e.sum(axis=1, keepdims=True)).astype(F32)
    if "da_inited" in st and int(st["da_inited"][0]) != 0:
        q = (p * (st["da_p_target"] + F32(1e-6)) / (st["da_p_model"] + F32(1e-6))).astype(F32)
        p = q if fault == "not_renormalised" else (q / q.sum(axis=1, keepdims=True)).astype(F32)
    label = p.argmax(axis=1)
    if fault == "last_index":
        label = C - 1 - p[:, ::-1].argmax(axis=1)
    conf = p.max(axis=1)
    src = z if fault == "margin_from_logits" else p
    second = np.sort(src, axis=1)[:, -2] if C > 1 else np.zeros(len(p), F32)
    margin = (src.max(axis=1) - second).astype(F32) if C > 1 else conf
    with np.errstate(divide="ignore", invalid="ignore"):
        plogp = p * np.log(p) if fault == "zero_log_zero" else np.where(p > 0, p * np.log(np.where(p > 0, p, 1)), 0)
    entropy = (-plogp.sum(axis=1)).astype(F32)
    pc = F32(st["p_cutoff"])
    if mode == "fixed":
        w = conf >= pc
    elif mode == "flex":
        acc = st["classwise_acc"][label]
        w = conf >= (pc * acc if fault == "flex_no_division" else pc * (acc / (F32(2) - acc)))
    elif mode == "free":
        w = conf >= st["time_p"][0] * (st["p_model"][label] / st["p_model"].max())
    else:
        den = F32(2) * st["mu_var"][1] / F32(st["n_sigma"] ** 2)
        w = np.exp(-(np.minimum(conf - st["mu_var"][0], F32(0)) ** 2) / den)
    return dict(label=label.astype(np.int64), conf=conf, margin=margin, entropy=entropy, weight=np.asarray(w, F32))


@pytest.mark.parametrize("spec", SPECS, ids=SC.case_id)
def test_checker_accepts_a_correct_fp32_implementation(spec):
    case, ref = case_and_ref(spec)
    assert SC.check_rows(case, ref, emulate(case)) == []


FAULTS = {"last_index": (100, 8, "fixed", 0, 0, "perm"), "margin_from_logits": (10, 17, "fixed", 0, 0, "perm"),
          "zero_log_zero": (10, 8, "free", 3, 1, "perm"), "flex_no_division": (10, 65, "flex", 0, 0, "perm"),
          "not_renormalised": (100, 17, "soft_da1", 3, 1, "perm")}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_checker_rejects_planted_faults(fault):
    case = SC.make_case(*FAULTS[fault])
    ref = SC.restate_rows(case)
    assert SC.check_rows(case, ref, emulate(case)) == []
    assert SC.check_rows(case, ref, emulate(case, fault)) != [], fault


def test_checker_rejects_a_commit_that_ignores_idx():
    case = SC.make_case(10, 8, "fixed", 0, 0, "perm")
    cols = emulate(case)
    before = SC.sentinel_table(case["n"])
    want, flag = SC.restate_commit(case, cols, before)
    assert not flag and SC.tables_differ(want, want) == []
    untouched = np.setdiff1d(np.arange(case["n"]), case["idx"])
    for k in SC.TABLE:                                # entries no row goes to keep their bits, NaN sentinels included
        assert want[k][untouched].tobytes() == before[k][untouched].tobytes(), k
    wrong, _ = SC.restate_commit(dict(case, idx=None, row_offset=0), cols, before)       # rows in arrival order instead
    assert SC.tables_differ(wrong, want) != []
    oob = SC.make_case(10, 8, "fixed", 0, 0, "oob")
    t, flag = SC.restate_commit(oob, emulate(oob), SC.sentinel_table(oob["n"]))
    assert flag and int((t["count"] - SC.sentinel_table(oob["n"])["count"]).sum()) == oob["B"] - 1


# ---- argument refusals --------------------------------------------------------------------------------------------------------------
def test_every_invalid_argument_is_refused_before_a_launch():
    from semireward_amd import _lib
    lib = _lib.lib()
    a, E = 0x10000, -1                                # an aligned host address that is never dereferenced; SR_EINVAL

    def rows(**kw):
        d = dict(logits=a, ld=10, B=4, C=10, mode=_lib.SCORE_FIXED, pc=0.9, acc=None, tp=None, pm=None, mv=None, ns=0, dpm=None, dpt=None,
                 di=None, label=a, conf=a, margin=a, entropy=a, weight=a)
        d.update(kw)
        return lib.srhip_score_rows(d["logits"], d["ld"], d["B"], d["C"], d["mode"], d["pc"], d["acc"], d["tp"], d["pm"], d["mv"], d["ns"],
                                    d["dpm"], d["dpt"], d["di"], d["label"], d["conf"], d["margin"], d["entropy"], d["weight"], None)

    for k in ("logits", "label", "conf", "margin", "entropy", "weight"):
        assert rows(**{k: None}) == E, k
    for kw in (dict(B=0), dict(B=65536), dict(C=0), dict(ld=9), dict(mode=4), dict(mode=-1), dict(label=a + 4),
               dict(mode=_lib.SCORE_FLEX), dict(mode=_lib.SCORE_FREE), dict(mode=_lib.SCORE_FREE, tp=a), dict(mode=_lib.SCORE_FREE, pm=a),
               dict(mode=_lib.SCORE_SOFT, ns=2), dict(mode=_lib.SCORE_SOFT, mv=a, ns=0),
               dict(mode=_lib.SCORE_SOFT, mv=a, ns=2, dpm=a), dict(mode=_lib.SCORE_SOFT, mv=a, ns=2, dpm=a, dpt=a),
               dict(mode=_lib.SCORE_SOFT, mv=a, ns=2, di=a)):
        assert rows(**kw) == E, kw

    names = ("label", "conf", "margin", "entropy", "weight", "reward", "keep", "idx", "row_offset", "B", "n", "t_label", "t_conf", "t_margin",
             "t_entropy", "t_weight", "t_reward", "t_keep", "t_selected", "t_count")

    def commit(**kw):
        d = {k: a for k in names}
        d.update(row_offset=0, B=4, n=16)
        d.update(kw)
        return lib.srhip_score_commit(*[d[k] for k in names], None)

    for k in names:
        if k not in ("idx", "row_offset", "B", "n"):
            assert commit(**{k: None}) == E, k
    for kw in (dict(B=0), dict(B=65536), dict(n=0), dict(idx=None, row_offset=-1), dict(label=a + 4), dict(t_label=a + 4), dict(idx=a + 4)):
        assert commit(**kw) == E, kw
    assert lib.srhip_reward_mask2_ragged(None, a, None, 8, 4, None) == E and lib.srhip_reward_mask2_ragged(a, a, None, 0, 4, None) == E
    assert lib.srhip_reward_mask2_ragged(a, a, None, 8, 0, None) == E


def test_binding_matches_the_header():
    import re
    from semireward_amd import _lib, ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "srhip.h")).read(),
                 flags=re.S)
    for n in ("srhip_score_rows", "srhip_score_commit", "srhip_reward_mask2_ragged"):
        assert len(_lib.SIGNATURES[n][1]) == len(re.search(r"\b%s\s*\(([^)]*)\)" % n, src).group(1).split(",")), n
    assert [int(re.search(r"#define SRHIP_SCORE_%s (\d+)" % m.upper(), src).group(1)) for m in ("fixed", "flex", "free", "soft")] == \
        [ops.SCORE_MODES[m] for m in ("fixed", "flex", "free", "soft")]
    assert ops._SCORE_ERR_BIT == 6 and "table" in ops._SCORE_ERR


# ---- PseudoLabelTable on host arrays ------------------------------------------------------------------------------------------------
def host_table():
    from semireward_amd.core.pl_table import PseudoLabelTable
    cols = dict(label=np.array([2, 0, -1, 1, 2, 2], np.int64), conf=np.array([.9, .8, 0, .7, .6, .95], F32),
                margin=np.array([.8, .7, 0, .5, .3, .9], F32), entropy=np.array([.1, .2, 0, .3, .4, .05], F32),
                weight=np.array([1, 1, 0, 0, 1, 1], F32), reward=np.array([.9, .2, 0, .8, .7, .1], F32),
                reward_keep=np.array([1, 0, 0, 1, 1, 0], np.uint8), selected=np.array([1, 0, 0, 0, 1, 0], np.uint8),
                count=np.array([1, 1, 0, 2, 1, 1], np.int32))
    meta = dict(algorithm="srflexmatch", it=7, mode="flex", p_cutoff=0.95, reward_group=4, state=dict(classwise_acc=np.array([.1, .2, .3], F32)))
    return PseudoLabelTable.from_arrays(cols, 3, meta), cols, meta


def test_table_summary_on_host_arrays():
    t, cols, _ = host_table()
    s = t.summary()
    assert s["rows"] == 5 and s["selected"] == 2 and s["selected_ratio"] == 2 / 5 and s["repeats"] == 1
    assert s["selected_by_class"].tolist() == [0, 0, 2]
    s = t.summary(np.array([2, 1, 0, 1, 0, -1]))     # known and scored: rows 0, 1, 3, 4
    assert s["rows_known"] == 4 and s["acc_all"] == 2 / 4 and s["acc_threshold_kept"] == 1 / 3 and s["acc_selected"] == 1 / 2
    with pytest.raises(ValueError):
        t.summary(np.zeros(5, np.int64))


def test_table_save_load_round_trip(tmp_path):
    from semireward_amd.core.pl_table import COLUMNS, PseudoLabelTable
    t, cols, meta = host_table()
    path = t.save(str(tmp_path / "pl.npz"))
    u = PseudoLabelTable.load(path)
    got = u.read()
    for k in COLUMNS:
        assert got[k].dtype == cols[k].dtype and got[k].tobytes() == cols[k].tobytes(), k
    assert u.n == 6 and u.num_classes == 3
    assert {k: u.meta[k] for k in ("algorithm", "it", "mode", "p_cutoff", "reward_group")} == {k: meta[k] for k in ("algorithm", "it", "mode", "p_cutoff", "reward_group")}
    assert np.array_equal(u.meta["state"]["classwise_acc"], meta["state"]["classwise_acc"])
    with np.load(path, allow_pickle=False) as z:     # plain arrays: readable without this package
        assert set(COLUMNS) <= set(z.files)


def test_score_unlabeled_is_part_of_the_public_surface():
    from semireward_amd.core.algorithmbase import AlgorithmBase
    from inspect import signature
    assert list(signature(AlgorithmBase.score_unlabeled).parameters) == ["self", "loader", "use_ema_model", "batch_size", "reward_group"]
