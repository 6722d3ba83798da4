"""srhip_score_rows / srhip_score_commit (csrc/score_rows.hip) over the case table of tests/_score_rows_cases.py:
  label, conf    bit-equal to ops.row_max on a dense copy of the rows (aligned SOFT mode: to ops.distalign with momentum 1 on a state copy)
  weight         bit-equal to the hook's own masking launch with momentum 1 on a state copy, which leaves the state where it is
  against the float64 restatement: weight (rows within 1e-6 of their threshold excepted, at most 2 % of a case), margin within
                 2 (C + 8) 2^-24, entropy within 2 (C + 8) 2^-24 (1 + ln C) -- the sequential-sum, 2-ulp-expf and 1-ulp-division bounds
  commit         the scatter exact, untouched entries bit-preserved, count over two overlapping launches, the out-of-range row skipped and
                 reported through ops.check_label_errors()
  two launches on equal inputs give equal bits; sentinels behind every output survive.
Largest errors seen on one MI355X: profiles/score_unlabeled.txt."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _score_rows_cases as SC                 # noqa: E402
from semireward_amd import ops                # noqa: E402

DEV = "cuda:0"
SPECS = SC.case_table()
_CASES = {}
TAIL = 3                                       # sentinel entries behind every dense output column


def case_and_ref(spec):
    """A case and its restatement, computed once and shared (read-only)."""
    if spec not in _CASES:
        case = SC.make_case(*spec)
        _CASES[spec] = (case, SC.restate_rows(case))
    return _CASES[spec]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def logits_view(case):
    """The rows where the case put them: pitch ld, base ``off`` elements past an aligned allocation, NaN around every row."""
    buf = dev(case["buf"])
    v = torch.as_strided(buf, (case["B"], case["C"]), (case["ld"], 1), case["off"])
    assert v.data_ptr() % 16 == (4 * case["off"]) % 16
    return buf, v


def state_tensors(case):
    return {k: dev(v) for k, v in case["state"].items() if isinstance(v, np.ndarray)}


def fresh_out(B):
    out = {}
    for k, dt in ops.SCORE_COLUMNS:
        out[k] = torch.full((B + TAIL,), -7, dtype=dt, device=DEV)
    return out


def score(case, view, st, out):
    mode = "soft" if case["mode"].startswith("soft") else case["mode"]
    ops.score_rows(view, mode, out, p_cutoff=case["state"]["p_cutoff"], classwise_acc=st.get("classwise_acc"), time_p=st.get("time_p"),
                   p_model=st.get("p_model"), mu_var=st.get("mu_var"), n_sigma=case["state"]["n_sigma"], da_p_model=st.get("da_p_model"),
                   da_p_target=st.get("da_p_target"), da_inited=st.get("da_inited"))


def host(out, B):
    h = {k: v.cpu().numpy() for k, v in out.items()}
    for k, v in h.items():
        assert (v[B:] == -7).all(), "%s: written behind row B" % k
    return {k: v[:B] for k, v in h.items()}


@pytest.mark.parametrize("spec", SPECS, ids=SC.case_id)
def test_columns(spec):
    case, ref = case_and_ref(spec)
    B = case["B"]
    buf, view = logits_view(case)
    st = state_tensors(case)
    st0 = {k: v.clone() for k, v in st.items()}
    out = fresh_out(B)
    score(case, view, st, out)
    got = host(out, B)
    assert buf.cpu().numpy().tobytes() == case["buf"].tobytes()                       # the rows and the NaN around them are only read
    for k in st:
        assert torch.equal(st[k], st0[k]), "state %s was written" % k
    mode = "soft" if case["mode"].startswith("soft") else case["mode"]
    mp, mi, w = SC.training_launches(dev(case["logits"]), mode, st, case["state"]["p_cutoff"], case["state"]["n_sigma"])
    assert got["label"].tobytes() == mi.cpu().numpy().tobytes(), "label differs from the training launches"
    assert got["conf"].tobytes() == mp.cpu().numpy().tobytes(), "conf differs from the training launches"
    assert got["weight"].tobytes() == w.cpu().numpy().tobytes(), "weight differs from the hook's launch"
    print("score_rows %s max errors: %s" % (SC.case_id(spec), SC.max_errors(ref, got)))
    assert SC.check_rows(case, ref, got) == []
    again = fresh_out(B)
    score(case, view, st, again)
    for k, v in host(again, B).items():
        assert v.tobytes() == got[k].tobytes(), "%s: two launches on equal inputs differ" % k


def drain_flags():
    try:
        ops.check_label_errors()
    except IndexError:
        pass


def table_to_dev(t):
    return {k: dev(v) for k, v in t.items()}


@pytest.mark.parametrize("spec", list(dict.fromkeys(SPECS[::3] + [s for s in SPECS if s[5] == "oob"][:3])), ids=SC.case_id)
def test_commit(spec):
    case, _ = case_and_ref(spec)
    B, n = case["B"], case["n"]
    drain_flags()
    _, view = logits_view(case)
    out = fresh_out(B)
    score(case, view, state_tensors(case), out)
    cols = host(out, B)
    before = SC.sentinel_table(n)
    tab = table_to_dev(before)
    reward, keep, idx = dev(case["reward"]), dev(case["keep"]), dev(case["idx"])
    ops.score_commit(out, reward, keep, tab, B, idx=idx, row_offset=case["row_offset"])
    want, flag = SC.restate_commit(case, cols, before)
    got = {k: v.cpu().numpy() for k, v in tab.items()}
    assert SC.tables_differ(got, want) == []                                           # the scatter exact, every other entry's bits kept
    if flag:
        with pytest.raises(IndexError, match="pseudo-label table"):
            ops.check_label_errors()
    ops.check_label_errors()                                                           # ... and the read reset the word
    # a second, overlapping launch: the same rows in arrival order from entry 1 on -- the later launch wins, count shows the repeats
    second = dict(case, idx=None, row_offset=1)
    ops.score_commit(out, reward, keep, tab, B, idx=None, row_offset=1)
    want2, flag2 = SC.restate_commit(second, cols, want)
    assert not flag2
    got2 = {k: v.cpu().numpy() for k, v in tab.items()}
    assert SC.tables_differ(got2, want2) == []
    assert (got2["count"] - before["count"]).sum() == 2 * B - int(flag) and (got2["count"] - before["count"]).max() <= 2
    ops.check_label_errors()


def test_ragged_reward_groups_take_their_own_mean():
    """ops.reward_mask2(total=...): whole groups as the plain launch gives them, the last group's mean over the rows that are left."""
    rng = np.random.Generator(np.random.PCG64(5))
    for total, g in ((40, 7), (5, 8), (130, 64), (200, 70), (24, 8)):
        r = rng.random(total).astype(np.float32)
        rd, m = dev(r), torch.full((total + 2,), -7.0, device=DEV)
        G = -(-total // g)
        ops.reward_mask2(rd, m, None, G, g, total=total)
        want = torch.full((total + 2,), -7.0, device=DEV)
        if total // g:
            ops.reward_mask2(rd, want, None, total // g, g)
        if total % g:
            ops.reward_mask2(rd[total // g * g:].clone(), want[total // g * g:], None, 1, total % g)
        assert torch.equal(m, want), (total, g)
        if g <= 64:                                                                    # left-to-right fp32 mean (score_filter.hip)
            for k in range(G):
                seg = r[k * g:(k + 1) * g]
                s = np.float32(0)
                for v in seg:
                    s = np.float32(s + v)
                assert np.array_equal(m[k * g:k * g + seg.size].cpu().numpy(), (seg >= np.float32(s / np.float32(seg.size))).astype(np.float32))
