"""The 13 kernels of csrc/score_filter.hip one by one, every output element and every state word against the float64 restatements of
tests/_score_filter_cases.py: row softmax / max / argmax (dense and strided), the FreeMatch column statistics, the FreeMatch EMA state and mask,
the fairness loss and its gradient, DistAlign, the SoftMatch state and weight, masked cross-entropy, the reward-mean mask; the fixed mask, the
top-k reward mask and the three FlexMatch kernels through one cross-check each at a new size (257) against a plain numpy statement.  What the
cases exercise, that no row of theirs sits near a threshold, and that the bounds below reject a list of plausible wrong versions is asserted
without a GPU by tests/test_cpu_score_filter_cases.py.  Needs a MI355X.

Bounds.  None is chosen and none comes from a kernel's output.  For every compared quantity a float32 evaluation of the same operation
(oracle/hooks_ref.py in float32 with one thread; a left-to-right float32 numpy sum where the kernel sums left to right) is compared with the
float64 restatement over all committed cases; "floor" is the worst deviation, to three digits, and the kernel's bound is 8 x floor (another,
still float32, reduction order), at least 1e-7.  tests/test_cpu_score_filter_cases.py measures the floors afresh and holds this table and
_score_filter_cases.FLOORS to them within 1 %, from both sides.

    quantity        floor      bound      measure
    rm/probs        1.35e-07   1.08e-06   absolute, every probability of every row
    rm/maxp         1.35e-07   1.08e-06   absolute
    st/colsum       4.05e-08   3.24e-07   largest element error / largest magnitude, divided by sqrt(B) (a left-to-right sum of B terms)
    fm/time_p       6.56e-08   5.25e-07   absolute, the quantile rule
    fm/time_p_mean  7.45e-09   1.00e-07   absolute divided by sqrt(n_all), the mean rule (a left-to-right sum of n_all terms)
    fm/p_model      1.38e-07   1.10e-06   largest element error / largest magnitude of the vector
    fm/label_hist   5.73e-08   4.58e-07   "
    ent/loss        1.44e-07   1.15e-06   |error| / max(|loss|, 1)
    ent/grad        5.21e-07   4.17e-06   largest element error / largest magnitude of dlogits as the kernel leaves it (scales with the gradient)
    da/p_model      1.63e-07   1.30e-06   largest element error / largest magnitude of the vector
    da/p_target     1.19e-07   9.52e-07   "
    da/aligned      2.02e-07   1.62e-06   absolute, every aligned probability
    da/maxp         2.02e-07   1.62e-06   absolute
    sm/mu           5.97e-08   4.78e-07   absolute
    sm/var          6.77e-08   5.42e-07   relative
    sm/weight       5.35e-07   4.28e-06   |error| / (w max(1, -ln w)): through the exponent, whose error the weight carries as a relative one
    ce/loss         3.25e-08   2.60e-07   |error| / max(|loss|, 1), divided by sqrt(B) (a left-to-right sum of B rows)
    ce/dlogits      1.56e-07   1.25e-06   largest element error / largest magnitude of the tensor
    rw/mean         1.42e-07   1.14e-06   absolute

Masks and argmax labels are exact: a row whose float64 distance to its threshold (for an argmax: whose top-two gap) is at most NEAR = 1e-6 may
fall on either side, every other row must match, and the committed cases have no such row; the planted exact ties (FreeMatch at n_all = 1,
equal rewards, a reward at an exactly representable mean, tied logits) have one right answer.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _score_filter_cases as SC            # noqa: E402
from semireward_amd import ops              # noqa: E402

DEV = "cuda:0"
F32, F64 = np.float32, np.float64
SENT = 7.0                                  # what every output buffer holds before the launch
IDS = lambda cs: [c["id"] for c in cs]  # noqa: E731
WORST = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sent(*shape, dtype=torch.float32):
    return torch.full(shape, -77 if dtype == torch.int64 else SENT, dtype=dtype, device=DEV)


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    print("\n    worst deviation per quantity over all cases of this file")
    for k in SC.FLOORS:
        if k in WORST:
            print("    %-15s %.3e   (bound %.2e)   %s" % (k, WORST[k][0], SC.BOUNDS[k], WORST[k][1]))


def check(errors, cid):
    """Print every figure, then hold each against its committed bound."""
    for k, v in errors.items():
        print("    %-28s %-15s %.3e   (bound %.2e)" % (cid, k, v, SC.BOUNDS[k]))
        if k not in WORST or not v <= WORST[k][0]:
            WORST[k] = (v, cid)
    bad = {k: v for k, v in errors.items() if not v <= SC.BOUNDS[k]}           # (not <=: NaN fails)
    assert not bad, (cid, bad)


def where_worst(got, ref):
    idx, e = SC.worst(got, ref)
    return "worst element %s: got %r, want %r" % (tuple(int(i) for i in idx), float(np.asarray(got)[idx]), float(np.asarray(ref)[idx]))


def check_rows(cid, what, got, ref, bound):
    """A [B, C] output row by row under an absolute bound; the message names case, row and column of the worst element."""
    got = np.asarray(got, F64)
    assert np.isfinite(got).all(), (cid, what, "not finite in rows %s" % np.nonzero(~np.isfinite(got).all(axis=1))[0].tolist()[:8])
    e = np.abs(got - ref).max(axis=1)
    assert (e <= bound).all(), "%s %s: %d rows over %.2e; %s" % (cid, what, int((e > bound).sum()), bound, where_worst(got, ref))


def check_labels(cid, what, got, ref, gap):
    bad = SC.check_discrete(what, got, ref, SC.argmax_near(gap))
    assert not bad, (cid, bad)


# ---- 1. row softmax / max / argmax, dense and strided -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SC.ROWS, ids=IDS(SC.ROWS))
def test_row_max(c):
    B, C = c["B"], c["C"]
    inp = SC.row_inputs(c)
    ref = SC.row_ref(c, inp)
    z = dev(inp["z"])
    probs, mp, mi = sent(B + 2, C), sent(B + 3), sent(B + 3, dtype=torch.int64)
    ops.row_max(z, False, probs, mp, mi, B, C)
    p_np = host(probs)
    check_rows(c["id"], "probs", p_np[:B], ref["probs"], SC.BOUNDS["rm/probs"])
    check(SC.row_errors(dict(probs=p_np[:B], maxp=host(mp)[:B]), ref), c["id"])
    check_labels(c["id"], "argmax", host(mi)[:B], ref["idx"], ref["gap"])
    assert np.array_equal(host(mp)[:B], p_np[:B].max(axis=1))                  # the max is an element of the row it wrote
    assert (p_np[B:] == SENT).all() and bool((mp[B:] == SENT).all()) and bool((mi[B:] == -77).all())        # nothing past B is written
    # without probs_out; and rows that are probabilities already: max and first argmax of the float32 rows, exactly
    mp2, mi2 = sent(B), sent(B, dtype=torch.int64)
    ops.row_max(z, False, None, mp2, mi2, B, C)
    assert torch.equal(mp2, mp[:B]) and torch.equal(mi2, mi[:B])
    pin = SC.softmax64(inp["z"]).astype(F32)
    ops.row_max(dev(pin), True, None, mp2, mi2, B, C)
    assert np.array_equal(host(mp2), pin.max(axis=1)) and np.array_equal(host(mi2), pin.argmax(axis=1))
    # strided: groups of rpg rows, `pad` NaN rows between them and around -- the bits of the dense call
    rpg, gr, first = c["rpg"], c["rpg"] + c["pad"], 2
    n_groups = -(-B // rpg)
    base = np.full((first + n_groups * gr + 1, C), np.nan, F32)
    for r in range(B):
        base[first + (r // rpg) * gr + r % rpg] = inp["z"][r]
    probs3, mp3, mi3 = sent(B + 2, C), sent(B + 3), sent(B + 3, dtype=torch.int64)
    ops.row_max_strided(dev(base), first, False, probs3, mp3, mi3, B, C, rpg, gr)
    assert torch.equal(probs3, probs) and torch.equal(mp3, mp) and torch.equal(mi3, mi)


# ---- 2. column sums and predicted-class histogram -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SC.STATS, ids=IDS(SC.STATS))
def test_freematch_stats(c):
    B, C = c["B"], c["C"]
    inp = SC.stats_inputs(c)
    ref = SC.stats_ref(c, inp)
    colsum, hist = sent(C + 3), sent(C + 3)
    ops.freematch_stats(dev(inp["probs"]), dev(inp["idx"]), colsum, hist, B, C)
    check(SC.stats_errors(c, dict(colsum=host(colsum)[:C]), ref), c["id"])
    assert np.array_equal(host(hist)[:C], ref["hist"]), (c["id"], where_worst(host(hist)[:C], ref["hist"]))
    assert bool((colsum[C:] == SENT).all()) and bool((hist[C:] == SENT).all())


# ---- 3. FreeMatch state and mask ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SC.FREEMATCH, ids=IDS(SC.FREEMATCH))
def test_freematch_update(c):
    B, C, n = c["B"], c["C"], c["n_all"]
    inp = SC.freematch_inputs(c)
    ref = SC.freematch_ref(c, inp)
    time_p, p_model, label_hist = dev(inp["time_p"]), dev(np.append(inp["p_model"], F32(SENT))), dev(np.append(inp["label_hist"], F32(SENT)))
    for t, (s, r) in enumerate(zip(inp["steps"], ref)):
        cid = "%s step %d" % (c["id"], t)
        mask = sent(B + 3)
        ops.freematch_update(dev(s["maxp_all"]), n, dev(s["colsum"]), dev(s["hist"]), dev(s["maxp_all"][:B]), dev(s["idx_all"][:B]), time_p,
                             p_model, label_hist, mask, B, C, c["m"], c["uq"], c["clip"])
        got = dict(time_p=float(time_p), p_model=host(p_model)[:C], label_hist=host(label_hist)[:C])
        assert all(np.isfinite(v).all() for v in got.values()), cid
        check(SC.freematch_errors(c, got, r), cid)           # at m == 0 the state IS the batch statistic: compared undamped
        bad = SC.check_discrete("mask", host(mask)[:B], r["mask"], r["near"])
        assert not bad, (cid, bad)
        assert bool((mask[B:] == SENT).all()) and float(p_model[C]) == SENT and float(label_hist[C]) == SENT
    if c["m"] == 0 and not c["clip"] and not c["uq"] and n == 1:
        assert float(time_p) == float(inp["steps"][-1]["maxp_all"][0]) and float(mask[0]) == 1.0       # the exact tie: conf >= conf * 1


# ---- 4. fairness loss and gradient -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SC.ENTROPY, ids=IDS(SC.ENTROPY))
def test_freematch_entropy(c):
    B, C = c["B"], c["C"]
    inp = SC.entropy_inputs(c)
    ref = SC.entropy_ref(c, inp)
    dl = sent(B + 1, C)
    if c["acc"]:
        dl[:B] = dev(inp["d0"])
    loss, ws = sent(1), torch.empty(B * C, device=DEV)
    ops.freematch_entropy(dev(inp["z"]), dev(inp["mask"]), dev(inp["p_model"]), dev(inp["label_hist"]), c["gs"], loss, dl, ws, B, C, accumulate=c["acc"])
    out = host(dl)
    assert (out[B] == SENT).all()                            # nothing past B is written
    unsel = inp["mask"] == 0
    if c["acc"]:
        assert np.array_equal(out[:B][unsel], inp["d0"][unsel])                 # an unselected row is left as it was
    else:
        assert (out[:B][unsel] == 0.0).all()                                    # ... or is exactly 0
    if c["sel"] == "none":
        assert float(loss) == 0.0
        return
    assert np.isfinite(out).all() and np.isfinite(float(loss))
    check(SC.entropy_errors(float(loss), out[:B], ref), c["id"])
    e = np.abs(out[:B].astype(F64) - ref["out"]).max(axis=1)
    lim = SC.BOUNDS["ent/grad"] * (np.abs(ref["out"]).max() or 1.0)
    assert (e <= lim).all(), (c["id"], where_worst(out[:B], ref["out"]))


# ---- 5. DistAlign ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SC.DISTALIGN, ids=IDS(SC.DISTALIGN))
def test_distalign(c):
    B, C = c["B"], c["C"]
    inp = SC.distalign_inputs(c)
    ref = SC.distalign_ref(c, inp)
    p_model, p_target, inited = torch.zeros(C + 1, device=DEV), dev(np.append(inp["p_target"], F32(SENT))), torch.zeros(1, dtype=torch.int32, device=DEV)
    p_model[C] = SENT
    for t, (s, r) in enumerate(zip(inp["steps"], ref)):       # step 0: the first-call form; later steps: the EMA form
        cid = "%s step %d" % (c["id"], t)
        al, mp, mi = sent(B + 1, C), sent(B + 2), sent(B + 2, dtype=torch.int64)
        ops.distalign(dev(s["probs_all"][:B]), dev(s["colsum_ulb"]), c["n_ulb"], dev(s["colsum_lb"]) if c["model"] else None, c["n_lb"], p_model,
                      p_target, inited, c["m"], al, mp, mi, B, C)
        a_np = host(al)
        got = dict(p_model=host(p_model)[:C], p_target=host(p_target)[:C], aligned=a_np[:B], maxp=host(mp)[:B])
        check_rows(cid, "aligned", a_np[:B], r["aligned"], SC.BOUNDS["da/aligned"])
        check(SC.distalign_errors(c, got, r), cid)
        check_labels(cid, "argmax", host(mi)[:B], r["idx"], r["gap"])
        assert np.array_equal(host(mp)[:B], a_np[:B].max(axis=1))
        if not c["model"]:
            assert np.array_equal(got["p_target"], inp["p_target"])             # uniform target: left alone
        assert int(inited) == 1 and float(p_model[C]) == SENT and float(p_target[C]) == SENT
        assert (a_np[B] == SENT).all() and bool((mp[B:] == SENT).all()) and bool((mi[B:] == -77).all())


# ---- 6. SoftMatch ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SC.SOFTMATCH, ids=IDS(SC.SOFTMATCH))
def test_softmatch(c):
    B, n = c["B"], c["n_all"]
    inp = SC.softmatch_inputs(c)
    ref = SC.softmatch_ref(c, inp)
    mu_var = dev(np.append(inp["mu_var"], F32(SENT)))
    for t, (x, r) in enumerate(zip(inp["steps"], ref)):
        cid = "%s step %d" % (c["id"], t)
        w = sent(B + 2)
        ops.softmatch_mask(dev(x), n, dev(x[:B]), mu_var, c["m"], c["ns"], w, B)
        mv = host(mu_var)
        got = dict(mu=mv[0], var=mv[1], weight=host(w)[:B])
        assert np.isfinite(got["weight"]).all() and (got["weight"] <= 1.0).all() and (got["weight"] > 0.0).all(), cid
        check(SC.softmatch_errors(got, r), cid)
        assert (got["weight"][x[:B] >= r["mu"] + SC.NEAR] == 1.0).all(), cid       # rows above mu weigh exactly 1 (none sits within 1e-6 of mu)
        assert mv[2] == SENT and bool((w[B:] == SENT).all())


# ---- 7. masked cross-entropy ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SC.MASKED_CE, ids=IDS(SC.MASKED_CE))
def test_masked_ce(c):
    B, C = c["B"], c["C"]
    inp = SC.ce_inputs(c)
    ref = SC.ce_ref(c, inp)
    opt = lambda a: None if a is None else dev(a)  # noqa: E731
    loss, dl = sent(1), sent(B + 1, C)
    ops.masked_ce(dev(inp["z"]), dev(inp["y"]), opt(inp["mask"]), opt(inp["mask2"]), c["gs"], loss, dl, B, C)
    out = host(dl)
    assert np.isfinite(out).all() and (out[B] == SENT).all()
    check(SC.ce_errors(c, dict(loss=float(loss), dlogits=out[:B]), ref), c["id"])
    e = np.abs(out[:B].astype(F64) - ref["dlogits"]).max(axis=1)
    assert (e <= SC.BOUNDS["ce/dlogits"] * np.abs(ref["dlogits"]).max()).all(), (c["id"], where_worst(out[:B], ref["dlogits"]))
    assert (out[:B][ref["w"] == 0] == 0.0).all()             # an unselected row gets exactly 0
    loss2 = sent(1)
    ops.masked_ce(dev(inp["z"]), dev(inp["y"]), opt(inp["mask"]), opt(inp["mask2"]), c["gs"], loss2, None, B, C)
    assert torch.equal(loss2, loss)                          # the loss alone: the same bits


# ---- 8. reward-mean mask ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SC.REWARD, ids=IDS(SC.REWARD))
def test_reward_mask2(c):
    G, Bg, total = c["groups"], c["Bg"], c["total"]
    inp = SC.reward_inputs(c)
    ref = SC.reward_ref(c, inp)
    mask2, mean_out = sent(G * Bg + 2), sent(G + 1)
    ops.reward_mask2(dev(inp["reward"]), mask2, mean_out, G, Bg, mean_in=dev(inp["mean_in"]) if c["mean_in"] else None,
                     total=total if total != G * Bg else None)
    m_np, mean_np = host(mask2), host(mean_out)
    for g in range(G):
        n = SC.group_rows(c, g)
        sl = slice(g * Bg, g * Bg + n)
        bad = SC.check_discrete("mask2 of group %d" % g, m_np[sl], ref["mask"][sl], ref["near"][sl])
        assert not bad, (c["id"], bad)
        assert (m_np[g * Bg + n: (g + 1) * Bg] == SENT).all()                    # the rows a ragged last group does not hold
    check(SC.reward_errors(dict(mean=mean_np[:G]), ref), c["id"])
    if c["mean_in"]:
        assert np.array_equal(mean_np[:G], inp["mean_in"])                      # the supplied mean, returned as it came
    assert (m_np[G * Bg:] == SENT).all() and mean_np[G] == SENT
    ops.reward_mask2(dev(inp["reward"]), mask2, None, G, Bg, mean_in=dev(inp["mean_in"]) if c["mean_in"] else None,
                     total=total if total != G * Bg else None)
    assert np.array_equal(host(mask2), m_np)                                    # without mean_out: the same mask


# ---- 9. fixed mask, top-k mask and the FlexMatch kernels at a new size, against plain numpy -------------------------------------------------------------
@pytest.mark.parametrize("B", [257, 1025])
def test_fixed_mask_at_new_sizes(B):
    rng = np.random.Generator(np.random.PCG64([19, B]))
    mp = rng.random(B).astype(F32)
    mp[[0, 255, 256, B - 1]] = F32(0.95)                     # rows AT the cutoff are kept, in the first and in the last workgroup
    mask = sent(B + 3)
    ops.fixed_mask(dev(mp), 0.95, mask, B)
    assert np.array_equal(host(mask)[:B], (mp >= F32(0.95)).astype(F32)) and bool((mask[B:] == SENT).all())
    assert 0.0 < host(mask)[:B].mean() < 0.2


def test_reward_topk_at_257_rows():
    """Two groups of 257 rows (a second slice of 256 rows with one row in it), the last group ragged; ties planted across the k-th place."""
    Bg, total, k, k_last = 257, 257 + 130, 100, 50
    rng = np.random.Generator(np.random.PCG64([20, Bg]))
    r = rng.random(2 * Bg).astype(F32)
    tied = [3, 200, 256]
    r[tied] = np.sort(r[:Bg])[Bg - k]                        # three more rows equal to the k-th best: the lower indices go first
    want = np.full(2 * Bg, SENT, F32)
    for g, (n, kk) in enumerate(((Bg, k), (total - Bg, k_last))):
        x = r[g * Bg: g * Bg + n]
        order = np.lexsort((np.arange(n), -x.astype(F64)))   # larger reward first, lower index first among equals
        want[g * Bg: g * Bg + n] = 0.0
        want[g * Bg + order[:kk]] = 1.0
    mask2 = sent(2 * Bg)
    ops.reward_topk_mask(dev(r), mask2, 2, Bg, k, total=total, k_last=k_last)
    assert np.array_equal(host(mask2), want)
    assert int(want[:Bg].sum()) == k and int(want[Bg:total].sum()) == k_last and want[256] == 0.0 and want[3] == 1.0       # the tie straddles the cut


def _flexmatch_numpy(mp, mi, idx, p_cutoff, sel, acc, C, n, warmup):
    """One FlexMatch masking call, stated plainly: the mask BEFORE the update, the table, the histogram with its unused bin, classwise_acc."""
    a = acc[mi]
    mask = (mp >= F32(p_cutoff) * (a / (F32(2.0) - a))).astype(F32)             # float32, op by op
    sel = sel.copy()
    keep = mp >= F32(p_cutoff)
    sel[idx[keep]] = mi[keep]
    cnt, unused = np.bincount(sel[sel >= 0], minlength=C), int((sel < 0).sum())
    acc = acc.copy()
    if max(int(cnt.max()), unused) < n:
        den = max(int(cnt.max()), unused) if warmup else int(cnt.max())
        if den:
            acc = (cnt.astype(F64) / den).astype(F32)
    return mask, sel, np.append(cnt, unused).astype(np.int32), acc


@pytest.mark.parametrize("general", [False, True], ids=["lds", "general"])
@pytest.mark.parametrize("warmup", [True, False])
def test_flexmatch_at_257_classes(monkeypatch, general, warmup):
    """C = 257 (a second stride of every class loop), B = 300 (a second stride of the row loops), three calls on the state the last one left;
    the table's histogram rebuilt at C = 257 first."""
    if general:
        monkeypatch.setenv("SRHIP_FLEXMATCH_GENERAL", "1")
    C, B, n = 257, 300, 700
    rng = np.random.Generator(np.random.PCG64([21, C, B]))
    sel = np.where(rng.random(n) < 0.5, -1, rng.integers(0, C, size=n)).astype(np.int64)
    acc = rng.random(C).astype(F32)
    d_sel, d_hist, d_acc = dev(sel), sent(C + 1, dtype=torch.int32), dev(acc)
    ops.flexmatch_rebuild_hist(d_sel, d_hist, n, C)
    assert np.array_equal(host(d_hist), np.append(np.bincount(sel[sel >= 0], minlength=C), (sel < 0).sum()))
    for t in range(3):
        mp = np.where(rng.random(B) < 0.5, rng.random(B), 0.95 + 0.05 * rng.random(B)).astype(F32)
        mi, idx = rng.integers(0, C, size=B, dtype=np.int64), rng.permutation(n)[:B].astype(np.int64)
        mask_w, sel, hist_w, acc = _flexmatch_numpy(mp, mi, idx, 0.95, sel, acc, C, n, warmup)
        mask = sent(B + 3)
        ops.flexmatch_mask(dev(mp), dev(mi), dev(idx), 0.95, d_sel, d_hist, d_acc, mask, B, C, n, warmup)
        assert np.array_equal(host(mask)[:B], mask_w) and bool((mask[B:] == SENT).all()), t
        assert np.array_equal(host(d_sel), sel) and np.array_equal(host(d_hist), hist_w) and np.array_equal(host(d_acc), acc), t
        assert 0.0 < mask_w.mean() < 1.0
    ops.check_label_errors()


# ---- 10. argument limits: refused, nothing launched ------------------------------------------------------------------------------------------------------
def test_argument_limits_are_refused():
    f = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    i = lambda *s: torch.zeros(*s, dtype=torch.int64, device=DEV)  # noqa: E731
    C, B = 3, 2
    tp, pm, lh, mask = f(1), f(C), f(C), sent(B)
    with pytest.raises(RuntimeError, match="invalid argument"):                # n_all = 1025 > srt[1024]
        ops.freematch_update(f(1025), 1025, f(C), f(C), f(B), i(B), tp, pm, lh, mask, B, C, 0.5, True, False)
    ops.freematch_update(f(1024) + 0.5, 1024, f(C) + 1.0, f(C) + 1.0, f(B) + 0.5, i(B), tp, pm, lh, sent(B), B, C, 0.5, True, False)      # 1024 is fine
    loss, ws = sent(1), f(1025 * 2049)
    with pytest.raises(RuntimeError, match="invalid argument"):                # B = 1025 > pred[1024]
        ops.freematch_entropy(f(1025, C), f(1025), pm, lh, 1.0, loss, sent(1025, C), ws, 1025, C)
    with pytest.raises(RuntimeError, match="invalid argument"):                # C = 2049 > g[2048]
        ops.freematch_entropy(f(B, 2049), f(B), f(2049), f(2049), 1.0, loss, sent(B, 2049), ws, B, 2049)
    mu_var, w = torch.tensor([0.5, 0.1], device=DEV), sent(B)
    with pytest.raises(RuntimeError, match="invalid argument"):                # n_sigma = 0 would divide by zero
        ops.softmatch_mask(f(4), 4, f(B), mu_var, 0.5, 0, w, B)
    with pytest.raises(RuntimeError, match="invalid argument"):                # a group stride shorter than a group's rows
        ops.row_max_strided(f(16, C), 0, False, None, f(8), i(8), 8, C, 4, 3)
    torch.cuda.synchronize()
    assert bool((mask == SENT).all()) and float(loss) == SENT and bool((w == SENT).all())
    assert host(mu_var).tolist() == [0.5, float(F32(0.1))] and float(tp) == 0.25 and float(mask[0]) == SENT
