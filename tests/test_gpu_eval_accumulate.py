"""srhip_eval_accumulate (csrc/eval.hip) against a float64 restatement in numpy: predictions, confusion counts and row counters exactly, the
fp64 loss accumulator within the tree's fp32-vs-float64 bound; ties and NaNs as numpy.argmax, ignore_index rows, accumulation over batches,
run-to-run bits, the label-range flag and the argument checks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from semireward_amd import _lib, ops          # noqa: E402

DEV = "cuda:0"
F64_BOUND = 2e-6          # fp32 row arithmetic against float64, relative: the bound of tests/test_gpu_criterions.py


def restate64(z, y):
    """(pred, confusion [C + 1, C], loss_sum, nll_sum, rows, kept) of ONE batch: z fp32 [B, C], y int64 [B] in [-1, C)."""
    B, C = z.shape
    pred = np.argmax(z, axis=1)
    cm = np.zeros((C + 1, C), dtype=np.int64)
    np.add.at(cm, (np.where(y < 0, C, y), pred), 1)
    z64 = z.astype(np.float64)
    mx = np.where(np.isnan(z64), -np.inf, z64).max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        lse = mx[:, 0] + np.log(np.exp(z64 - mx).sum(axis=1))
    keep = y >= 0
    nll = float((lse[keep] - z64[keep, y[keep]]).sum())
    return pred, cm, nll / max(int(keep.sum()), 1) * B, nll, B, int(keep.sum())


def place(z, layout):
    """z on the device as a dense tensor, as the leading columns of a wider buffer (row stride C + 3), or as a view one float past an aligned base."""
    B, C = z.shape
    t = torch.from_numpy(z)
    if layout == "dense":
        return t.to(DEV)
    if layout == "ld+3":
        buf = torch.full((B, C + 3), float("nan"), device=DEV)
        buf[:, :C] = t.to(DEV)
        return buf[:, :C]
    buf = torch.zeros(B * C + 1, device=DEV)
    buf[1:] = t.to(DEV).reshape(-1)
    v = buf[1:].view(B, C)
    assert v.data_ptr() % 16 == 4
    return v


def accumulate(batches, C, want_pred=True, layout="dense"):
    """Runs the batches [(z, y), ...] into one accumulator: (pred, confusion, loss_sum, nll_sum, rows, kept, raw block bytes)."""
    block, state, confusion = ops.eval_accumulator(C, DEV)
    n = sum(z.shape[0] for z, _ in batches)
    pred = torch.full((n,), -7, dtype=torch.int64, device=DEV) if want_pred else None
    off = 0
    for z, y in batches:
        ops.eval_accumulate(place(z, layout), torch.from_numpy(y).to(DEV), confusion, state, pred, off)
        off += z.shape[0]
    cm, loss_sum, nll_sum, rows, kept = ops.eval_accumulator_read(block, C)
    return (pred.cpu().numpy() if want_pred else None), cm, loss_sum, nll_sum, rows, kept, block.cpu().numpy().tobytes()


def data(B, C, seed=0):
    rng = np.random.Generator(np.random.PCG64(1000 * B + C + seed))
    return (3.0 * rng.standard_normal((B, C))).astype(np.float32), rng.integers(0, C, size=B)


def check(got, want, what=""):
    pred, cm, loss_sum, nll_sum, rows, kept, _ = got
    wpred, wcm, wloss, wnll, wrows, wkept = want
    if pred is not None:
        assert np.array_equal(pred, wpred), what
    assert cm.dtype == np.int32 and np.array_equal(cm, wcm), what
    assert (rows, kept) == (wrows, wkept), what
    print("eval_accumulate %s: loss_sum %.9g (float64 %.9g, rel %.2e), nll_sum rel %.2e" % (
        what, loss_sum, wloss, abs(loss_sum - wloss) / max(abs(wloss), 1e-300), abs(nll_sum - wnll) / max(abs(wnll), 1e-300)))
    assert abs(loss_sum - wloss) <= F64_BOUND * abs(wloss), (what, loss_sum, wloss)
    assert abs(nll_sum - wnll) <= F64_BOUND * abs(wnll), (what, nll_sum, wnll)


SHAPES = [(1, 2, "dense"), (7, 10, "dense"), (64, 100, "dense"), (65, 100, "dense"), (300, 257, "dense"), (5, 1024, "dense"), (5, 1025, "dense"),
          (3, 1500, "dense"), (16, 100, "ld+3"), (16, 100, "offset1"), (65535, 7, "dense")]


@pytest.mark.parametrize("B,C,layout", SHAPES, ids=["%dx%d_%s" % s for s in SHAPES])
def test_shapes_against_float64(B, C, layout):
    z, y = data(B, C)
    if B == 1:
        # one row, two classes: the loss of the likelier class is log(1 + e^-d), which fp32 rounds at eps32 ABSOLUTE (1 + e^-d is formed first) --
        # no relative bound can hold for it.  The label is the other class: loss = d + log(1 + e^-d), O(1).
        y = np.argmin(z, axis=1)
    check(accumulate([(z, y)], C, layout=layout), restate64(z, y), "%dx%d %s" % (B, C, layout))
    if B == 1:
        # ... and the likelier class against that absolute bound: the kernel forms s = 1 + e^-d (half an ulp of s: eps32 / 2), takes logf (an
        # ulp of the result) and subtracts (z_y - max) = 0 exactly: |error| <= eps32, with eps32 = 2^-23
        y = np.argmax(z, axis=1)
        pred, cm, loss_sum, nll_sum, rows, kept, _ = accumulate([(z, y)], C, layout=layout)
        w = restate64(z, y)
        print("eval_accumulate 1x2 likelier class: loss %.9g (float64 %.9g, abs %.2e)" % (loss_sum, w[2], abs(loss_sum - w[2])))
        assert np.array_equal(pred, w[0]) and np.array_equal(cm, w[1]) and (rows, kept) == (1, 1)
        assert abs(loss_sum - w[2]) <= 2.0 ** -23 and abs(nll_sum - w[3]) <= 2.0 ** -23
    ops.check_label_errors()


def test_aligned_and_unaligned_rows_give_the_same_bits():
    z, y = data(16, 100)
    a, b, c = (accumulate([(z, y)], 100, layout=k) for k in ("dense", "offset1", "ld+3"))
    assert a[6] == b[6] == c[6] and np.array_equal(a[0], b[0])
    z, y = data(3, 1500)
    assert accumulate([(z, y)], 1500, layout="dense")[6] == accumulate([(z, y)], 1500, layout="offset1")[6]


def test_ties_and_nans_follow_numpy_argmax():
    z, y = data(8, 12, seed=1)
    z[0, 3] = z[0, 9] = 50.0                                # equal maxima: the first
    z[1, 9] = z[1, 3] = z[1, 11] = 50.0
    z[2, 5] = np.nan                                        # a NaN is maximal
    z[3, 7] = z[3, 2] = np.nan                              # the first NaN
    z[4, 0] = np.inf
    z[4, 6] = np.nan                                        # NaN beats +inf
    z[5, :] = -np.inf                                       # all equal: column 0
    z[6, :] = 0.0
    z[6, 4] = -0.0                                          # -0.0 == 0.0: column 0
    want = np.argmax(z, axis=1)
    assert list(want[:7]) == [3, 3, 5, 2, 6, 0, 0]
    y[:] = -1                                               # (the loss of a NaN row is NaN: these rows stay out of it)
    pred, cm, loss_sum, _, rows, kept, _ = accumulate([(z, y)], 12)
    assert np.array_equal(pred, want) and np.array_equal(pred, torch.from_numpy(z).argmax(dim=1).numpy())
    assert np.array_equal(cm[12], np.bincount(want, minlength=12)) and not cm[:12].any() and (rows, kept, loss_sum) == (8, 0, 0.0)
    # long rows (re-read path), ties and NaNs in different 256-column chunks and lanes
    z, y = data(4, 1500, seed=2)
    z[0, 1400] = z[0, 300] = z[0, 1023] = 60.0
    z[1, 1499] = z[1, 1025] = np.nan
    z[2, 257] = np.nan
    z[2, 256] = 90.0
    assert np.array_equal(accumulate([(z, np.full(4, -1))], 1500)[0], np.argmax(z, axis=1))
    # a NaN row that is kept makes the loss NaN, as the reference's; its prediction and count are still exact
    z, y = data(5, 10, seed=3)
    z[2, 4] = np.nan
    pred, cm, loss_sum, _, rows, kept, _ = accumulate([(z, y)], 10)
    assert np.array_equal(pred, np.argmax(z, axis=1)) and cm[y[2], 4] >= 1 and np.isnan(loss_sum) and np.isnan(restate64(z, y)[2])


def test_ignored_rows_land_in_row_C_and_stay_out_of_the_loss():
    z, y = data(33, 10, seed=4)
    y[::4] = -1
    got = accumulate([(z, y)], 10)
    check(got, restate64(z, y), "ignored")
    assert got[1][10].sum() == 9 and got[5] == 33 - 9
    # the loss is the mean over the KEPT rows times B: the kept rows alone, as a batch of their own, give the same mean
    alone = restate64(z[y >= 0], y[y >= 0])
    assert abs(got[2] / 33 - alone[2] / 24) <= F64_BOUND * abs(alone[2] / 24)
    # a batch of ignored rows only contributes 0 to the loss and B rows to row C
    pred, cm, loss_sum, nll_sum, rows, kept, _ = accumulate([(z, np.full(33, -1))], 10)
    assert (loss_sum, nll_sum, rows, kept) == (0.0, 0.0, 33, 0) and cm[10].sum() == 33 and not cm[:10].any()
    assert np.array_equal(pred, np.argmax(z, axis=1))


def test_batches_accumulate_and_two_runs_give_the_same_bits():
    z, y = data(10, 10, seed=5)
    y[7] = -1
    parts = [(z[:4], y[:4]), (z[4:8], y[4:8]), (z[8:], y[8:])]
    got = accumulate(parts, 10)
    per = [restate64(a, b) for a, b in parts]
    want = (np.argmax(z, axis=1), restate64(z, y)[1], sum(p[2] for p in per), sum(p[3] for p in per), 10, 9)
    check(got, want, "4 + 4 + 2")
    assert np.array_equal(got[1], sum(p[1] for p in per))
    again = accumulate(parts, 10)
    assert got[6] == again[6] and np.array_equal(got[0], again[0])
    assert accumulate(parts, 10, want_pred=False)[6] == got[6]              # pred_out is optional
    zb, yb = data(300, 257, seed=6)
    assert accumulate([(zb, yb)] * 3, 257)[6] == accumulate([(zb, yb)] * 3, 257)[6]


@pytest.mark.parametrize("bad", [10, -2, 1 << 40, -(1 << 40)])
def test_label_out_of_range_raises_and_touches_no_accumulator(bad):
    ops.check_label_errors()
    z, y = data(6, 10, seed=7)
    y[:] = bad
    block, state, confusion = ops.eval_accumulator(10, DEV)
    ops.eval_accumulate(torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV), confusion, state)
    with pytest.raises(IndexError, match="evaluation label"):
        ops.check_label_errors()
    ops.check_label_errors()                                                # reset by the failed check
    assert not block.cpu().numpy().any()
    # one bad row among good ones: the others are counted, the bad one nowhere
    z, y = data(6, 10, seed=8)
    good = y.copy()
    y[3] = bad
    pred, cm, loss_sum, nll_sum, rows, kept, _ = accumulate([(z, y)], 10)
    with pytest.raises(IndexError):
        ops.check_label_errors()
    keep = np.arange(6) != 3
    w = restate64(z[keep], good[keep])
    assert np.array_equal(cm, w[1]) and (rows, kept) == (5, 5) and abs(nll_sum - w[3]) <= F64_BOUND * abs(w[3])
    assert np.array_equal(pred, np.argmax(z, axis=1))


def test_invalid_arguments_return_the_error_code_without_a_launch():
    f = _lib.lib().srhip_eval_accumulate
    B, C = 4, 10
    z = torch.zeros(B, C, device=DEV)
    y = torch.zeros(B, dtype=torch.int64, device=DEV)
    block, state, confusion = ops.eval_accumulator(C, DEV)
    s = torch.cuda.current_stream().cuda_stream
    ok = dict(z=z.data_ptr(), ld=C, y=y.data_ptr(), cm=confusion.data_ptr(), st=state.data_ptr(), pred=None, off=0, B=B, C=C)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["z"], a["ld"], a["y"], a["cm"], a["st"], a["pred"], a["off"], a["B"], a["C"], s)
    for kw in (dict(ld=C - 1), dict(B=0), dict(B=65536), dict(C=0), dict(cm=None), dict(st=None), dict(z=None), dict(y=None), dict(off=-1),
               dict(st=state.data_ptr() + 4)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert not block.cpu().numpy().any()
    assert call() == 0
    assert ops.eval_accumulator_read(block, C)[3:] == (B, B)
