"""Host reference and cases of the DropPath plan (srhip_vit_droppath_plan): per block, the number of samples whose MLP factor is not 0 and a
stable partition of the samples -- those first, the dropped ones behind them, each group in ascending order.  Pure numpy, no device."""
import numpy as np

KEPT = np.float32(1.0 / 0.85)
BATCHES = (1, 3, 64, 65, 130, 300)          # one sample, a part of a wave, a wave, one past it, past a wave quartet's half, past 256
DEPTHS = (2, 12)
MARGIN = 5                                   # columns in front of a column slice (and 6 behind it)


def plan_ref(dp):
    """dp fp32 [depth, 2, B] -> int32 [depth, 1 + B]."""
    dp = np.asarray(dp)
    depth, _, B = dp.shape
    out = np.empty((depth, 1 + B), dtype=np.int32)
    for l in range(depth):
        keep = dp[l, 1] != 0
        out[l, 0] = int(keep.sum())
        out[l, 1:] = np.argsort(~keep, kind="stable")
    return out


def mlp_keep_pattern(l, B):
    """Which samples keep the MLP branch of block l: nothing dropped, everything dropped, and mixed patterns (factors written, not drawn)."""
    b = np.arange(B)
    kind = l % 6
    if kind == 0:
        return np.ones(B, dtype=bool)
    if kind == 1:
        return np.zeros(B, dtype=bool)
    if kind == 2:
        return (b * 7 + l) % 3 != 0
    if kind == 3:                           # the first and the last sample dropped, and every fifth
        return ~((b == 0) | (b == B - 1) | (b % 5 == 2))
    if kind == 4:                           # only the last sample kept
        return b == B - 1
    return b % 64 != 63                     # the last lane of every wave dropped


def table(depth, B):
    """fp32 [depth, 2, B]: branch 1 from mlp_keep_pattern, branch 0 (attention) its complement -- a plan made from the wrong branch is wrong."""
    t = np.zeros((depth, 2, B), dtype=np.float32)
    for l in range(depth):
        k = mlp_keep_pattern(l, B)
        t[l, 1, k] = KEPT
        t[l, 0, ~k] = KEPT
    return t


def wide_table(depth, B):
    """The same table as columns MARGIN .. MARGIN + B of a wider one whose other columns hold the opposite decisions."""
    t = table(depth, B)
    w = np.zeros((depth, 2, B + 2 * MARGIN + 1), dtype=np.float32)
    w[:, :, :MARGIN] = np.where(t[:, :, :1] != 0, 0, KEPT)
    w[:, :, MARGIN + B:] = np.where(t[:, :, -1:] != 0, 0, KEPT)
    w[:, :, MARGIN:MARGIN + B] = t
    return w


def check_plan(plan, dp):
    """The defining properties, stated without the reference's argsort."""
    dp = np.asarray(dp)
    depth, _, B = dp.shape
    assert plan.shape == (depth, 1 + B) and plan.dtype == np.int32
    for l in range(depth):
        keep = dp[l, 1] != 0
        n = int(plan[l, 0])
        order = plan[l, 1:]
        assert n == int(keep.sum())
        assert sorted(order.tolist()) == list(range(B))
        assert keep[order[:n]].all() and not keep[order[n:]].any()
        assert (np.diff(order[:n]) > 0).all() and (np.diff(order[n:]) > 0).all()
