"""Opt-in pseudo-label quality monitor (``monitor_pseudo_labels: True``): how good the pseudo labels are that the confidence mask and the
rewarder let through, measured against the true labels of the unlabelled set and accumulated on the device.

One launch per training step (``ops.pl_monitor``, csrc/pl_monitor.hip) adds the step's counts into a device-resident state; the host copies
the state ONCE when somebody reads a log value and derives the metrics from the counts (``PlMonitor.metrics_from_state``).  Nothing of the
step waits for the monitor and the monitor changes nothing the step computes.  The state layout is the contract of include/srhip.h.

The true labels are ``args.ulb_targets`` only: an explicit int array with one entry per unlabelled sample, -1 where unknown (STL-10's extra
split).  The device loaders drop the targets of the unlabelled dataset objects on purpose, as the reference's unlabelled batches carry none.
"""
import numpy as np
import torch

from .. import ops
from .algorithmbase import DeferredScalar

HEADER = ("steps", "rows", "rows_correct", "sel", "sel_correct", "conf_sel", "conf_sel_correct", "rows_unknown", "gen_rows", "gen_correct",
          "reward_bad", "m2", "m2_correct")
LOG_KEYS = ("pl_acc", "select_ratio", "select_acc", "conf_select_acc", "reward_filter_acc", "reward_mean_correct", "reward_mean_wrong",
            "reward_auc")


def _ratio(a, b):
    return float(a) / float(b) if b else float("nan")


class _Window:
    """The metrics of the steps since the previous read, shared by the eight log values of ONE step: the first value anybody reads copies the
    state (and starts the next window), the others take theirs from the same copy."""
    __slots__ = ("monitor", "it", "_m")

    def __init__(self, monitor, it):
        self.monitor, self.it, self._m = monitor, it, None

    def metrics(self):
        if self._m is None:
            self._m = self.monitor._metrics_for_step(self.it)
        return self._m


class MonitorScalar(DeferredScalar):
    """A log value of the monitor: becomes a python float on first use, as DeferredScalar; a step whose log values nobody reads copies
    nothing and does not synchronise."""
    __slots__ = ("_w", "_k")

    def __init__(self, window, key):
        super().__init__(None)
        self._w, self._k = window, key

    def __float__(self):
        if self._v is None:
            self._v = float(self._w.metrics()[self._k])
        return self._v


class PlMonitor:
    """Owns the device copy of the true labels and the monitor's state: an int64 block [16 + 2 C + 64] and four float64 sums, side by side in
    one tensor so that ONE copy brings both to the host."""

    log_keys = LOG_KEYS

    def __init__(self, ulb_targets, num_classes, device, ulb_dest_len=None):
        t = self.check_targets(ulb_targets, ulb_dest_len)
        self.num_classes = int(num_classes)
        self.device = device
        self.targets = torch.from_numpy(t).to(device)
        self.words = ops.pl_monitor_words(self.num_classes)
        self.block = torch.zeros(self.words + ops.PL_SUMS, dtype=torch.int64, device=device)
        self.istate, self.fstate = self.block[:self.words], self.block[self.words:].view(torch.float64)
        self._log_it, self._log_metrics = None, None

    @staticmethod
    def check_targets(ulb_targets, ulb_dest_len=None):
        """The explicit label array as contiguous int64, or a ValueError naming what is wrong with it."""
        if ulb_targets is None:
            raise ValueError("monitor_pseudo_labels: True needs args.ulb_targets: an int array with the true label of every unlabelled sample "
                             "(-1 where unknown); the unlabelled datasets' own targets are not used")
        t = ulb_targets.detach().cpu().numpy() if torch.is_tensor(ulb_targets) else np.asarray(ulb_targets)
        if t.ndim != 1 or t.size == 0 or not np.issubdtype(t.dtype, np.integer):
            raise ValueError("monitor_pseudo_labels: args.ulb_targets must be a non-empty 1-D int array, got shape %s dtype %s" % (t.shape, t.dtype))
        if ulb_dest_len is not None and int(ulb_dest_len) != t.size:
            raise ValueError("monitor_pseudo_labels: args.ulb_targets has %d entries, the unlabelled set (ulb_dest_len) has %d"
                             % (t.size, int(ulb_dest_len)))
        return np.ascontiguousarray(t.astype(np.int64))

    # ---- per step ---------------------------------------------------------------------------------------------------------------------
    def accumulate(self, K, masks, pseudo, reward, mask2, idx_ulb):
        """The one launch of a step: ``masks`` the step's list of K + 1 confidence masks (only the first and the last are read), ``pseudo``
        int64 [(K + 1) * nu], ``reward`` / ``mask2`` fp32 [K * nu] (None when K == 0), ``idx_ulb`` int64 [nu] on the device."""
        if idx_ulb is None:
            raise ValueError("monitor_pseudo_labels needs the batch's idx_ulb (the unlabelled rows' positions in the unlabelled set)")
        nu = int(idx_ulb.numel())
        ops.pl_monitor(pseudo, masks[0], masks[K], mask2 if K > 0 else None, reward if K > 0 else None, idx_ulb, self.targets, K + 1, nu,
                       self.num_classes, self.istate, self.fstate)

    def log_values(self, it):
        """The eight lazy log values of step ``it`` (LOG_KEYS, in that order)."""
        w = _Window(self, it)
        return {k: MonitorScalar(w, k) for k in LOG_KEYS}

    def restart(self):
        """An empty window and no line read yet (a checkpoint was loaded: the window is not part of it, and ``it`` may have stepped back)."""
        self.block.zero_()
        self._log_it, self._log_metrics = None, None

    def _metrics_for_step(self, it):
        """The line of step ``it``: the window up to now on its first read (which starts the next window), the same copy on every later
        read.  A line OLDER than the newest one read (its window went into that one) reads nan and leaves the running window alone."""
        if self._log_it is not None and it < self._log_it:
            return {k: float("nan") for k in LOG_KEYS}
        if self._log_it != it or self._log_metrics is None:
            self._log_metrics = self.read(reset=True)["metrics"]
            self._log_it = it
        return self._log_metrics

    # ---- reading ----------------------------------------------------------------------------------------------------------------------
    def read(self, reset=True):
        """One copy of the state (synchronises the current stream): the raw counts -- per-class arrays and histograms included -- and under
        'metrics' the derived metrics of the window.  reset=True zeroes the window behind the copy."""
        h = self.block.cpu().numpy()
        if reset:
            self.block.zero_()
        st = self.state_from_words(h, self.num_classes)
        st["metrics"] = self.metrics_from_state(st)
        return st

    @staticmethod
    def state_from_words(h, C):
        """The int64 words of the block (integer state, then the four float64 sums bit for bit) as a dict of counts."""
        h = np.ascontiguousarray(np.asarray(h, dtype=np.int64))
        W = ops.pl_monitor_words(C)
        assert h.shape == (W + ops.PL_SUMS,)
        st = {k: int(h[i]) for i, k in enumerate(HEADER)}
        o = ops.PL_HEADER_WORDS
        st["sel_by_class"], st["sel_correct_by_class"] = h[o:o + C].copy(), h[o + C:o + 2 * C].copy()
        st["hist"] = h[o + 2 * C:W].reshape(2, ops.PL_BINS).copy()              # [0]: wrong pseudo labels, [1]: right ones
        f = h[W:].view(np.float64)
        st["sum_w"], st["sum_w_correct"], st["sum_r"] = float(f[0]), float(f[1]), np.array([f[2], f[3]], dtype=np.float64)
        return st

    @staticmethod
    def metrics_from_state(st):
        """The eight metrics from the counts alone; an empty denominator gives nan.
          pl_acc               rows_correct / rows                 accuracy of the kept pass's pseudo labels, selected or not
          select_ratio         sum_w / rows                        share (SoftMatch: mean weight) of the unlabelled rows the loss keeps
          select_acc           sum_w_correct / sum_w               accuracy of the kept rows, weighted as the loss weights them
          conf_select_acc      conf_sel_correct / conf_sel         the confidence mask of pass 0 alone (what util_ratio describes)
          reward_filter_acc    m2_correct / m2                     accuracy of the data_generator rows the reward filter lets through
          reward_mean_correct  sum_r[1] / (rewards binned in hist[1]),   reward_mean_wrong likewise with [0]
          reward_auc           P(a right row's reward lies in a higher bin than a wrong row's) + 0.5 * P(same bin), from the two histograms"""
        hist = np.asarray(st["hist"], dtype=np.int64).reshape(2, -1)
        n0, n1 = int(hist[0].sum()), int(hist[1].sum())
        below, pairs2 = 0, 0                                   # exact integers: twice the (half-)pairs won
        for b in range(hist.shape[1]):
            pairs2 += int(hist[1, b]) * (2 * below + int(hist[0, b]))
            below += int(hist[0, b])
        return {"pl_acc": _ratio(st["rows_correct"], st["rows"]),
                "select_ratio": _ratio(st["sum_w"], st["rows"]),
                "select_acc": _ratio(st["sum_w_correct"], st["sum_w"]),
                "conf_select_acc": _ratio(st["conf_sel_correct"], st["conf_sel"]),
                "reward_filter_acc": _ratio(st["m2_correct"], st["m2"]),
                "reward_mean_correct": _ratio(st["sum_r"][1], n1),
                "reward_mean_wrong": _ratio(st["sum_r"][0], n0),
                "reward_auc": (pairs2 / (2.0 * n0 * n1)) if n0 and n1 else float("nan")}
