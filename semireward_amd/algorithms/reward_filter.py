"""The reward filter ``mask2`` of the SemiReward steps: which unlabelled rows of a pass the Rewarder keeps.

The reference has one rule, ``mask2 = reward >= reward.mean()`` per pass (srflexmatch.py:100-101), which keeps about half of every pass's rows
whatever the Rewarder says.  Two opt-in rules make the filter's selectivity a setting (yaml keys, read with ``getattr(args, ..., None)``; none
of them is a ``get_argument()`` entry):

    reward_filter: mean | topk | fixed      (absent = mean: the reference's rule, the same launches bit for bit)
    reward_topk: k                          topk: keep the k best rows of every pass (int >= 1)            -- exactly one of these two
    reward_keep_ratio: r                    topk: k = ceil(r * rows of the group), 0 < r <= 1, r resolved to 1e-6 in integer arithmetic
    reward_threshold: t                     fixed: mask2 = reward >= t (finite float)

topk orders the rows of a group: non-NaN before NaN, larger reward first (-0 == +0), lower row index first among equal rewards, and keeps
the first min(k, non-NaN rows); a NaN reward is never kept (``srhip_reward_topk_mask``, one launch for all groups).  fixed is
``srhip_reward_mask2`` with its threshold input filled with t.  Everything else of the step -- the loss launch and its mean over all rows,
which pass's mask2 enters the loss, the Rewarder updates -- stays as it is.

Data parallel: per rank, as the mean rule under the reference's DDP.  With ``global_reward_threshold: True`` topk keeps the best k * world
rows (ratio: ceil(r * rows * world)) of ALL ranks' rows of the pass (``DataParallel.gather_rewards``: one all-gather per step); fixed needs
no collective.
"""
import math

import torch

from .. import ops

FILTERS = ("mean", "topk", "fixed")
MAX_CANDIDATES = 65536            # rows of a group times the ranks that share it (srhip_reward_topk_mask)
_PPM = 1000000
_OWNER = (("reward_topk", "topk"), ("reward_keep_ratio", "topk"), ("reward_threshold", "fixed"))


class RewardFilter:
    """The parsed rule (``kind``; ``topk`` or ``ratio_ppm``; ``threshold``) and its dispatch ``apply``."""

    def __init__(self, kind="mean", topk=None, ratio_ppm=None, threshold=None):
        self.kind, self.topk, self.ratio_ppm, self.threshold = kind, topk, ratio_ppm, threshold
        self._thr = {}                  # fixed: device -> fp32 tensor filled with the threshold (one entry per group of a launch)

    def k_for(self, rows, world=1):
        """Rows kept of a group of ``rows`` rows per rank, ranked over ``world`` ranks' rows."""
        if self.topk is not None:
            return self.topk * world
        return max(1, (self.ratio_ppm * rows * world + _PPM - 1) // _PPM)

    def meta(self, rows):
        """What a scored table records about the rule (``rows``: its reward group)."""
        m = dict(reward_filter=self.kind)
        if self.kind == "topk":
            m["k"] = int(self.k_for(rows))
            if self.ratio_ppm is not None:
                m["reward_keep_ratio"] = self.ratio_ppm / _PPM
        elif self.kind == "fixed":
            m["reward_threshold"] = float(self.threshold)
        return m

    def _threshold_rows(self, device, n):
        t = self._thr.get(device)
        if t is None or t.numel() < n:
            t = self._thr[device] = torch.full((max(64, n),), float(self.threshold), dtype=torch.float32, device=device)
        return t

    def apply(self, reward, mask2, groups, B, total=None, mean_in=None, peers=None, self_peer=0):
        """mask2 of ``groups`` groups of ``B`` rows (``total`` rows in all: the last group holds the rows that are left).
        mean_in: the mean rule's external thresholds [groups]; peers [n_peers, groups * B]: topk over all ranks' rows of a group."""
        total = groups * B if total is None else total
        if self.kind == "mean":
            ops.reward_mask2(reward, mask2, None, groups, B, mean_in=mean_in, total=total)
        elif self.kind == "topk":
            world = 1 if peers is None else int(peers.shape[0])
            if B * world > MAX_CANDIDATES or groups * B >= 2 ** 31:
                raise ValueError("reward_filter: topk ranks at most %d rows per group (rows of a pass times the ranks that share it), got %d x %d"
                                 % (MAX_CANDIDATES, B, world))
            ops.reward_topk_mask(reward, mask2, groups, B, self.k_for(B, world), total=total,
                                 k_last=self.k_for(total - (groups - 1) * B, world), peers=peers, self_peer=self_peer)
        else:
            # srhip_reward_mask2 with the threshold in place of the mean: the whole groups in the plain launch, the rows that are left in one more
            G, r = divmod(total, B)
            thr = self._threshold_rows(reward.device, max(G, 1))
            if G:
                ops.reward_mask2(reward, mask2, None, G, B, mean_in=thr)
            if r:
                ops.reward_mask2(ops.RawRows(reward, G * B), ops.RawRows(mask2, G * B), None, 1, r, mean_in=thr)


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def read_reward_filter(args):
    """The rule of ``args`` (see the module docstring).  A ValueError that names the key, before any device work: an unknown filter, topk
    without or with both of reward_topk / reward_keep_ratio, fixed without reward_threshold, a key of another filter, a value out of range."""
    v = getattr(args, "reward_filter", None)
    kind = "mean" if v is None else str(v).strip().lower()
    if kind not in FILTERS:
        raise ValueError("reward_filter must be one of %s, got %r" % (", ".join(FILTERS), v))
    given = {k: getattr(args, k, None) for k, _ in _OWNER}
    for key, owner in _OWNER:
        if given[key] is not None and owner != kind:
            raise ValueError("%s belongs to reward_filter: %s, not to reward_filter: %s" % (key, owner, kind))
    if kind == "mean":
        return RewardFilter()
    if kind == "fixed":
        t = given["reward_threshold"]
        if t is None:
            raise ValueError("reward_filter: fixed needs reward_threshold")
        if not _number(t) or not math.isfinite(t):
            raise ValueError("reward_threshold must be a finite number, got %r" % (t,))
        return RewardFilter("fixed", threshold=float(t))
    k, ratio = given["reward_topk"], given["reward_keep_ratio"]
    if (k is None) == (ratio is None):
        raise ValueError("reward_filter: topk needs exactly one of reward_topk and reward_keep_ratio, got %s" % ("both" if k is not None else "neither"))
    if k is not None:
        if not isinstance(k, int) or isinstance(k, bool) or k < 1 or k >= 2 ** 31 // MAX_CANDIDATES:
            raise ValueError("reward_topk must be an integer >= 1 (and below %d), got %r" % (2 ** 31 // MAX_CANDIDATES, k))
        return RewardFilter("topk", topk=int(k))
    if not _number(ratio) or not math.isfinite(ratio) or not 0 < ratio <= 1:
        raise ValueError("reward_keep_ratio must lie in (0, 1], got %r" % (ratio,))
    ppm = int(round(ratio * _PPM))
    if ppm < 1:
        raise ValueError("reward_keep_ratio is resolved to 1e-6: %r rounds to 0" % (ratio,))
    return RewardFilter("topk", ratio_ppm=ppm)
