"""Scoring and exporting pseudo labels for a whole unlabelled set (``AlgorithmBase.score_unlabeled``): which samples the model would
pseudo-label now and with which label, how confident it is, and which of them the Rewarder keeps.

Per batch, after the backbone's inference forward, four kinds of launches and nothing else: ``ops.score_rows`` (label, confidence, margin,
entropy and the algorithm's mask / weight from its threshold state as it stands), the Rewarder's forward in groups of ``reward_group`` rows,
``ops.reward_mask2`` (or the launch of the algorithm's opt-in ``reward_filter``) and ``ops.score_commit`` (the scatter into the table).  No torch indexing op, no allocation after the first batch, no
host synchronisation, and no training state is written: the thresholds, the Rewarder, the DropPath counter and ``it`` are where they were.

``PseudoLabelTable`` owns the columns, one entry per unlabelled sample:
  label int64 (-1: never scored), conf, margin, entropy, weight, reward fp32, reward_keep uint8 (the reward filter ``reward >= mean`` of the
  row's group), selected uint8 (weight > 0 and reward_keep), count int32 (how often the entry was written; > 1 shows a repeat).
"""
import copy
import json

import numpy as np
import torch

from .. import ops

COLUMNS = tuple(k for k, _ in ops.TABLE_COLUMNS)
_NP = dict(label=np.int64, conf=np.float32, margin=np.float32, entropy=np.float32, weight=np.float32, reward=np.float32,
           reward_keep=np.uint8, selected=np.uint8, count=np.int32)
# the device block: columns in decreasing element size, so that every column starts aligned to its own size
_ORDER = ("label", "conf", "margin", "entropy", "weight", "reward", "count", "reward_keep", "selected")
_EMPTY_META = dict(algorithm=None, it=0, mode=None, p_cutoff=None, reward_group=None, state={})


class PseudoLabelTable:
    """The columns of ``n`` unlabelled samples: on a device (one byte block, so that ``read()`` is ONE copy) while a pass fills them, or on
    the host (``load``, ``from_arrays``).  ``meta``: algorithm key, ``it``, mode, ``p_cutoff``, ``reward_group`` and a copy of the threshold
    state the weights were computed from."""

    def __init__(self, n, device=None, num_classes=None, meta=None):
        self.n, self.num_classes = int(n), num_classes
        self.meta = dict(_EMPTY_META, **(meta or {}))
        self.device = None if device is None else torch.device(device)
        self._host = None
        if self.device is None:
            self._host = {k: np.zeros(self.n, _NP[k]) for k in COLUMNS}
            self._host["label"][:] = -1
            return
        sizes = [np.dtype(_NP[k]).itemsize * self.n for k in _ORDER]
        self.block = torch.zeros(sum(sizes), dtype=torch.uint8, device=self.device)
        self.columns, off = {}, 0
        for k, sz in zip(_ORDER, sizes):
            self.columns[k] = self.block[off:off + sz].view(dict(ops.TABLE_COLUMNS)[k])
            off += sz
        self.columns["label"].fill_(-1)

    # ---- reading ------------------------------------------------------------------------------------------------------------------
    def read(self):
        """The columns as numpy arrays: one device-to-host copy (which synchronises), then views of it."""
        if self._host is not None:
            return self._host
        h = self.block.cpu().numpy()
        ops.check_label_errors()                     # an index outside the table: skipped by the scatter, raised here
        out, off = {}, 0
        for k in _ORDER:
            sz = np.dtype(_NP[k]).itemsize * self.n
            out[k] = h[off:off + sz].view(_NP[k])
            off += sz
        return {k: out[k] for k in COLUMNS}

    def summary(self, ulb_targets=None):
        """rows scored, selected ratio, per-class selected counts (``num_classes`` bins, or up to the largest label); with ``ulb_targets``
        (one true label per sample, -1 = unknown, as the pseudo-label monitor takes them) the accuracy of all scored rows, of the rows the
        threshold keeps (weight > 0) and of the selected rows, over the rows whose label is known (nan where there is none)."""
        c = self.read()
        scored = c["count"] > 0
        sel = scored & (c["selected"] > 0)
        nc = int(self.num_classes) if self.num_classes else int(max(c["label"].max(initial=-1) + 1, 1))
        lab = c["label"]
        inb = (lab >= 0) & (lab < nc)
        out = {"rows": int(scored.sum()), "selected": int(sel.sum()),
               "selected_ratio": float(sel.sum()) / float(scored.sum()) if scored.any() else float("nan"),
               "selected_by_class": np.bincount(lab[sel & inb], minlength=nc).astype(np.int64),
               "repeats": int((c["count"] > 1).sum())}
        if ulb_targets is not None:
            t = ulb_targets.detach().cpu().numpy() if torch.is_tensor(ulb_targets) else np.asarray(ulb_targets)
            if t.shape != (self.n,):
                raise ValueError("ulb_targets must hold one label per table entry (%d), got shape %s" % (self.n, t.shape))
            known = scored & (t >= 0)
            ok = lab == t
            acc = lambda m: float((ok & m).sum()) / float(m.sum()) if m.any() else float("nan")   # noqa: E731
            out.update(acc_all=acc(known), acc_threshold_kept=acc(known & (c["weight"] > 0)), acc_selected=acc(known & sel),
                       rows_known=int(known.sum()))
        return out

    # ---- files --------------------------------------------------------------------------------------------------------------------
    def save(self, path):
        """An ``.npz``: the columns, ``meta`` (a JSON string) and the threshold state's arrays under ``state/<name>``."""
        c = self.read()
        meta = {k: v for k, v in self.meta.items() if k != "state"}
        meta.update(n=self.n, num_classes=self.num_classes)
        arrays = {k: np.ascontiguousarray(c[k]) for k in COLUMNS}
        arrays["meta"] = np.array(json.dumps(meta))
        for k, v in (self.meta.get("state") or {}).items():
            arrays["state/" + k] = np.asarray(v)
        with open(path, "wb") as f:
            np.savez(f, **arrays)
        return path

    @classmethod
    def from_arrays(cls, columns, num_classes=None, meta=None):
        n = int(np.asarray(columns["label"]).shape[0])
        t = cls(n, None, num_classes, meta)
        for k in COLUMNS:
            a = np.asarray(columns[k])
            if a.shape != (n,):
                raise ValueError("column %r must hold %d entries, got shape %s" % (k, n, a.shape))
            t._host[k] = np.ascontiguousarray(a.astype(_NP[k]))
        return t

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            meta = json.loads(str(z["meta"]))
            meta["state"] = {k[len("state/"):]: z[k] for k in z.files if k.startswith("state/")}
            n, nc = meta.pop("n"), meta.pop("num_classes")
            t = cls.from_arrays({k: z[k] for k in COLUMNS}, nc, meta)
        assert t.n == n
        return t


# ---- the pass over a loader ---------------------------------------------------------------------------------------------------------
def score_rule(alg):
    """(mode, keyword arguments of ops.score_rows, {name: device tensor} of the threshold state) for the algorithm's MaskingHook -- read only."""
    from ..algorithms.hooks import (FixedThresholdingHook, FlexMatchThresholdingHook, FreeMatchThresholdingHook, SoftMatchWeightingHook)
    h = alg.hooks_dict["MaskingHook"]
    if isinstance(h, FixedThresholdingHook):
        return "fixed", dict(p_cutoff=float(alg.p_cutoff)), {}
    if isinstance(h, FlexMatchThresholdingHook):
        return "flex", dict(p_cutoff=float(alg.p_cutoff), classwise_acc=h.classwise_acc), dict(classwise_acc=h.classwise_acc)
    if isinstance(h, FreeMatchThresholdingHook):
        return "free", dict(time_p=h.time_p, p_model=h.p_model), dict(time_p=h.time_p, p_model=h.p_model)
    if isinstance(h, SoftMatchWeightingHook):
        kw, st = dict(mu_var=h.mu_var, n_sigma=int(h.n_sigma)), dict(mu_var=h.mu_var)
        da = alg.hooks_dict.get("DistAlignHook")
        if da is not None:               # the step weights the rows by the max of the ALIGNED probabilities (srsoftmatch.py:137-140)
            kw.update(da_p_model=da.p_model, da_p_target=da.p_target, da_inited=da.inited)
            st.update(da_p_model=da.p_model, da_p_target=da.p_target, da_inited=da.inited)
        return "soft", kw, st
    raise NotImplementedError("score_unlabeled: no scoring rule for the masking hook %s" % type(h).__name__)


def unlabelled_eval_loader(alg, batch_size):
    """The device mode's own evaluation loader over ``dataset_dict['train_ulb']``: the unaugmented evaluation view, in index order."""
    ds = (alg.dataset_dict or {}).get("train_ulb")
    if ds is None:
        raise ValueError("score_unlabeled(loader=None): dataset_dict['train_ulb'] is missing")
    view = copy.copy(ds)                 # the evaluation loaders want labels beside the rows; the unlabelled store has none: -1 (unknown), unused here
    if view.targets is None:
        view.targets = torch.full((len(ds),), -1, dtype=torch.int64, device=ds.device)
    return alg.input_mode.eval_loader(alg.args, view, batch_size, alg.print_fn)


def _batch_rows(alg, data):
    """(backbone input on the device, idx_ulb or None) of an eval-style ({'x_lb'}) or train-style ({'x_ulb_w', 'idx_ulb'}) batch."""
    if "x_ulb_w" in data:
        x, idx = data["x_ulb_w"], data.get("idx_ulb")
    elif "x_lb" in data:
        x, idx = data["x_lb"], data.get("idx_ulb")
    else:
        raise ValueError("score_unlabeled: a batch needs 'x_lb' (evaluation style) or 'x_ulb_w' (training style), got keys %s" % sorted(data))
    if isinstance(x, dict):                                              # usb_nlp: {'input_ids', 'attention_mask'}
        from ..nets.bert import TokenBatch
        x = TokenBatch.from_dict(x, alg.device)
    elif hasattr(x, "key_len"):                                          # a TokenBatch of the device token loaders
        x = x.to(alg.device, non_blocking=True)
    else:
        x = x.to(alg.device, non_blocking=True).contiguous()
    if idx is not None:
        idx = idx.to(alg.device, non_blocking=True).long().contiguous()
    return x, idx


class _Scratch:
    """The dense per-batch buffers, allocated once for the largest batch a pass has seen (the first one, for every loader that keeps only its
    last batch partial)."""

    def __init__(self, rows, device):
        self.rows = rows
        self.cols = {k: torch.empty(rows, dtype=dt, device=device) for k, dt in ops.SCORE_COLUMNS}
        self.reward = torch.empty(rows, dtype=torch.float32, device=device)
        self.keep = torch.empty(rows, dtype=torch.float32, device=device)


def score_loader(alg, net, loader, n, reward_group):
    """The pass: every batch of ``loader`` through ``net``'s inference forward and the four kinds of launches into a new table of ``n`` entries."""
    mode, kw, state = score_rule(alg)
    rw = alg.rewarder
    F, L = rw.feature_dim, rw.label_dim
    meta = dict(algorithm=alg.algorithm, it=int(alg.it), mode=mode, p_cutoff=kw.get("p_cutoff"), reward_group=int(reward_group),
                state={k: v.detach().cpu().numpy().copy() for k, v in state.items()})
    rf = alg.reward_filter
    meta.update(rf.meta(int(reward_group)))
    table = PseudoLabelTable(n, alg.device, alg.num_classes, meta)
    scratch, seen, g = None, 0, int(reward_group)
    with ops.stream_scope():
        for data in loader:
            x, idx = _batch_rows(alg, data)
            lg, feat, _ = net.forward_features(alg._bucket_tokens(x, net), None, None, save=False)
            B = int(lg.shape[0])
            if scratch is None or scratch.rows < B:
                scratch = _Scratch(B, alg.device)
            ops.score_rows(lg, mode, scratch.cols, **kw)
            if feat.dtype != torch.float32 or not feat.is_contiguous():
                feat = feat.float().contiguous()
            # rewards in groups of g rows, the batch's last group with the rows that are left: the Rewarder's attention is a softmax over
            # its group (semireward.py:60-62), so a reward is what training would see only at the training group size
            G, r = divmod(B, g)
            if G:
                ops.rewarder_fwd(rw.flat, rw.flat_t, feat, scratch.cols["label"], scratch.reward, rw._workspace(G, g), G, g, F, L)
            if r:
                ops.rewarder_fwd(rw.flat, rw.flat_t, ops.RawRows(feat, G * g * F), ops.RawRows(scratch.cols["label"], G * g),
                                 ops.RawRows(scratch.reward, G * g), rw._workspace(1, r), 1, r, F, L)
            rf.apply(scratch.reward, scratch.keep, G + (1 if r else 0), g, total=B)       # the algorithm's reward filter (mean: ops.reward_mask2)
            ops.score_commit(scratch.cols, scratch.reward, scratch.keep, table.columns, B, idx=idx, row_offset=seen)
            seen += B
    return table
