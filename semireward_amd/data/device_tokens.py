"""Device-resident token store and loaders of the usb_nlp configurations (``device_tokens: True``): every sentence and every augmented variant
is tokenised ONCE and lives in HBM in one flat int32 array, the reference's sampler decides which sentences form a batch, and a view of a
batch -- gather, right-pad with [PAD] to the batch's longest row, int64 ids, the lengths -- is one srhip_token_view launch
(csrc/token_view.hip).  No tokenizer in the step, no worker processes, no per-step host-to-device copy, no srhip_mask_lengths launch: the
loaders hand ``nets.bert.TokenBatch`` objects to the step.

Restates
  semilearn/datasets/nlp_datasets/datasetbase.py:43-81     which keys a labelled / unlabelled sample carries; 'text_s' is one of the two variants
  semilearn/datasets/collactors/nlp_collactor.py:49-61     tokenizer(text, max_length=max_length, truncation=True, padding=False)['input_ids']
  semilearn/datasets/collactors/nlp_collactor.py:63-110    tokenizer.pad(padding=True): every view right-padded to ITS OWN batch's longest row
  semilearn/datasets/samplers/sampler.py:55-73             the epoch's index stream (EpochSampler of data/device_loader.py, unchanged)
One deviation, documented in configs/README.md: the reference picks the strong variant with an unseeded ``random.randint(1, 2)`` in every
worker process; here the pick comes from a numpy generator seeded with (seed, rank, loader role, epoch), so the draws cannot be matched.  The
sampler stream, the tokenisation and the padding are matched exactly (tests/golden/device_tokens.npz).

``device_tokens_strong: True`` makes the strong view on the device from the clean sentence instead of reading a stored variant: two
token-level slots (delete / mask / cutoff / swap) drawn per sample and epoch, one srhip_token_strong launch (csrc/token_strong.hip).  That
chain is the engine's own, not the reference's back-translation; tests/_token_strong_cases.py restates it exactly."""
import os

import numpy as np
import torch

from .. import ops
from .device_loader import ROLES, EpochSampler             # noqa: F401  (re-exported beside the loaders they feed)
from .modes import active_mode, build_loaders
from .ragged import RaggedEvalLoader, RaggedStore, RaggedTrainLoader, _h2d, with_variants

HUB_NAMES = {"bert_base_uncased": "bert-base-uncased", "bert_base_cased": "bert-base-cased"}     # the reference's collators (nlp_collactor.py:113-122)
TOKENIZER_FILES = ("tokenizer.json", "vocab.txt")
DATA_S_HELP = ("give the unlabelled set the augmented variants of every sentence as {'data': [...], 'data_s': [[variant 0 of every sentence], "
               "[variant 1 ...]]} (the reference's (ori, aug_0, aug_1) triples: its back-translations)")


def _rows(data, what, tokenize, max_length):
    """A list of strings / 1-D integer arrays -> list of contiguous int32 arrays, each refusal with its reason."""
    out = []
    for i, s in enumerate(data):
        if isinstance(s, str):
            if tokenize is None:
                raise ValueError("device_tokens: row %d of %s is a string and no tokenizer was given (pass tokenize=, or already-tokenised "
                                 "1-D integer arrays)" % (i, what))
            s = np.asarray(tokenize(str(s)), dtype=np.int64)                # truncated to max_length by the tokenizer, [SEP] kept last
        else:
            s = s.detach().cpu().numpy() if torch.is_tensor(s) else np.asarray(s)
            if s.dtype.kind not in "iu":
                raise ValueError("device_tokens needs strings or already-tokenised integer arrays, got dtype %s for row %d of %s" % (s.dtype, i, what))
        if s.ndim != 1:
            raise ValueError("device_tokens needs 1-D token rows, got shape %s for row %d of %s" % (s.shape, i, what))
        if s.size == 0:
            raise ValueError("device_tokens: row %d of %s is empty (a tokenised sentence holds at least [CLS] [SEP])" % (i, what))
        if max_length is not None and s.size > max_length:
            raise ValueError("device_tokens: row %d of %s holds %d tokens, more than max_length = %d; the store does not truncate silently "
                             "(truncate as the tokenizer does: keep [SEP] last)" % (i, what, s.size, max_length))
        if s.min() < 0 or s.max() > np.iinfo(np.int32).max:
            raise ValueError("device_tokens: row %d of %s holds a negative token id (or one past int32)" % (i, what))
        out.append(np.ascontiguousarray(s, dtype=np.int32))
    return out


def _is_text(x):
    return isinstance(x, str) or (isinstance(x, np.ndarray) and x.ndim == 0 and x.dtype.kind in "US")


def _triples(data):
    """The reference's (ori, aug_0, aug_1) string triples -> (sentences, [every aug_0, every aug_1]) as lists of str; None when ``data`` is
    something else.  The evaluation sets keep the list of tuples json_data.py builds; the training sets went through split_ssl_data
    (semilearn/datasets/utils.py:38-52: ``np.array(data)[idx]``) and are [n, 3] string arrays, whose rows are 1-D arrays of 3 strings."""
    rows = list(data)
    if not rows or not all(isinstance(t, (tuple, list, np.ndarray)) and not isinstance(t, str) and np.ndim(t) == 1 and len(t) == 3
                           and all(_is_text(x) for x in t) for t in rows):
        return None
    return [str(t[0]) for t in rows], [[str(t[1 + v]) for t in rows] for v in range(2)]


class DeviceTokenDataset(RaggedStore):
    """Token rows of any length in one flat int32 device array ``store``; row r occupies store[row_off[r] : row_off[r] + row_len[r]] and
    starts at a multiple of 4 ints (the gap holds ``pad_id``).  Rows 0 .. n - 1 are the sentences; with ``data_s`` (V lists of n variants)
    row n (1 + v) + i is variant v of sentence i (``strong_row``).  int64 targets resident too (None: unlabelled).  ``row_len_host`` /
    ``row_off_host`` / ``targets_host`` keep numpy copies for the host side of a loader; ``max_id_host`` is the largest stored id, checked
    against the model's vocabulary before anything is launched.  ``data`` items: strings (tokenised once, here, by ``tokenize``) or
    already-tokenised 1-D integer arrays (refused when longer than ``max_length``)."""
    pad_id = 0                                         # [PAD] of both reference vocabularies, BertConfig.pad_id

    def __init__(self, data, targets, device, data_s=None, max_length=None, tokenize=None):
        self.max_length = None if max_length is None else int(max_length)
        rows, n, n_variants = with_variants(lambda d, what: _rows(d, what, tokenize, self.max_length), data, data_s,
                                            "device_tokens", "sentence", DATA_S_HELP)
        self.max_id_host = int(max(int(r.max()) for r in rows))
        super().__init__(rows, n, n_variants, targets, device, self.pad_id, "sentence")

    @classmethod
    def from_reference(cls, dset, device, tokenize=None, max_length=None):
        """A reference nlp ``BasicDataset`` (``.data``: (ori, aug_0, aug_1) string triples -- a list of tuples, or the [n, 3] string array
        split_ssl_data leaves in the training sets --, ``.targets``, ``.is_ulb``) or a plain
        {'data': [...], 'targets': ..., 'data_s': [[...], [...]]} dict of strings / token arrays.  Evaluation sets carry the literal 'None'
        as both augmentations (json_data.py:42): such variants are not stored."""
        if isinstance(dset, cls):
            return dset
        data, targets, data_s = cls.reference_fields(dset)
        tri = None if isinstance(dset, dict) else _triples(data)
        if tri is not None:
            data, var = tri
            data_s = None if all(x == "None" for v in var for x in v) else var
        return cls(data, targets, device, data_s, max_length, tokenize)


def _view(ds, src_row, L):
    from ..nets.bert import TokenBatch
    return TokenBatch(*ops.token_view(ds.store, ds.row_off, ds.row_len, src_row, L, ds.pad_id))


STRONG_KEY = "device_tokens_strong"
STRONG_RATE_KEY, MASK_ID_KEY = "device_tokens_strong_rate", "device_tokens_mask_id"
STRONG_RATE = 0.3                 # a design default, not a measurement: the upper end of the 0.1 .. 0.3 token-level augmentation papers use
MASK_ID = 103                     # [MASK] of both reference vocabularies (bert-base-uncased / bert-base-cased)


def draw_token_slots(rng, n0, rate):
    """The strong view's draws for rows of ``n0`` tokens from ``rng``, whole-epoch vectors in this order: op [2, N] = rng.integers(1, 5)
    (delete, mask, cutoff, swap; uniform, with replacement), u [2, N] = rng.random(), seed [2, N] = rng.integers(0, 2^32).  The counts are
    c = floor(u * rate * ni) slot by slot, with the interior ni = max(0, n - 2) that slot meets (0 for a swap when ni < 2); 'len' int64 [3, N]
    is the row, after slot 0, after slot 1 (ops.token_strong_len)."""
    n0 = np.asarray(n0, dtype=np.int64)
    op = rng.integers(1, 5, size=(2, n0.size))
    u = rng.random((2, n0.size))
    seed = rng.integers(0, 2 ** 32, size=(2, n0.size))
    c, lens = np.zeros_like(op), [n0]
    for s in (0, 1):
        ni = np.maximum(lens[s] - 2, 0)
        c[s] = np.minimum(np.floor(u[s] * rate * ni).astype(np.int64), ni)
        c[s][(op[s] == ops.TOKEN_SWAP) & (ni < 2)] = 0
        lens.append(ops.token_strong_len(lens[s], op[s], c[s]))
    return {"op": op, "c": c, "seed": seed, "len": np.stack(lens)}


class TokenTrainLoader(RaggedTrainLoader):
    """Per-step dicts of one epoch: consecutive ``batch_size`` chunks of the sampler's stream (drop_last).  'idx_*' the dataset indices,
    'y_*' the targets, 'x_*' the sentence and 'x_*_s' one of its variants, picked uniformly -- every view a ``TokenBatch`` right-padded to
    the longest row of ITS OWN batch (the collator's ``padding=True``; the views of a step are NOT padded to a common length), one
    srhip_token_view launch.  ``strong=False`` leaves the strong views out: not drawn, not launched.  The draws are a function of
    (``seed``, epoch): ``set_epoch`` / iterating again replays them.  Everything an epoch needs -- its index stream, targets and store rows --
    goes to the device in ONE copy when the epoch starts; the per-batch lengths are computed on the host from ``row_len_host`` (vectorised;
    nothing is read back from the device).  ``draws`` keeps the host arrays of the last epoch started:
    {view key: (store rows int64 [N], padded length of every batch int64 [len(self)])}.

    ``device_strong=True`` (``device_tokens_strong``): 'x_*_s' is made on the device from the CLEAN sentence instead -- two token-level slots
    (delete / mask / cutoff / swap at ``rate``) drawn per sample and epoch (``draw_token_slots``), one srhip_token_strong launch, no host
    synchronisation, no allocation besides the view.  The two packed slot rows ride behind the view's store rows in the same one copy and are
    drawn last, so every other view is what it is without the option; the padded length of a batch is its longest OUTPUT row, by the host's
    length rule.  ``strong_draws`` keeps the draws of the last epoch started: 'op' / 'c' / 'seed' int64 [2, N], 'len' int64 [3, N]."""
    mode_key, data_s_help = "device_tokens", DATA_S_HELP

    def __init__(self, dataset, batch_size, sampler, strong=True, keys=("idx_lb", "x_lb", "y_lb"), seed=(0,), device_strong=False,
                 rate=STRONG_RATE, mask_id=MASK_ID):
        self.makes_strong = bool(device_strong)
        super().__init__(dataset, batch_size, sampler, strong, keys, seed)
        if self.makes_strong and any(self._is_strong(k) for k in self.keys):
            if dataset.n_variants:
                raise ValueError("%s: the unlabelled set carries data_s (pre-augmented variants) and the strong view is to be made on the device: "
                                 "there must be one source of strong views -- drop data_s or the key" % STRONG_KEY)
            self.rate, self.mask_id = check_strong_rate(rate), int(mask_id)
            if self.mask_id < 0:
                raise ValueError("%s: %s = %d is no token id" % (STRONG_KEY, MASK_ID_KEY, self.mask_id))
            self.Lsrc = int(dataset.row_len_host.max())
            if self.Lsrc > ops.TOKEN_STRONG_MAX_LSRC:
                raise ValueError("%s: sentence %d holds %d tokens, more than the %d srhip_token_strong keeps in LDS"
                                 % (STRONG_KEY, int(dataset.row_len_host.argmax()), self.Lsrc, ops.TOKEN_STRONG_MAX_LSRC))
            self.strong_draws = None

    def _copy(self, table):
        return _h2d(table, self.dataset.device)

    def _draw(self, rng, key, src):
        """No table row beyond the store rows; the padded length of every batch comes from the host's copy of the row lengths.  A device-made
        strong view adds its two packed slot rows, and its batches are as long as their longest output row."""
        lens, B, nb = self.dataset.row_len_host, self.batch_size, len(self)
        ops.check_token_rows(src, lens)
        if not (self.makes_strong and self._is_strong(key)):
            return [], (src, lens[src[:nb * B]].reshape(nb, B).max(axis=1).astype(np.int64))
        sd = self.strong_draws = draw_token_slots(rng, lens[src], self.rate)
        slots = np.stack([ops.pack_token_slot(sd["op"][s], sd["c"][s], sd["seed"][s]) for s in (0, 1)])
        padded = sd["len"][2][:nb * B].reshape(nb, B).max(axis=1).astype(np.int64)
        ops.check_token_strong(src[:nb * B], slots[:, :nb * B], np.repeat(padded, B), lens, self.Lsrc)
        return [slots[0], slots[1]], (src, padded)

    def _view_fn(self, dev, row, draw, key):
        ds, B, src, lengths = self.dataset, self.batch_size, dev[row], draw[1].tolist()
        if not (self.makes_strong and self._is_strong(key)):
            return lambda s, t: _view(ds, src[s:s + B], lengths[t])
        from ..nets.bert import TokenBatch
        slot0, slot1, Lsrc, mask_id, token_strong = dev[row + 1], dev[row + 2], self.Lsrc, self.mask_id, ops.token_strong
        return lambda s, t: TokenBatch(*token_strong(ds.store, ds.row_off, ds.row_len, src[s:s + B], slot0[s:s + B], slot1[s:s + B], lengths[t],
                                                     Lsrc, ds.pad_id, mask_id))


class TokenEvalLoader(RaggedEvalLoader):
    """The dataset in order, last partial batch kept: {'x_lb': TokenBatch, 'y_lb'}, every batch right-padded to its own longest row -- the
    reference's evaluation collator.  The host knows the lengths: no synchronisation and no host-to-device copy."""

    def _view(self, s, e, length):
        return _view(self.dataset, self._rows[s:e], length)


# ---- the tokenizer (needed only when a dataset holds strings) ----------------------------------------------------------------------------
def load_tokenizer(directory, tried=()):
    """``BertTokenizerFast.from_pretrained(directory, local_files_only=True)``: the vocabulary of a directory on disk, never the network."""
    tried = list(tried) or [directory]
    if not (os.path.isdir(directory) and any(os.path.isfile(os.path.join(directory, f)) for f in TOKENIZER_FILES)):
        raise RuntimeError("device_tokens: %s holds no tokenizer files (%s); tried: %s" % (directory, " / ".join(TOKENIZER_FILES), ", ".join(map(str, tried))))
    try:
        from transformers import BertTokenizerFast
    except ImportError as e:
        raise RuntimeError("device_tokens: the datasets hold strings and transformers is not importable (%s): install it, or pass "
                           "already-tokenised integer arrays; tokenizer directory tried: %s" % (e, ", ".join(map(str, tried))))
    return BertTokenizerFast.from_pretrained(directory, local_files_only=True)


def resolve_tokenizer(args):
    """The tokenizer of the net's snapshot directory as nets/pretrained.find_snapshot resolves it: ``pretrain_path``, else the hub cache."""
    from ..nets.pretrained import find_snapshot
    net = str(getattr(args, "net", "") or "")
    snap, tried = find_snapshot(HUB_NAMES.get(net), getattr(args, "pretrain_path", None))
    if snap is None:
        raise RuntimeError("device_tokens: the datasets hold strings and no snapshot directory with a tokenizer was found for net %r (tried: %s): "
                           "set pretrain_path to a directory holding config.json, the weights and vocab.txt, or pass already-tokenised integer "
                           "arrays" % (net, ", ".join(map(str, tried)) or "nothing to try"))
    return load_tokenizer(snap, tried)


def make_tokenize(tokenizer, max_length):
    """The collator's call (nlp_collactor.py:51): str -> list of ids, truncated to ``max_length`` with [SEP] kept last, not padded."""
    return lambda text: tokenizer(text, max_length=max_length, truncation=True, padding=False)["input_ids"]


# ---- the option's wiring (core/algorithmbase.py) -----------------------------------------------------------------------------------------
def _is_token_net(net):
    net = str(net or "").lower()
    return "bert" in net and "hubert" not in net


def refuse_unsupported(args):
    """The configurations the token loaders do not cover, each with its reason, decided from the yaml keys before any array is moved."""
    active_mode(args, "device_tokens")
    net =getattr(args, "net", None)
    if net and not _is_token_net(net):
        raise NotImplementedError("device_tokens covers the usb_nlp token pipelines only (ClassificationBert backbones): net %r does not take "
                                  "token batches" % (net,))
    sampler = getattr(args, "train_sampler", "RandomSampler")
    if sampler != "RandomSampler":
        raise NotImplementedError("device_tokens: train_sampler %r is not supported (only 'RandomSampler', the reference's DistributedSampler "
                                  "index stream, is restated on the device path)" % (sampler,))
    view_length(args)
    device_strong(args)


def device_strong(args):
    """Whether ``device_tokens_strong`` is on -- refused without ``device_tokens``, whose resident token store it reads, and with a rate
    outside (0, 1]."""
    on = bool(getattr(args, STRONG_KEY, False))
    if on and not getattr(args, "device_tokens", False):
        raise ValueError("%s: True makes the strong token view on the device from the resident token store: it needs device_tokens: True" % STRONG_KEY)
    if on:
        check_strong_rate(getattr(args, STRONG_RATE_KEY, None))
    return on


def check_strong_rate(rate):
    rate = STRONG_RATE if rate is None else rate
    if isinstance(rate, bool) or not isinstance(rate, (int, float)) or not 0.0 < float(rate) <= 1.0:
        raise ValueError("%s: %s = %r must lie in (0, 1] (the largest share of a sentence's interior one slot touches)" % (STRONG_KEY, STRONG_RATE_KEY, rate))
    return float(rate)


def strong_mask_id(args, tokenizer=None):
    """``device_tokens_mask_id`` when set; else the resolved tokenizer's ``mask_token_id``; else 103, [MASK] of both reference vocabularies."""
    key = getattr(args, MASK_ID_KEY, None)
    if key is not None:
        return int(key)
    tok = getattr(tokenizer, "mask_token_id", None)
    return MASK_ID if tok is None else int(tok)


def view_length(args):
    ml = getattr(args, "max_length", None)
    if ml is None or int(ml) <= 0:
        raise ValueError("device_tokens needs args.max_length (the length the tokenizer truncates every sentence to), got %r" % (ml,))
    return int(ml)


def refuse_unsupported_model(model, dataset_dict=None):
    """Decided from the model once it exists, before anything is launched: a backbone that takes no token batches, ``max_length`` beyond its
    position table, a stored id beyond its vocabulary (the embedding kernel indexes the table with the ids: a bad id must never reach it)."""
    if not getattr(model, "takes_tokens", False):
        raise NotImplementedError("device_tokens covers the usb_nlp token pipelines only: this backbone (%s) does not take token batches"
                                  % type(model).__name__)
    for name, ds in (dataset_dict or {}).items():
        if not isinstance(ds, DeviceTokenDataset):
            continue
        mask_id = getattr(ds, "strong_mask_id", None)          # set where device_tokens_strong makes views of this set
        if mask_id is not None and (mask_id >= model.cfg.vocab or mask_id == ds.pad_id or mask_id < 0):
            raise ValueError("%s: %s = %d %s (set %s to the vocabulary's [MASK] id)"
                             % (STRONG_KEY, MASK_ID_KEY, mask_id, "is the store's pad_id" if mask_id == ds.pad_id else
                                "lies outside the model's vocabulary of %d" % model.cfg.vocab, MASK_ID_KEY))
        longest = int(ds.row_len_host.max()) if ds.max_length is None else ds.max_length
        if longest > model.cfg.max_pos:
            raise ValueError("device_tokens: max_length = %d of dataset %r exceeds the model's %d positions (max_pos)" % (longest, name, model.cfg.max_pos))
        if ds.max_id_host >= model.cfg.vocab:
            raise ValueError("device_tokens: dataset %r holds token id %d, outside the model's vocabulary of %d (the tokenizer and the "
                             "checkpoint do not belong together)" % (name, ds.max_id_host, model.cfg.vocab))


def _holds_strings(dset):
    if dset is None or isinstance(dset, DeviceTokenDataset):
        return False
    data = list(dset["data"] if isinstance(dset, dict) else dset.data)
    for var in ((dset.get("data_s") if isinstance(dset, dict) else getattr(dset, "data_s", None)) or ()):
        data += list(var)
    return _triples(data) is not None or any(_is_text(x) for x in data)


def build_token_datasets(args, dataset_dict, device):
    """dataset_dict values (reference-style objects, plain dicts or None) -> DeviceTokenDataset / None, same keys.  The tokenizer is looked
    for only when a set holds strings; with already-tokenised rows transformers is never imported."""
    refuse_unsupported(args)
    max_length = view_length(args)
    tokenizer = resolve_tokenizer(args) if any(_holds_strings(v) for v in dataset_dict.values()) else None
    tokenize = None if tokenizer is None else make_tokenize(tokenizer, max_length)
    out = {k: (None if v is None else DeviceTokenDataset.from_reference(v, device, tokenize, max_length)) for k, v in dataset_dict.items()}
    if out.get("train_ulb") is not None:                                  # what the strong views of this set mask with; checked against the model
        out["train_ulb"].strong_mask_id = strong_mask_id(args, tokenizer) if device_strong(args) else None
    return out


def build_token_loaders(args, dataset_dict, step_keys, num_train_iter, epochs, num_replicas, rank, print_fn=print):
    """The loader_dict of AlgorithmBase.set_data_loader from resident datasets: train_lb (batch_size), train_ulb (batch_size * uratio),
    eval / test (eval_batch_size).  ``step_keys``: the parameter names of the algorithm's train_step -- a view it does not take is not made."""
    for name in ("train_lb", "train_ulb"):
        if dataset_dict.get(name) is None:
            raise ValueError("device_tokens: dataset_dict[%r] is missing or None; the train loaders need a labelled and an unlabelled set (every "
                             "train_step of this project takes x_lb and x_ulb_w)" % name)
    made, ulb = device_strong(args), dataset_dict["train_ulb"]
    if made and ulb.n_variants:
        raise ValueError("%s: the unlabelled set carries data_s (pre-augmented variants) and the key asks for strong views made on the device: "
                         "there must be one source of strong views -- drop data_s or the key" % STRONG_KEY)
    if "x_ulb_s" in step_keys and ulb.n_variants == 0 and not made:
        raise ValueError("device_tokens: this algorithm's train_step takes x_ulb_s but the unlabelled set has no data_s; " + DATA_S_HELP)
    if not made:
        return build_loaders(args, dataset_dict, step_keys, num_train_iter, epochs, num_replicas, rank, TokenTrainLoader, TokenEvalLoader)
    rate = check_strong_rate(getattr(args, STRONG_RATE_KEY, None))
    mask_id = getattr(ulb, "strong_mask_id", None)
    mask_id = strong_mask_id(args) if mask_id is None else mask_id
    return build_loaders(args, dataset_dict, step_keys, num_train_iter, epochs, num_replicas, rank,
                         lambda ds, bs, sampler, strong, keys, seed: TokenTrainLoader(ds, bs, sampler, strong=strong, keys=keys, seed=seed,
                                                                                      device_strong=True, rate=rate, mask_id=mask_id),
                         TokenEvalLoader)


def eval_loader(args, dataset, batch_size, print_fn=print):
    """The evaluation view of one resident dataset, as the 'eval' loader of build_token_loaders makes it."""
    return TokenEvalLoader(dataset, batch_size)
