"""What the device input modes share.  ``EpochLoader``: the part of a train loader that is the same for images, waveforms and tokens (which
keys a step gets, the seed of the epoch's draws, ``set_epoch``).  ``RaggedStore`` / ``RaggedTrainLoader`` / ``RaggedEvalLoader``: rows of any
length in one flat device array, an epoch as ONE int64 host table and one host-to-device copy, and the evaluation pass in index order -- the
waveform mode (data/device_audio.py) and the token mode (data/device_tokens.py) add their row validation, their draws and their one launch
per view, and say which reference lines they follow."""
import numpy as np
import torch


def _h2d(t, device):
    """Every host-to-device copy of the ragged loaders goes through here (one per epoch and train loader; the tests count them)."""
    return t.to(device)


def with_variants(validate, data, data_s, key, noun, data_s_help):
    """``data`` and the V lists of ``data_s`` through ``validate(rows, what)`` -> (rows with the variants appended behind the originals, n, V)."""
    rows = validate(data, "data")
    n, n_variants = len(rows), 0
    if n == 0:
        raise ValueError("%s: the dataset holds no %s" % (key, noun))
    if data_s is not None:
        for v, var in enumerate(data_s):
            var = validate(var, "data_s[%d]" % v)
            if len(var) != n:
                raise ValueError("%s: data_s[%d] must hold one variant of every %s (%d), got %d" % (key, v, noun, n, len(var)))
            rows += var
        n_variants = len(data_s)
        if n_variants == 0:
            raise ValueError("%s: data_s is empty; %s" % (key, data_s_help))
    return rows, n, n_variants


class RaggedStore:
    """Validated rows (contiguous 1-D numpy arrays of one dtype) in one flat device array ``store``; row r occupies
    store[row_off[r] : row_off[r] + row_len[r]] and starts at a multiple of 4 elements (the gap holds ``fill``).  Rows 0 .. n - 1 are the
    originals, row n (1 + v) + i is variant v of row i (``strong_row``).  int64 targets resident too (None: unlabelled); ``targets_host`` /
    ``row_len_host`` / ``row_off_host`` keep numpy copies for the host side of a loader."""

    def __init__(self, rows, n, n_variants, targets, device, fill, noun):
        self.n, self.n_variants, self.device = n, n_variants, torch.device(device)
        self.row_len_host = np.array([r.size for r in rows], dtype=np.int32)
        padded = (self.row_len_host.astype(np.int64) + 3) & ~np.int64(3)
        self.row_off_host = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
        flat = np.full(int(padded.sum()), fill, dtype=rows[0].dtype)
        for r, o in zip(rows, self.row_off_host):
            flat[o:o + r.size] = r
        self.store = torch.from_numpy(flat).to(self.device)
        self.row_off = torch.from_numpy(self.row_off_host).to(self.device)
        self.row_len = torch.from_numpy(self.row_len_host).to(self.device)
        if targets is None:
            self.targets = self.targets_host = None
        else:
            self.targets_host = np.asarray(targets.cpu() if torch.is_tensor(targets) else targets).astype(np.int64)
            if self.targets_host.shape != (self.n,):
                raise ValueError("targets must hold one label per %s (%d %ss, targets of shape %s)" % (noun, self.n, noun, self.targets_host.shape))
            self.targets = torch.from_numpy(self.targets_host).to(self.device)

    @staticmethod
    def reference_fields(dset):
        """(data, targets, data_s) of a reference-style dataset object (``.data``, ``.targets``, ``.is_ulb``, optionally ``.data_s``) or of a
        plain {'data': [...], 'targets': ..., 'data_s': [[...], ...]} dict."""
        if isinstance(dset, dict):
            return dset["data"], dset.get("targets"), dset.get("data_s")
        ulb = bool(getattr(dset, "is_ulb", False))
        return dset.data, None if ulb else getattr(dset, "targets", None), getattr(dset, "data_s", None)

    def strong_row(self, variant, index):
        return self.n * (1 + np.asarray(variant, dtype=np.int64)) + np.asarray(index, dtype=np.int64)

    def __len__(self):
        return self.n


class EpochLoader:
    """Per-step dicts of one epoch: consecutive ``batch_size`` chunks of the sampler's stream (drop_last).  ``keys`` name what a sample
    carries: 'idx_*' the dataset indices, 'y_*' the targets, 'x_*' a weak view and 'x_*_s' a strong view; ``strong=False`` leaves the strong
    views out.  The draws are a function of (``seed``, epoch): ``set_epoch`` / iterating again replays them."""

    def __init__(self, dataset, batch_size, sampler, strong, keys, seed):
        self.dataset, self.batch_size, self.sampler = dataset, int(batch_size), sampler
        self.keys = tuple(k for k in keys if strong or not self._is_strong(k))
        if any(k.startswith("y") for k in self.keys) and dataset.targets is None:
            raise ValueError("a loader with a target key needs a labelled dataset")
        self.seed = tuple(int(s) for s in seed)
        self.epoch = 0

    @staticmethod
    def _is_strong(k):
        return k.startswith("x") and k.endswith("_s")

    def set_epoch(self, epoch):
        self.epoch = int(epoch)
        self.sampler.set_epoch(epoch)

    def __len__(self):
        return len(self.sampler) // self.batch_size


class RaggedTrainLoader(EpochLoader):
    """Everything an epoch needs -- its index stream, targets, the store rows of every view and what ``_draw`` adds -- goes to the device in ONE
    copy when the epoch starts, sliced per step; a view is one launch.  A strong view reads one of the row's variants, picked uniformly.
    ``draws`` keeps the host arrays of the last epoch started, {view key: (store rows int64 [N], the mode's second array)}.
    A mode sets ``mode_key`` / ``data_s_help`` (its messages) and the two hooks ``_draw`` and ``_view_fn``.  A loader whose ``makes_strong`` is
    set makes its strong view itself, from the clean row: no variant is drawn and none is needed, the strong key's store rows are the stream."""
    makes_strong = False

    def __init__(self, dataset, batch_size, sampler, strong=True, keys=("idx_lb", "x_lb", "y_lb"), seed=(0,)):
        super().__init__(dataset, batch_size, sampler, strong, keys, seed)
        if any(self._is_strong(k) for k in self.keys) and dataset.n_variants == 0 and not self.makes_strong:
            raise ValueError("%s: a strong view was asked of a dataset without data_s; %s" % (self.mode_key, self.data_s_help))
        self.draws = {}

    def _draw(self, rng, key, src):
        """(the table rows a view adds behind its store rows ``src``, draws[key]); draws from ``rng`` and checks the rows on the host."""
        raise NotImplementedError

    def _view_fn(self, dev, row, draw, key):
        """f(s, t) -> the view ``key`` of step t (stream positions s .. s + batch_size) from the device table, whose ``row`` holds the store rows."""
        raise NotImplementedError

    def _copy(self, table):
        """The epoch's one host-to-device copy.  A mode overrides this with the same line so that the copy goes through the ``_h2d`` name of
        its own module, where that mode's tests count the copies."""
        return _h2d(table, self.dataset.device)

    def _epoch_table(self):
        """The epoch as one int64 host table [rows, N] and the meaning of its rows: {key: row} ('idx' / 'y': the values; views: the store
        rows, with the rows of ``_draw`` behind them)."""
        ds = self.dataset
        self.sampler.set_epoch(self.epoch)
        rng = np.random.Generator(np.random.PCG64(self.seed + (self.epoch,)))
        stream = np.ascontiguousarray(self.sampler.indices(), dtype=np.int64)
        N, rows, where, self.draws = stream.size, [], {}, {}
        for k in self.keys:
            where[k] = len(rows)
            if k.startswith("idx"):
                rows.append(stream)
            elif k.startswith("y"):
                rows.append(ds.targets_host[stream])
            else:
                variant = self._is_strong(k) and not self.makes_strong
                src = ds.strong_row(rng.integers(0, ds.n_variants, size=N), stream) if variant else stream
                extra, self.draws[k] = self._draw(rng, k, src)
                rows += [src] + extra
        return np.stack(rows), where, N

    def __iter__(self):
        B = self.batch_size
        table, where, N = self._epoch_table()
        dev = self._copy(torch.from_numpy(table))                                          # the epoch's one copy, sliced per step
        cols = [(k, None, self._view_fn(dev, where[k], self.draws[k], k)) if k in self.draws else (k, dev[where[k]], None) for k in self.keys]
        for t in range(len(self)):
            s, out = t * B, {}
            for k, col, view in cols:                                                      # (the rows are cut once per epoch: a step only slices)
                out[k] = col[s:s + B] if view is None else view(s, t)
            yield out


class RaggedEvalLoader:
    """The dataset in order, last partial batch kept: {'x_lb', 'y_lb'}, every row taken from its first element and the batch padded to its own
    longest row (at most ``L`` where a mode sets it).  The host knows the lengths: no synchronisation and no host-to-device copy."""
    L = None

    def __init__(self, dataset, batch_size):
        if dataset.targets is None:
            raise ValueError("the evaluation loader needs a labelled dataset")
        self.dataset, self.batch_size = dataset, int(batch_size)
        self._rows = torch.arange(len(dataset), dtype=torch.int64, device=dataset.device)          # made on the device: nothing to copy

    def __len__(self):
        return -(-len(self.dataset) // self.batch_size)

    def batch_lengths(self):
        ds, n = self.dataset, len(self.dataset)
        lens = [int(ds.row_len_host[s:min(s + self.batch_size, n)].max()) for s in range(0, n, self.batch_size)]
        return lens if self.L is None else [min(x, self.L) for x in lens]

    def _view(self, s, e, length):
        """The view of rows s .. e - 1 padded to ``length``: the mode's one launch."""
        raise NotImplementedError

    def __iter__(self):
        ds, n = self.dataset, len(self.dataset)
        for s, length in zip(range(0, n, self.batch_size), self.batch_lengths()):
            e = min(s + self.batch_size, n)
            yield {"x_lb": self._view(s, e, length), "y_lb": ds.targets[s:e]}
