"""Device-resident waveform store and loaders of the usb_audio configurations (``device_audio: True``): every clip lives in HBM in one flat
fp32 array, the reference's sampler decides which clips form a batch, and a view of a batch -- crop, zero padding, the feature extractor's
normalisation -- is one srhip_wave_view launch (csrc/wave_view.hip).  No ``random_subsample`` in Python, no numpy feature extractor, no worker
processes, no per-step host-to-device copy.

Restates
  semilearn/datasets/audio_datasets/datasetbase.py:84-133   which keys a labelled / unlabelled sample carries, train crops, eval takes the clip whole
  semilearn/datasets/utils.py:177-183                       random_subsample: offset uniform on [0, len - L - 1] when len > L (the last window is never drawn)
  semilearn/datasets/collactors/audio_collactor.py:45-110   Wav2Vec2FeatureExtractor: truncate to int(max_length * sample_rate), pad, normalise
  semilearn/datasets/samplers/sampler.py:55-73              the epoch's index stream (EpochSampler of data/device_loader.py, unchanged)
with the reference's unseeded draws (``random.randint`` in every worker process) replaced by a numpy generator seeded with
(seed, rank, loader role, epoch).  Two deviations, both documented in configs/README.md:
  * every training view is padded to L = int(round(sample_rate * max_length_seconds)) samples.  The reference pads x_lb / x_ulb_w to the
    batch's own longest row and only the strong view to L; the step concatenates the three views, so they need one length.  The two agree
    whenever a batch holds a clip of at least L samples.
  * the strong view is a crop of a PRE-AUGMENTED variant of the clip (``data_s``).  The reference runs a random sox effect chain on the CPU
    (torchaudio.sox_effects, unseeded): it can be neither restated on the device nor pinned by a fixture."""
import json
import os

import numpy as np
import torch

from .. import ops
from .device_loader import ROLES, EpochSampler             # noqa: F401  (re-exported: tests and tools reach them through this module)
from .modes import active_mode, build_loaders
from .ragged import RaggedEvalLoader, RaggedStore, RaggedTrainLoader, _h2d, with_variants

HUB_NAMES = {"wave2vecv2_base": "facebook/wav2vec2-base-960h", "hubert_base": "facebook/hubert-base-ls960"}     # the reference's collators (audio_collactor.py:115-124)
DATA_S_HELP = ("the strong view must be precomputed: give the unlabelled set V >= 1 pre-augmented variants of every clip as "
               "{'data': [...], 'data_s': [[variant 0 of every clip], [variant 1 ...], ...]} (e.g. the reference's WaveformTransforms applied V times "
               "on a machine that has torchaudio; configs/README.md has the recipe)")


def _clips(data, what):
    """A list of 1-D float arrays -> list of contiguous float32 arrays, each refusal with its reason."""
    out = []
    for i, c in enumerate(data):
        c = c.detach().cpu().numpy() if torch.is_tensor(c) else np.asarray(c)
        if c.dtype.kind != "f":
            raise ValueError("device_audio needs float waveforms (the reference's BasicDataset.data: a list of 1-D float arrays), got dtype %s "
                             "for clip %d of %s" % (c.dtype, i, what))
        if c.ndim != 1:
            raise ValueError("device_audio needs 1-D (mono) clips, got shape %s for clip %d of %s" % (c.shape, i, what))
        if c.size == 0:
            raise ValueError("device_audio: clip %d of %s is empty" % (i, what))
        out.append(np.ascontiguousarray(c, dtype=np.float32))
    return out


class DeviceWaveDataset(RaggedStore):
    """Clips of any length in one flat fp32 device array ``store``; clip r occupies store[row_off[r] : row_off[r] + row_len[r]] and starts at
    a multiple of 4 floats (the gap is zero).  Rows 0 .. n - 1 are the clips; with ``data_s`` (V lists of n pre-augmented variants) row
    n (1 + v) + i is variant v of clip i (``strong_row``).  int64 targets resident too (None: unlabelled); ``targets_host`` / ``row_len_host`` /
    ``row_off_host`` keep numpy copies for the host side of a loader."""

    def __init__(self, data, targets, device, data_s=None):
        clips, n, n_variants = with_variants(_clips, data, data_s, "device_audio", "clip", DATA_S_HELP)
        super().__init__(clips, n, n_variants, targets, device, 0, "clip")

    @classmethod
    def from_reference(cls, dset, device):
        """A reference-style dataset object (``.data``, ``.targets``, ``.is_ulb``, optionally ``.data_s``) or a plain
        {'data': [...], 'targets': ..., 'data_s': [[...], ...]} dict."""
        if isinstance(dset, cls):
            return dset
        data, targets, data_s = cls.reference_fields(dset)
        return cls(data, targets, device, data_s)


def crop_offsets(rng, lens, L):
    """random_subsample's offset for clips of ``lens`` samples: 0 when len <= L, else uniform on [0, len - L - 1], both ends included."""
    lens = np.asarray(lens, dtype=np.int64)
    off = rng.integers(0, np.maximum(lens - L, 1))             # (high is exclusive)
    return np.where(lens <= L, 0, off).astype(np.int32)


class WaveTrainLoader(RaggedTrainLoader):
    """Per-step dicts of one epoch: consecutive ``batch_size`` chunks of the sampler's stream (drop_last).  'idx_*' the dataset indices, 'y_*'
    the targets, 'x_*' a crop of the clip and 'x_*_s' a crop of one of its pre-augmented variants, picked uniformly -- every view fp32
    [batch_size, L], one srhip_wave_view launch.  ``strong=False`` leaves the strong views out: not drawn, not launched.  The draws are a
    function of (``seed``, epoch): ``set_epoch`` / iterating again replays them.  Everything an epoch needs -- its index stream, targets, store
    rows and crop offsets -- goes to the device in ONE copy when the epoch starts; ``draws`` keeps the host arrays of the last epoch started:
    {view key: (store rows int64 [N], crop offsets int32 [N])}."""
    mode_key, data_s_help = "device_audio", DATA_S_HELP

    def __init__(self, dataset, batch_size, sampler, L, normalize=True, strong=True, keys=("idx_lb", "x_lb", "y_lb"), seed=(0,)):
        self.L, self.normalize = int(L), bool(normalize)
        super().__init__(dataset, batch_size, sampler, strong, keys, seed)

    def _copy(self, table):
        return _h2d(table, self.dataset.device)

    def _draw(self, rng, key, src):
        """One more table row behind the store rows: its first N int32 are the crop offsets."""
        lens = self.dataset.row_len_host
        crop = crop_offsets(rng, lens[src], self.L)
        ops.check_wave_rows(src, crop, lens)
        packed = np.zeros(src.size, dtype=np.int64)
        packed.view(np.int32)[:src.size] = crop
        return [packed], (src, crop)

    def _view_fn(self, dev, row, draw):
        ds, B, L, normalize, wave_view = self.dataset, self.batch_size, self.L, self.normalize, ops.wave_view
        store, row_off, row_len = ds.store, ds.row_off, ds.row_len
        src, crop = dev[row], dev.view(torch.int32)[row + 1]                               # (as int32 the table is [rows, 2 N]: the crop offsets are the first N)
        return lambda s, t: wave_view(store, row_off, row_len, src[s:s + B], crop[s:s + B], L, normalize)


class WaveEvalLoader(RaggedEvalLoader):
    """The dataset in order, last partial batch kept: {'x_lb', 'y_lb'} with every clip taken from its first sample, truncated to L and the
    batch padded to its own longest row (at most L) -- the reference's evaluation collator (``padding=True, truncation=True``).  The host
    knows the lengths: no synchronisation and no host-to-device copy."""

    def __init__(self, dataset, batch_size, L, normalize=True):
        super().__init__(dataset, batch_size)
        self.L, self.normalize = int(L), bool(normalize)
        self._crop = torch.zeros(len(dataset), dtype=torch.int32, device=dataset.device)

    def _view(self, s, e, length):
        ds = self.dataset
        return ops.wave_view(ds.store, ds.row_off, ds.row_len, self._rows[s:e], self._crop[s:e], length, self.normalize)


# ---- the option's wiring (core/algorithmbase.py) -----------------------------------------------------------------------------------------
def _is_audio_net(net):
    net = str(net or "").lower()
    return "wave2vec" in net or "hubert" in net


def refuse_unsupported(args):
    """The configurations the waveform loaders do not cover, each with its reason, decided from the yaml keys before any array is moved."""
    active_mode(args, "device_audio")
    net = getattr(args, "net", None)
    if net and not _is_audio_net(net):
        raise NotImplementedError("device_audio covers the usb_audio waveform pipelines only (ClassificationWave2Vec / HuBERT backbones): "
                                  "net %r does not take waveforms" % (net,))
    sampler = getattr(args, "train_sampler", "RandomSampler")
    if sampler != "RandomSampler":
        raise NotImplementedError("device_audio: train_sampler %r is not supported (only 'RandomSampler', the reference's DistributedSampler "
                                  "index stream, is restated on the device path)" % (sampler,))
    view_length(args)


def refuse_unsupported_model(model, dataset_dict=None):
    """The same refusal for a builder handed in without a ``net`` name: decided from the model once it exists."""
    from ..nets.wave2vec import ClassificationWave2Vec
    if not isinstance(model, ClassificationWave2Vec):
        raise NotImplementedError("device_audio covers the usb_audio waveform pipelines only: this backbone (%s) is not a "
                                  "ClassificationWave2Vec / HuBERT and does not take waveforms" % type(model).__name__)


def view_length(args):
    """L = int(round(sample_rate * max_length_seconds)), the window of random_subsample -- refused when the collator's
    int(max_length_seconds * sample_rate) is another number (the reference would crop to one and truncate to the other)."""
    mls, sr = getattr(args, "max_length_seconds", None), getattr(args, "sample_rate", None)
    if mls is None or sr is None:
        raise ValueError("device_audio needs args.max_length_seconds and args.sample_rate (the window every training view is cropped and padded to)")
    L = int(round(sr * mls))
    if L != int(mls * sr) or L <= 0:
        raise ValueError("device_audio: int(round(sample_rate * max_length_seconds)) = %d (random_subsample's window) differs from "
                         "int(max_length_seconds * sample_rate) = %d (the collator's max_length), or is not positive" % (L, int(mls * sr)))
    return L


def resolve_normalize(args, print_fn=print):
    """Whether the views are normalised: the yaml key ``audio_do_normalize`` when set; else ``do_normalize`` of preprocessor_config.json in the
    snapshot directory nets/pretrained.find_snapshot resolves for the net (what AutoFeatureExtractor.from_pretrained reads); else True (the
    default of Wav2Vec2FeatureExtractor and of both reference checkpoints) with one warning line."""
    key = getattr(args, "audio_do_normalize", None)
    if key is not None:
        return bool(key)
    from ..nets.pretrained import find_snapshot
    net = str(getattr(args, "net", "") or "")
    snap, tried = find_snapshot(HUB_NAMES.get(net), getattr(args, "pretrain_path", None))
    cfg = os.path.join(snap, "preprocessor_config.json") if snap else None
    if cfg is None or not os.path.isfile(cfg):
        print_fn("warning: device_audio found no preprocessor_config.json for net %r (tried: %s): the views are normalised (do_normalize: True, "
                 "the feature extractor's default); set audio_do_normalize to choose" % (net, ", ".join(map(str, tried)) or "nothing to try"))
        return True
    with open(cfg) as f:
        pc = json.load(f)
    if pc.get("return_attention_mask", False):
        raise NotImplementedError("device_audio: %s sets return_attention_mask: true -- the feature extractor then normalises every clip over its "
                                  "own samples only (masked statistics), which srhip_wave_view does not build" % cfg)
    return bool(pc.get("do_normalize", True))


def build_wave_datasets(args, dataset_dict, device):
    """dataset_dict values (reference-style objects, plain dicts or None) -> DeviceWaveDataset / None, same keys."""
    refuse_unsupported(args)
    return {k: (None if v is None else DeviceWaveDataset.from_reference(v, device)) for k, v in dataset_dict.items()}


def build_wave_loaders(args, dataset_dict, step_keys, num_train_iter, epochs, num_replicas, rank, print_fn=print):
    """The loader_dict of AlgorithmBase.set_data_loader from resident datasets: train_lb (batch_size), train_ulb (batch_size * uratio),
    eval / test (eval_batch_size).  ``step_keys``: the parameter names of the algorithm's train_step -- a view it does not take is not made."""
    L = view_length(args)
    if "x_ulb_s" in step_keys and dataset_dict["train_ulb"].n_variants == 0:
        raise ValueError("device_audio: this algorithm's train_step takes x_ulb_s but the unlabelled set has no data_s; " + DATA_S_HELP)
    normalize = resolve_normalize(args, print_fn)
    return build_loaders(args, dataset_dict, step_keys, num_train_iter, epochs, num_replicas, rank,
                         lambda ds, bs, sampler, strong, keys, seed: WaveTrainLoader(ds, bs, sampler, L, normalize, strong=strong, keys=keys, seed=seed),
                         lambda ds, bs: WaveEvalLoader(ds, bs, L, normalize))


def eval_loader(args, dataset, batch_size, print_fn=print):
    """The evaluation view of one resident dataset, as the 'eval' loader of build_wave_loaders makes it."""
    return WaveEvalLoader(dataset, batch_size, view_length(args), resolve_normalize(args, print_fn))
