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
  * the strong view is a crop of a PRE-AUGMENTED variant of the clip (``data_s``), or -- ``device_audio_strong: True`` -- of the clip after two
    effects made on the device (srhip_wave_effect, csrc/wave_strong.hip), drawn afresh per sample and epoch.  The reference runs a random sox
    effect chain on the CPU (torchaudio.sox_effects, unseeded): sox's filters can be neither restated on the device nor pinned by a fixture.
    The device chain keeps the reference's structure and draw distributions (``draw_effects``: two of gain / pitch / speed / reverb with
    replacement, applied to the whole clip before the crop) with filters of the engine's own: a peak-normalising gain, one windowed-sinc
    resampler for speed and pitch (pitch changes the length by at most 0.12 %, sox keeps it by WSOLA), Freeverb.  Effects run one after the
    other at the clip's own rate; a clip shorter than the shortest comb delay leaves the reverb as silence."""
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


STRONG_KEY = "device_audio_strong"
MAX_GROWTH = 4                    # two slots, each at most doubles a clip (speed 0.5)
MAX_VIEW_SOURCE = 1 << 30         # the longest row srhip_wave_effect / srhip_wave_view address
EFFECTS = ("gain", "pitch", "speed", "reverb")                 # the reference's effects_list, in its order


def draw_effects(rng, n0):
    """The strong view's draws for clips of ``n0`` samples, the reference's rule (datasetbase.py:14-27) from ``rng``: per sample three uniforms,
    always drawn -- speed = 0.5 + 1.5 u, cents = -2 + 4 u, att = int(-5 + 10 u), truncated toward zero: an integer in -4 .. 4 -- then two effects
    uniform on 0 .. 3 with replacement (``random.choices(effects_list, k=2)``).  Returned with what srhip_wave_effect is given for them
    ('op', 'param': gain -> the fp32 bits of 10^(att / 20); pitch and speed -> the 32.32 fixed-point step round(s 2^32) with s = 2^(cents / 1200)
    and s = speed; reverb -> 0) and the length chain 'lens' [N, 3] by the kernel's integer rule (ops.wave_effect_len)."""
    n0 = np.asarray(n0, dtype=np.int64)
    u = rng.random((n0.size, 3))
    effect = rng.integers(0, 4, size=(n0.size, 2))
    speed, cents = 0.5 + 1.5 * u[:, 0], -2.0 + 4.0 * u[:, 1]
    att = np.clip(np.trunc(-5.0 + 10.0 * u[:, 2]), -4, 4).astype(np.int64)              # (u = 0 exactly would give -5: kept inside the stated range)
    gain = np.asarray(10.0 ** (att / 20.0), dtype=np.float32).view(np.uint32).astype(np.int64)
    step_pitch, step_speed = (np.floor(s * float(ops.WAVE_STEP_ONE) + 0.5).astype(np.int64) for s in (2.0 ** (cents / 1200.0), speed))
    op = np.array([ops.WAVE_GAIN, ops.WAVE_RESAMPLE, ops.WAVE_RESAMPLE, ops.WAVE_REVERB], dtype=np.int32)[effect]
    param = np.stack([gain, step_pitch, step_speed, np.zeros_like(gain)], axis=1)[np.arange(n0.size)[:, None], effect]
    n1 = ops.wave_effect_len(n0, op[:, 0], param[:, 0])
    n2 = ops.wave_effect_len(n1, op[:, 1], param[:, 1])
    return dict(speed=speed, cents=cents, att=att, effect=effect, op=op, param=param, lens=np.stack([n0, n1, n2], axis=1))


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
    {view key: (store rows int64 [N], crop offsets int32 [N])}.

    ``device_strong=True`` (``device_audio_strong``): 'x_*_s' is made on the device from the CLEAN clip instead -- two effects drawn per sample
    and epoch (``draw_effects``), two srhip_wave_effect launches through two scratch buffers [batch_size, pitch] allocated once, then the crop
    of the augmented clip by srhip_wave_view: three launches, no host synchronisation, no allocation besides the view.  The effect draws ride
    behind the view's rows in the same one copy and are drawn last, so every other view is what it is without the option.  ``strong_draws``
    keeps them for the last epoch started: 'speed' / 'cents' / 'att' [N], 'effect' [N, 2] (0 gain, 1 pitch, 2 speed, 3 reverb), 'op' int32
    [N, 2] and 'param' int64 [N, 2] (what srhip_wave_effect is given), 'lens' int64 [N, 3] (the clip, after slot 0, after slot 1)."""
    mode_key, data_s_help = "device_audio", DATA_S_HELP

    def __init__(self, dataset, batch_size, sampler, L, normalize=True, strong=True, keys=("idx_lb", "x_lb", "y_lb"), seed=(0,), device_strong=False,
                 sample_rate=None):
        self.L, self.normalize, self.makes_strong = int(L), bool(normalize), bool(device_strong)
        super().__init__(dataset, batch_size, sampler, strong, keys, seed)
        self.strong_draws = None
        if self.makes_strong and any(self._is_strong(k) for k in self.keys):
            if dataset.n_variants:
                raise ValueError("%s: the unlabelled set carries data_s (pre-augmented variants) and the strong view is to be made on the device: "
                                 "there must be one source of strong views -- drop data_s or the key" % STRONG_KEY)
            if not sample_rate or sample_rate <= 0:
                raise ValueError("%s needs the clips' sample_rate (the reverb's delays are set in samples)" % STRONG_KEY)
            longest = int(dataset.row_len_host.argmax())
            self.pitch = (MAX_GROWTH * int(dataset.row_len_host[longest]) + 3) & ~3        # each slot at most doubles a clip (speed 0.5)
            if self.pitch > MAX_VIEW_SOURCE:
                raise ValueError("%s: clip %d holds %d samples; after two effects it may hold %d times as many, beyond the 2^30 samples "
                                 "srhip_wave_view addresses" % (STRONG_KEY, longest, dataset.row_len_host[longest], MAX_GROWTH))
            dev, B = dataset.device, self.batch_size
            self.delays = ops.reverb_delays(sample_rate)
            self._scratch = [torch.empty(B, self.pitch, dtype=torch.float32, device=dev) for _ in range(2)]
            self._rows = torch.arange(B, dtype=torch.int64, device=dev)                    # a scratch row per batch row ...
            self._scratch_off = self._rows * self.pitch                                     # ... at a fixed pitch

    def _copy(self, table):
        return _h2d(table, self.dataset.device)

    def _draw(self, rng, key, src):
        """One more table row behind the store rows: its first N int32 are the crop offsets.  A device-made strong view adds its effects:
        [crop | op 0], [op 1 | length after slot 0], [length after slot 1 | -], param 0, param 1."""
        lens = self.dataset.row_len_host
        made = self.makes_strong and self._is_strong(key)
        if made:
            self.strong_draws = draw_effects(rng, lens[src])
            op, param, chain = (self.strong_draws[k] for k in ("op", "param", "lens"))
            crop = crop_offsets(rng, chain[:, 2], self.L)
            ops.check_wave_rows(np.arange(src.size), crop, chain[:, 2])
            ops.check_wave_rows(src, np.zeros_like(crop), lens)
        else:
            crop = crop_offsets(rng, lens[src], self.L)
            ops.check_wave_rows(src, crop, lens)

        def pack(lo, hi=None):
            packed = np.zeros(src.size, dtype=np.int64)
            packed.view(np.int32)[:src.size] = lo
            if hi is not None:
                packed.view(np.int32)[src.size:] = hi
            return packed
        if not made:
            return [pack(crop)], (src, crop)
        return [pack(crop, op[:, 0]), pack(op[:, 1], chain[:, 1]), pack(chain[:, 2]), param[:, 0].copy(), param[:, 1].copy()], (src, crop)

    def _view_fn(self, dev, row, draw, key):
        ds, B, L, normalize, wave_view = self.dataset, self.batch_size, self.L, self.normalize, ops.wave_view
        store, row_off, row_len = ds.store, ds.row_off, ds.row_len
        i32, N = dev.view(torch.int32), dev.shape[1]                                         # (as int32 the table is [rows, 2 N]: two arrays of N a row)
        src, crop = dev[row], i32[row + 1]
        if not (self.makes_strong and self._is_strong(key)):
            return lambda s, t: wave_view(store, row_off, row_len, src[s:s + B], crop[s:s + B], L, normalize)
        wave_effect, (a, b), rows, off, delays = ops.wave_effect, self._scratch, self._rows, self._scratch_off, self.delays
        op0, op1, len1, len2, par0, par1 = i32[row + 1][N:], i32[row + 2], i32[row + 2][N:], i32[row + 3], dev[row + 4], dev[row + 5]
        sd, h_src, h_len, h_rows = self.strong_draws, draw[0], ds.row_len_host, np.arange(B)      # the host arrays the entry checks: cut once per epoch
        (h_op0, h_op1), (h_par0, h_par1) = (np.ascontiguousarray(sd[k].T) for k in ("op", "param"))
        _, h_len1, h_len2 = np.ascontiguousarray(sd["lens"].T.astype(np.int32))

        def view(s, t):
            e = s + B
            wave_effect(store, row_off, row_len, src[s:e], op0[s:e], par0[s:e], len1[s:e], a, delays,
                        host=(h_src[s:e], h_op0[s:e], h_par0[s:e], h_len1[s:e], h_len))
            wave_effect(a, off, len1[s:e], rows, op1[s:e], par1[s:e], len2[s:e], b, delays,
                        host=(h_rows, h_op1[s:e], h_par1[s:e], h_len2[s:e], h_len1[s:e]))
            return wave_view(b, off, len2[s:e], rows, crop[s:e], L, normalize)
        return view


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
    device_strong(args)


def device_strong(args):
    """Whether ``device_audio_strong`` is on -- refused without ``device_audio``, whose resident clip store it reads."""
    on = bool(getattr(args, STRONG_KEY, False))
    if on and not getattr(args, "device_audio", False):
        raise ValueError("%s: True makes the strong waveform view on the device from the resident clip store: it needs device_audio: True" % STRONG_KEY)
    return on


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
    made = device_strong(args)
    if made and dataset_dict["train_ulb"].n_variants:
        raise ValueError("%s: the unlabelled set carries data_s (pre-augmented variants) and the key asks for strong views made on the device: "
                         "there must be one source of strong views -- drop data_s or the key" % STRONG_KEY)
    if "x_ulb_s" in step_keys and dataset_dict["train_ulb"].n_variants == 0 and not made:
        raise ValueError("device_audio: this algorithm's train_step takes x_ulb_s but the unlabelled set has no data_s; " + DATA_S_HELP)
    normalize = resolve_normalize(args, print_fn)
    sr = getattr(args, "sample_rate", None)
    return build_loaders(args, dataset_dict, step_keys, num_train_iter, epochs, num_replicas, rank,
                         lambda ds, bs, sampler, strong, keys, seed: WaveTrainLoader(ds, bs, sampler, L, normalize, strong=strong, keys=keys, seed=seed,
                                                                                     device_strong=made, sample_rate=sr),
                         lambda ds, bs: WaveEvalLoader(ds, bs, L, normalize))


def eval_loader(args, dataset, batch_size, print_fn=print):
    """The evaluation view of one resident dataset, as the 'eval' loader of build_wave_loaders makes it."""
    return WaveEvalLoader(dataset, batch_size, view_length(args), resolve_normalize(args, print_fn))
