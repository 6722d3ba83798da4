"""Device-resident train / eval loaders of the usb_cv configurations (``device_data: True``): the dataset arrays live in HBM as uint8, the
reference's sampler decides which samples form a batch, and the views of a batch are one srhip_augment launch each -- no PIL, no torchvision,
no worker processes, no per-step H2D image copy.

Restates, with the random draws of the transforms replaced by ``GpuAugment.draw`` (the reference's come from unseeded per-worker global RNGs):
  semilearn/datasets/cv_datasets/datasetbase.py:72-111   which keys a labelled / unlabelled sample carries
  semilearn/datasets/samplers/sampler.py:55-73           the epoch's index stream (DistributedSampler.__iter__)
  semilearn/core/utils/build.py:176-182                  samples per epoch, consecutive batches, drop_last
  semilearn/datasets/cv_datasets/{cifar,stl10,eurosat}.py  Resize -> [crop, flip, (RandAugment)] -> ToTensor -> Normalize
``transforms.Resize`` is the first, deterministic op of all three transforms, so it is applied once to the stored array (csrc/resize.hip)."""
import numpy as np
import torch

from .. import ops
from .augment import GpuAugment
from .modes import build_loaders
from .ragged import EpochLoader

# Normalize statistics of the reference's transforms (cv_datasets/cifar.py:16-21, stl10.py:16-18, eurosat.py:37-38)
DATASET_STATS = {
    "cifar100": ([x / 255 for x in (129.3, 124.1, 112.4)], [x / 255 for x in (68.2, 65.4, 70.4)]),
    "stl10": ([x / 255 for x in (112.4, 109.1, 98.6)], [x / 255 for x in (68.4, 66.6, 68.5)]),
    "eurosat": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),
}
ROLES = {"train_lb": 0, "train_ulb": 1}          # the loader's role in the seed of its draws


class DeviceImageDataset:
    """uint8 [n, H0, H0, 3] images (numpy or torch) -> resident uint8 [n, S, S, 3] on ``device`` (resized like PIL's BILINEAR when
    H0 != S), int64 targets resident too (None: unlabelled).  ``targets_host`` keeps a numpy copy for the host-side gathers of a loader."""

    def __init__(self, data_u8, targets, img_size, device):
        if not torch.is_tensor(data_u8):
            data_u8 = np.asarray(data_u8)
        if data_u8.dtype != (torch.uint8 if torch.is_tensor(data_u8) else np.uint8):     # (checked before torch sees it: a list of file paths is a str array, not a tensor)
            raise ValueError("device_data needs decoded uint8 image arrays (the reference's BasicDataset.data; a dataset that keeps file "
                             "paths, as its EuroSat does, must be decoded first), got dtype %s" % data_u8.dtype)
        data = data_u8 if torch.is_tensor(data_u8) else torch.from_numpy(np.ascontiguousarray(data_u8))
        if data.dim() != 4 or data.shape[-1] != 3:
            raise ValueError("device_data needs [n, H, W, 3] image arrays, got shape %s" % (tuple(data.shape),))
        if data.shape[1] != data.shape[2]:
            raise ValueError("device_data needs square images (the Pillow-exact resize covers H == W only), got %d x %d" % tuple(data.shape[1:3]))
        self.device, self.img_size, self.stored_size = torch.device(device), int(img_size), int(data.shape[1])
        data = data.contiguous().to(self.device)
        self.data = data if self.stored_size == self.img_size else ops.resize_bilinear_u8(data, self.img_size)
        if targets is None:
            self.targets = self.targets_host = None
        else:
            self.targets_host = np.asarray(targets.cpu() if torch.is_tensor(targets) else targets).astype(np.int64)
            if self.targets_host.shape != (len(self.data),):
                raise ValueError("targets must hold one label per image")
            self.targets = torch.from_numpy(self.targets_host).to(self.device)

    @classmethod
    def from_reference(cls, dset, img_size, device):
        """A reference-style dataset object (``.data``, ``.targets``, ``.is_ulb``) or a plain {'data': ..., 'targets': ...} dict."""
        if isinstance(dset, cls):
            return dset
        if isinstance(dset, dict):
            return cls(dset["data"], dset.get("targets"), img_size, device)
        ulb = bool(getattr(dset, "is_ulb", False))
        return cls(dset.data, None if ulb else getattr(dset, "targets", None), img_size, device)

    def __len__(self):
        return int(self.data.shape[0])


class EpochSampler:
    """The index stream of the reference's DistributedSampler: a CPU generator seeded with the epoch, whole permutations of range(n) plus a
    truncated one up to ``num_samples_total`` indices, of which this rank takes every ``num_replicas``-th starting at ``rank``."""

    def __init__(self, n, num_samples_total, num_replicas=1, rank=0):
        if not isinstance(num_samples_total, int) or num_samples_total <= 0:
            raise ValueError("num_samples_total should be a positive integer, got %r" % (num_samples_total,))
        if num_samples_total % num_replicas:
            raise ValueError("%d samples cannot be evenly distributed among %d ranks" % (num_samples_total, num_replicas))
        self.n, self.total, self.num_replicas, self.rank, self.epoch = int(n), num_samples_total, int(num_replicas), int(rank), 0
        self.num_samples = self.total // self.num_replicas

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def indices(self):
        g = torch.Generator()
        g.manual_seed(self.epoch)
        parts = [torch.randperm(self.n, generator=g) for _ in range(self.total // self.n)]
        parts.append(torch.randperm(self.n, generator=g)[:self.total % self.n])
        return torch.cat(parts).numpy()[self.rank:self.total:self.num_replicas]

    def __iter__(self):
        return iter(self.indices().tolist())

    def __len__(self):
        return self.num_samples


class DeviceTrainLoader(EpochLoader):
    """Per-step dicts of one epoch: consecutive ``batch_size`` chunks of the sampler's stream (drop_last).  ``keys`` name what a sample
    carries: 'idx_*' the dataset indices, 'y_*' the targets, 'x_*' a weak view and 'x_*_s' a strong view of the stored image -- every view an
    independent draw of ``aug`` (one srhip_augment launch).  ``strong=False`` leaves the strong views out: not drawn, not launched.
    The draws are a function of (``seed``, epoch): ``set_epoch`` / iterating again replays them."""

    def __init__(self, dataset, batch_size, sampler, aug, strong=True, keys=("idx_lb", "x_lb", "y_lb"), seed=(0,)):
        super().__init__(dataset, batch_size, sampler, strong, keys, seed)
        self.aug = aug

    def __iter__(self):
        self.sampler.set_epoch(self.epoch)
        self.aug.reseed(self.seed + (self.epoch,))
        stream = self.sampler.indices()
        B, ds = self.batch_size, self.dataset
        idx_dev = torch.from_numpy(np.ascontiguousarray(stream)).to(ds.device)             # one copy per epoch, sliced per step
        y_dev = torch.from_numpy(ds.targets_host[stream]).to(ds.device) if ds.targets is not None else None
        for s in range(0, len(self) * B, B):
            idx, out = stream[s:s + B], {}
            for k in self.keys:
                if k.startswith("idx"):
                    out[k] = idx_dev[s:s + B]
                elif k.startswith("y"):
                    out[k] = y_dev[s:s + B]
                else:
                    out[k] = self.aug(ds.data, self._is_strong(k), src_index=idx)
            yield out


class DeviceEvalLoader:
    """transform_val over the dataset in order, last partial batch kept: {'x_lb', 'y_lb'} with x_lb = Normalize(ToTensor(resized image)) --
    ``aug`` is one GpuAugment(S, 0, mean, std) reused for every batch, with zero crop offset and no flip."""

    def __init__(self, dataset, batch_size, aug):
        if dataset.targets is None:
            raise ValueError("the evaluation loader needs a labelled dataset")
        self.dataset, self.batch_size, self.aug = dataset, int(batch_size), aug

    def __len__(self):
        return -(-len(self.dataset) // self.batch_size)

    def __iter__(self):
        ds, n = self.dataset, len(self.dataset)
        for s in range(0, n, self.batch_size):
            b = min(self.batch_size, n - s)
            d = dict(i=np.zeros(b, dtype=np.int64), j=np.zeros(b, dtype=np.int64), flip=np.zeros(b, dtype=bool))
            yield {"x_lb": self.aug(ds.data, False, draws=d, src_index=np.arange(s, s + b)), "y_lb": ds.targets[s:s + b]}


def refuse_unsupported(args):
    """The configurations the device loaders do not cover, each with its reason, decided from the yaml keys before any array is moved."""
    net = str(getattr(args, "net", "") or "").lower()
    if "bert" in net and "hubert" not in net:
        raise NotImplementedError("device_data covers the usb_cv image pipelines only: net %r takes token batches (usb_nlp)" % (args.net,))
    if "wave2vec" in net or "hubert" in net:
        raise NotImplementedError("device_data covers the usb_cv image pipelines only: net %r takes waveforms (usb_audio)" % (args.net,))
    sampler = getattr(args, "train_sampler", "RandomSampler")
    if sampler != "RandomSampler":
        raise NotImplementedError("device_data: train_sampler %r is not supported (only 'RandomSampler', the reference's DistributedSampler "
                                  "index stream, is restated on the device path)" % (sampler,))
    if getattr(args, "img_size", None) is None:
        raise ValueError("device_data needs args.img_size (the training resolution every transform resizes to)")


def refuse_unsupported_model(model, dataset_dict=None):
    """The same refusal for a builder handed in without a ``net`` name: decided from the model once it exists (the arrays are resident by then)."""
    from ..nets.wave2vec import ClassificationWave2Vec
    if getattr(model, "takes_tokens", False):
        raise NotImplementedError("device_data covers the usb_cv image pipelines only: this backbone takes token batches (usb_nlp)")
    if isinstance(model, ClassificationWave2Vec):
        raise NotImplementedError("device_data covers the usb_cv image pipelines only: this backbone takes waveforms (usb_audio)")


def dataset_stats(args):
    mean, std = getattr(args, "dataset_mean", None), getattr(args, "dataset_std", None)
    if mean is not None and std is not None:
        return tuple(mean), tuple(std)
    name = getattr(args, "dataset", None)
    if name not in DATASET_STATS:
        raise ValueError("device_data: no Normalize statistics for dataset %r: set args.dataset_mean / args.dataset_std (known: %s)"
                         % (name, ", ".join(sorted(DATASET_STATS))))
    return DATASET_STATS[name]


def build_device_datasets(args, dataset_dict, device):
    """dataset_dict values (reference-style objects, plain dicts or None) -> DeviceImageDataset / None, same keys."""
    refuse_unsupported(args)
    return {k: (None if v is None else DeviceImageDataset.from_reference(v, args.img_size, device)) for k, v in dataset_dict.items()}


def build_device_loaders(args, dataset_dict, step_keys, num_train_iter, epochs, num_replicas, rank, print_fn=print):
    """The loader_dict of AlgorithmBase.set_data_loader from resident datasets: train_lb (batch_size), train_ulb (batch_size * uratio),
    eval / test (eval_batch_size).  ``step_keys``: the parameter names of the algorithm's train_step -- a view it does not take is not made."""
    S = int(args.img_size)
    pad = int(S * (1 - getattr(args, "crop_ratio", 0.875)))          # RandomCrop(padding=...) of the transforms; train.py's default ratio
    mean, std = dataset_stats(args)
    return build_loaders(args, dataset_dict, step_keys, num_train_iter, epochs, num_replicas, rank,
                         lambda ds, bs, sampler, strong, keys, seed: DeviceTrainLoader(ds, bs, sampler, GpuAugment(S, pad, mean, std, n_ops=3, device=ds.device),
                                                                                       strong=strong, keys=keys, seed=seed),
                         lambda ds, bs: eval_loader(args, ds, bs))


def eval_loader(args, dataset, batch_size, print_fn=print):
    """transform_val over one resident dataset, as the 'eval' loader of build_device_loaders makes it."""
    mean, std = dataset_stats(args)
    return DeviceEvalLoader(dataset, batch_size, GpuAugment(int(args.img_size), 0, mean, std, device=dataset.device))
