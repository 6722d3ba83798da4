"""The device-resident input modes, one record per yaml key, and what their wiring shares: which mode a configuration turns on
(``active_mode``) and the loader_dict every mode builds the same way (``build_loaders``).  A mode's module is imported when its key is on."""
import importlib

NEEDS = ("%s: True needs the %s: pass args.dataset_dict (reference dataset objects, or plain %s dicts), or install semilearn so that its "
         "get_dataset runs")


class Mode:
    """``key``: the yaml key.  ``what``: what the pipeline feeds.  ``refuse_early``: the yaml keys are refused before a dataset is looked at
    (the image mode refuses inside its ``build_datasets``).  ``loaders_line`` / ``needs_datasets``: the log line of set_data_loader and the
    RuntimeError of set_dataset.  The functions are looked up in the mode's module when they are called."""

    def __init__(self, key, module, what, refuse_early, datasets, loaders, loaders_line, needs, dict_shape):
        self.key, self.module, self.what, self.refuse_early, self.loaders_line = key, module, what, refuse_early, loaders_line
        self._datasets, self._loaders, self.needs_datasets = datasets, loaders, NEEDS % (key, needs, dict_shape)

    def _fn(self, name):
        return getattr(importlib.import_module(self.module, __package__), name)

    def refuse_unsupported(self, args):
        self._fn("refuse_unsupported")(args)

    def refuse_unsupported_model(self, model, dataset_dict):
        self._fn("refuse_unsupported_model")(model, dataset_dict)

    def build_datasets(self, args, dataset_dict, device):
        return self._fn(self._datasets)(args, dataset_dict, device)

    def build_loaders(self, args, dataset_dict, step_keys, num_train_iter, epochs, num_replicas, rank, print_fn):
        return self._fn(self._loaders)(args, dataset_dict, step_keys, num_train_iter, epochs, num_replicas, rank, print_fn)

    def eval_loader(self, args, dataset, batch_size, print_fn):
        return self._fn("eval_loader")(args, dataset, batch_size, print_fn)


# in the order of their refusals: a mode names the ones behind it when two keys are set
MODES = (
    Mode("device_tokens", ".device_tokens", "token batches", True, "build_token_datasets", "build_token_loaders",
         "Create device-resident token train and test data loaders", "sentences",
         "{'data': [strings or 1-D token arrays], 'targets': ..., 'data_s': [[...], [...]]}"),
    Mode("device_audio", ".device_audio", "waveforms", True, "build_wave_datasets", "build_wave_loaders",
         "Create device-resident waveform train and test data loaders", "clips",
         "{'data': [1-D float arrays], 'targets': ..., 'data_s': [[...], ...]}"),
    Mode("device_data", ".device_loader", "images", False, "build_device_datasets", "build_device_loaders",
         "Create device-resident train and test data loaders", "dataset arrays", "{'data': uint8 [n, H, W, 3], 'targets': ...}"),
)


def active_mode(args, also=None):
    """The record of the one key that is on (``also``: a key taken as on), or None; two keys are refused."""
    on = [m for m in MODES if m.key == also or bool(getattr(args, m.key, False))]
    if len(on) > 1:
        raise ValueError("%s and %s are two input pipelines (%s / %s): set one of them" % (on[0].key, on[-1].key, on[0].what, on[-1].what))
    return on[0] if on else None


def build_loaders(args, dataset_dict, step_keys, num_train_iter, epochs, num_replicas, rank, make_train, make_eval):
    """The loader_dict of AlgorithmBase.set_data_loader from resident datasets: train_lb (batch_size), train_ulb (batch_size * uratio) from
    ``make_train(ds, bs, sampler, strong, keys, seed)``, eval / test (eval_batch_size) from ``make_eval(ds, bs)``.  ``step_keys``: the
    parameter names of the algorithm's train_step -- a view it does not take is not made."""
    from .device_loader import ROLES, EpochSampler
    strong = "x_ulb_s" in step_keys
    seed = int(getattr(args, "seed", 0) or 0)
    per_epoch = num_train_iter // max(1, epochs)
    ld = {}
    for name, bs, keys in (("train_lb", args.batch_size, ("idx_lb", "x_lb", "y_lb")),
                           ("train_ulb", args.batch_size * args.uratio, ("idx_ulb", "x_ulb_w", "x_ulb_s"))):
        ds = dataset_dict[name]
        sampler = EpochSampler(len(ds), per_epoch * bs * num_replicas, num_replicas, rank)     # one seed (the epoch) for both, as the reference
        ld[name] = make_train(ds, bs, sampler, strong, keys, (seed, rank, ROLES[name]))
    for name in ("eval", "test"):
        if dataset_dict.get(name) is not None:
            ld[name] = make_eval(dataset_dict[name], args.eval_batch_size)
    return ld
