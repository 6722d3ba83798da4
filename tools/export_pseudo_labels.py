#!/usr/bin/env python
"""yaml + checkpoint -> ``.npz`` of pseudo labels for the whole unlabelled set (``AlgorithmBase.score_unlabeled``, core/pl_table.py).

    python tools/export_pseudo_labels.py --c config/SemiReward/usb_cv/flexmatch/flexmatch_cifar100_200_0.yaml \\
        --load saved_models/run/latest_model.pth --out pseudo_labels.npz [--set device_data=True] [--ema] [--batch-size 256] [--reward-group 8]

The yaml is read as a training run reads it (semireward_amd.config.get_config); ``--set key=value`` lays keys on top (python literals).  The
unlabelled rows come from the device input mode the configuration turns on (device_data / device_audio / device_tokens): its evaluation
loader over ``train_ulb``, the unaugmented view in index order.  The datasets are the reference's own (``semilearn`` importable) unless the
process that imports this module hands ``dataset_dict`` in through ``main(overrides=...)``.  ``--targets file.npy``: true labels (-1 =
unknown) for the printed accuracies; they are not stored.
"""
import argparse
import ast
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semireward_amd.algorithms import get_algorithm          # noqa: E402
from semireward_amd.config import get_config                 # noqa: E402
from semireward_amd.nets import get_net_builder              # noqa: E402


def _literal(v):
    try:
        return ast.literal_eval(v)
    except (ValueError, SyntaxError):
        return v


def main(argv=None, overrides=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--c", required=True, help="the run's yaml")
    ap.add_argument("--load", required=True, help="checkpoint written by save_model (latest_model.pth / model_best.pth)")
    ap.add_argument("--out", required=True, help="the .npz to write")
    ap.add_argument("--set", action="append", default=[], metavar="KEY=VALUE", help="a key laid on top of the yaml (repeatable)")
    ap.add_argument("--ema", action="store_true", help="score with the EMA weights (default: the model the thresholds were calibrated on)")
    ap.add_argument("--batch-size", type=int, default=None, help="rows per batch (default: eval_batch_size)")
    ap.add_argument("--reward-group", type=int, default=None, help="rows per Rewarder group (default: batch_size * uratio, the training step's)")
    ap.add_argument("--targets", default=None, help=".npy with one true label per unlabelled sample, -1 = unknown: accuracies in the summary")
    a = ap.parse_args(argv)
    ov = dict(overrides or {})
    for kv in a.set:
        k, _, v = kv.partition("=")
        ov[k] = _literal(v)
    ov.setdefault("gpu", 0)
    args = get_config(a.c, ov)
    alg = get_algorithm(args, get_net_builder(args.net, args.net_from_name))
    alg.load_model(a.load)
    table = alg.score_unlabeled(use_ema_model=a.ema, batch_size=a.batch_size, reward_group=a.reward_group)
    table.save(a.out)
    s = table.summary(np.load(a.targets) if a.targets else None)
    print("wrote %s: %d entries, %d scored, %d selected (ratio %.4f), algorithm %s at it %d, mode %s, reward groups of %d" % (
        a.out, table.n, s["rows"], s["selected"], s["selected_ratio"], table.meta["algorithm"], table.meta["it"], table.meta["mode"],
        table.meta["reward_group"]))
    print("selected per class:", s["selected_by_class"].tolist())
    if a.targets:
        print("accuracy over the %d rows with a known label: all %.4f, threshold-kept %.4f, selected %.4f" % (
            s["rows_known"], s["acc_all"], s["acc_threshold_kept"], s["acc_selected"]))
    return table


if __name__ == "__main__":
    main()
