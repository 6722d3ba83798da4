#!/usr/bin/env python
"""Score and export the pseudo labels of a whole unlabelled set on one MI355X, in seconds: the synthetic task of
examples/train_device_loader.py at 8 x 8 on the tiny test ViT.  A short SRFlexMatch run (``device_data: True``), then
``alg.score_unlabeled()`` walks the unlabelled store in index order -- the unaugmented evaluation view, no training state touched -- and the
table says which samples the model would pseudo-label now, with which label and confidence, and which of them the Rewarder keeps.

    python examples/export_pseudo_labels.py --steps 40 --out pseudo_labels.npz
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semireward_amd.algorithms import get_algorithm          # noqa: E402
from semireward_amd.core.pl_table import PseudoLabelTable    # noqa: E402
from semireward_amd.nets import vit                          # noqa: E402

SIZE = 8


def synth_dataset(n, num_classes, seed):
    """uint8 [n, 8, 8, 3] images whose colour depends on the class, + labels."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y = rng.integers(0, num_classes, size=n)
    base = np.random.Generator(np.random.PCG64(12345)).integers(40, 216, size=(num_classes, 1, 1, 3))
    img = base[y] + rng.normal(0, 18, size=(n, SIZE, SIZE, 3))
    return np.clip(img, 0, 255).astype(np.uint8), y.astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--unlabelled", type=int, default=500)
    ap.add_argument("--out", default=None, help="write the table to this .npz")
    a = ap.parse_args()
    C = a.classes
    x_lb, y_lb = synth_dataset(4 * C, C, 1)
    x_ulb, y_ulb = synth_dataset(a.unlabelled, C, 2)          # the true labels stay on the host: only summary() sees them
    x_te, y_te = synth_dataset(64, C, 3)
    steps = max(a.steps, 8) // 2 * 2
    args = argparse.Namespace(
        algorithm="srflexmatch", num_classes=C, num_train_iter=steps, epoch=2, ema_m=0.0, ulb_loss_ratio=1.0, use_cat=True, amp=False,
        lr=5e-4, weight_decay=5e-4, layer_decay=0.5, num_warmup_iter=2, optim="AdamW", T=0.5, p_cutoff=0.5, hard_label=True, thresh_warmup=True,
        N_k=10, start_timing=steps // 2, feature_dim=128, sr_lr=5e-4, sr_ema=False, sr_ema_m=0.99, gpu=0, rank=0, world_size=1,
        distributed=False, seed=0, dataset="cifar100", img_size=SIZE, crop_ratio=0.875, batch_size=8, uratio=1, eval_batch_size=128,
        train_sampler="RandomSampler", device_data=True,
        dataset_dict={"train_lb": {"data": x_lb, "targets": y_lb}, "train_ulb": {"data": x_ulb, "targets": None},
                      "eval": {"data": x_te, "targets": y_te}})
    alg = get_algorithm(args, vit.vit_tiny_test)
    alg.train()
    table = alg.score_unlabeled()                                # loader=None: the device mode's evaluation loader over train_ulb
    s = table.summary(y_ulb)
    print("rows %d  selected %d (ratio %.3f)  acc_all %.3f  acc_threshold_kept %.3f  acc_selected %.3f" % (
        s["rows"], s["selected"], s["selected_ratio"], s["acc_all"], s["acc_threshold_kept"], s["acc_selected"]))
    print("selected per class:", s["selected_by_class"].tolist())
    c = table.read()
    for j in np.argsort(-c["conf"])[:5]:
        print("  sample %4d  label %d  conf %.3f  margin %.3f  entropy %.3f  weight %.0f  reward %.3f  selected %d" % (
            j, c["label"][j], c["conf"][j], c["margin"][j], c["entropy"][j], c["weight"][j], c["reward"][j], c["selected"][j]))
    if a.out:
        table.save(a.out)
        back = PseudoLabelTable.load(a.out)
        print("wrote %s: %d entries, mode %s, it %d, reward_group %d" % (a.out, back.n, back.meta["mode"], back.meta["it"],
                                                                       back.meta["reward_group"]))
    return table


if __name__ == "__main__":
    main()
