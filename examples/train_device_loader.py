#!/usr/bin/env python
"""End-to-end on one MI355X through the library's own input pipeline (``device_data: True``): the synthetic task of
examples/train_synthetic_cifar.py, stored at 64 x 64 and trained at img_size 32.  The arrays go in as a plain ``dataset_dict``; the engine
resizes them once on the device (Pillow's bilinear, csrc/resize.hip), builds the reference's sampler stream and the per-step weak / strong
views (data/device_loader.py), and ``alg.train()`` / ``alg.evaluate()`` run with no hand-written batch generator.

    python examples/train_device_loader.py --steps 100
    python examples/train_device_loader.py --steps 100 --run-hooks     # the reference's evaluation / checkpoint / logging hooks drive the run
"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semireward_amd.algorithms import get_algorithm          # noqa: E402
from semireward_amd.core.hooks import Hook                   # noqa: E402
from semireward_amd.nets import vit                          # noqa: E402


def synth_dataset(n, num_classes, seed, size):
    """uint8 [n, size, size, 3] images whose colour / stripe pattern depends on the class (the same pattern at every stored size), + labels."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y = rng.integers(0, num_classes, size=n)
    base = np.random.Generator(np.random.PCG64(12345)).integers(40, 216, size=(num_classes, 1, 1, 3))     # class prototypes: same for every split
    freq = 1 + np.arange(num_classes) % 7
    xs = (np.arange(size) * (32.0 / size))[None, None, :, None]
    img = base[y] + 35 * np.sin(xs * freq[y][:, None, None, None] * 0.4) + rng.normal(0, 18, size=(n, size, size, 3))
    return np.clip(img, 0, 255).astype(np.uint8), y.astype(np.int64)


class PrintHook(Hook):
    def after_train_step(self, alg):
        if alg.it % 10 == 0 or alg.it == alg.num_train_iter - 1:
            print("it %3d  epoch %d  sup %.3f  unsup %.3f  util %.2f" % (alg.it, alg.epoch, float(alg.log_dict["train/sup_loss"]),
                                                                        float(alg.log_dict["train/unsup_loss"]),
                                                                        float(alg.log_dict["train/util_ratio"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--stored-size", type=int, default=64)
    ap.add_argument("--run-hooks", action="store_true",
                    help="run_hooks + device_eval: evaluate and checkpoint every 20 steps (into a temporary save_dir), log every 10")
    a = ap.parse_args()
    C, H0 = a.classes, a.stored_size
    x_lb, y_lb = synth_dataset(40 * C // 10, C, 1, H0)             # "40 labels"-style split
    x_ulb, _ = synth_dataset(2048, C, 2, H0)
    x_te, y_te = synth_dataset(512, C, 3, H0)
    steps = max(a.steps, 40) // a.epochs * a.epochs
    args = argparse.Namespace(
        algorithm="srflexmatch", num_classes=C, num_train_iter=steps, epoch=a.epochs, ema_m=0.0, ulb_loss_ratio=1.0, use_cat=True, amp=False,
        lr=5e-4, weight_decay=5e-4, layer_decay=0.5, num_warmup_iter=5, optim="AdamW", T=0.5, p_cutoff=0.95, hard_label=True, thresh_warmup=True,
        N_k=10, start_timing=20, feature_dim=384, sr_lr=5e-4, sr_ema=False, sr_ema_m=0.99, gpu=0, rank=0, world_size=1, distributed=False, seed=0,
        # the input pipeline: what a usb_cv yaml says (dataset, img_size, crop_ratio, batch sizes, sampler) + the arrays + the option
        dataset="cifar100", img_size=32, crop_ratio=0.875, batch_size=a.batch, uratio=1, eval_batch_size=128, train_sampler="RandomSampler",
        device_data=True,
        dataset_dict={"train_lb": {"data": x_lb, "targets": y_lb}, "train_ulb": {"data": x_ulb, "targets": None},
                      "eval": {"data": x_te, "targets": y_te}})
    if a.run_hooks:
        with tempfile.TemporaryDirectory() as save_dir:
            vars(args).update(run_hooks=True, device_eval=True, num_eval_iter=20, num_log_iter=10, save_dir=save_dir, save_name="example")
            alg = get_algorithm(args, vit.vit_small_patch2_32)
            alg.train()
            print("results:", alg.results_dict, " files:", sorted(os.listdir(os.path.join(save_dir, "example"))))
            ev = alg.evaluate("eval")
    else:
        alg = get_algorithm(args, vit.vit_small_patch2_32)
        alg.register_hook(PrintHook(), "PrintHook", "LOWEST")
        alg.train()
        ev = alg.evaluate("eval")
    print("eval:", {k: round(float(v), 4) for k, v in ev.items()})
    return ev


if __name__ == "__main__":
    main()
