#!/usr/bin/env python
"""Host time per training batch of the input pipeline at the reference batch (8 labelled / 8 + 8 unlabelled views, three srhip_augment
launches): the device loaders (data/device_loader.py, vectorised GpuAugment.pack) beside the hand-written generator of
examples/train_synthetic_cifar.py with the loop ``pack`` it had before the loaders existed (kept verbatim in tests/test_cpu_device_loader.py).
time.perf_counter around next(...), no device synchronisation inside the timed region (what the training loop's host thread pays); the
device is drained between the two measurements.
Then ``pack`` alone (host only, strong draws of 3 ops) at several batch sizes: where the vectorised form overtakes the loop.
The loop lives only in the test file, as the yardstick of the vectorised code, so this tool imports it from there (and with it pytest and
the oracle): run it from a tree that has tests/.

    python tools/device_loader_hosttime.py [--steps 400] > profiles/device_loader.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
from semireward_amd.data import device_loader as DL          # noqa: E402
from semireward_amd.data.augment import GpuAugment           # noqa: E402

DEV = "cuda:0"
MEAN, STD = DL.DATASET_STATS["cifar100"]


def timed(it, steps, warm):
    for _ in range(warm):
        next(it)
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        next(it)
        ts.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    ts = np.array(ts) * 1e6
    return ts


def report(name, ts):
    print("%-58s median %7.1f us   mean %7.1f us   p10 %7.1f   p90 %7.1f   (n = %d)" % (name, np.median(ts), ts.mean(), np.percentile(ts, 10),
                                                                                      np.percentile(ts, 90), len(ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    a = ap.parse_args()
    from train_synthetic_cifar import synth_dataset
    B = 8
    x_lb, y_lb = synth_dataset(40, 10, 1)
    x_ulb, _ = synth_dataset(2048, 10, 2)
    n = a.steps + a.warmup

    # ---- the device loaders
    lb, ulb = DL.DeviceImageDataset(x_lb, y_lb, 32, DEV), DL.DeviceImageDataset(x_ulb, None, 32, DEV)
    ld_l = DL.DeviceTrainLoader(lb, B, DL.EpochSampler(len(lb), n * B), GpuAugment(32, 4, MEAN, STD, device=DEV), seed=(0, 0, 0))
    ld_u = DL.DeviceTrainLoader(ulb, B, DL.EpochSampler(len(ulb), n * B), GpuAugment(32, 4, MEAN, STD, device=DEV),
                                keys=("idx_ulb", "x_ulb_w", "x_ulb_s"), seed=(0, 0, 1))
    new = timed(zip(ld_l, ld_u), a.steps, a.warmup)

    # ---- the example's generator, with the loop pack
    from test_cpu_device_loader import _pack_loop
    aug = GpuAugment(32, 4, MEAN, STD, n_ops=3, device=DEV, seed=0)
    aug.pack = lambda d, src_index=None: _pack_loop(32, d, src_index)
    lbt, ulbt = torch.from_numpy(x_lb).to(DEV), torch.from_numpy(x_ulb).to(DEV)
    rng = np.random.Generator(np.random.PCG64(0))

    def batches():
        while True:
            il, iu = rng.integers(0, len(x_lb), size=B), rng.permutation(len(x_ulb))[:B]
            yield {"x_lb": aug(lbt, False, src_index=il), "y_lb": torch.from_numpy(y_lb[il]).to(DEV), "idx_ulb": torch.from_numpy(iu).to(DEV),
                   "x_ulb_w": aug(ulbt, False, src_index=iu), "x_ulb_s": aug(ulbt, True, src_index=iu)}
    old = timed(batches(), a.steps, a.warmup)

    # ---- the example's generator with the vectorised pack (what of the difference is pack, what is sampling + label / index copies)
    aug2 = GpuAugment(32, 4, MEAN, STD, n_ops=3, device=DEV, seed=0)
    aug = aug2
    mid = timed(batches(), a.steps, a.warmup)

    print("host time per training batch, 8 / 8 / 8 images of 32 x 32, three srhip_augment launches; %s (%s, %d CUs), torch %s" % (
        torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName, torch.cuda.get_device_properties(0).multi_processor_count,
        torch.__version__))
    report("device loaders (vectorised pack)", new)
    report("example generator, loop pack (before)", old)
    report("example generator, vectorised pack", mid)

    print("GpuAugment.pack alone, strong draws (3 ops), host only: us per call, median of 300 calls after 30")
    for Bp in (8, 16, 24, 32, 56, 64, 448):
        ag = GpuAugment(32, 4, MEAN, STD, n_ops=3, device=DEV, seed=2)
        ds = [ag.draw(Bp, True) for _ in range(330)]
        row = []
        for f in (lambda d: _pack_loop(32, d), ag.pack):
            ts = []
            for d in ds:
                t0 = time.perf_counter()
                f(d)
                ts.append(time.perf_counter() - t0)
            row.append(np.median(np.array(ts[30:]) * 1e6))
        print("  B = %3d   loop %8.1f us   vectorised %8.1f us   (x %.2f)" % (Bp, row[0], row[1], row[1] / row[0]))


if __name__ == "__main__":
    main()
