#!/usr/bin/env python
"""What ``device_audio: True`` costs per batch (semireward_amd/data/device_audio.py, csrc/wave_view.hip), and what it replaces, on one box:

  * srhip_wave_view alone at B = 8, S = 64 000 (4 s at 16 kHz, the usb_audio yamls' batch), with and without normalisation: HIP events around
    ``--launches`` back-to-back launches, us per launch (execution + dispatch), median of 5 windows after one warm-up window;
  * the train loader's HOST time per batch: time.perf_counter around ``next()`` of the loader without a device synchronise (three views per
    step: x_lb, x_ulb_w, x_ulb_s), and separately the once-per-epoch set-up (the draws, the table, its one copy);
  * beside them the reference's collator on the same clips on this box's CPU: a Python random_subsample per clip and one numpy
    Wav2Vec2FeatureExtractor call per view (semilearn/datasets/collactors/audio_collactor.py), in the main process, no workers -- skipped with a
    note when transformers is not importable;
  * every kernel case of tests/_wave_view_cases.py against its bound (4 d_ref + 4 ulp): the share of the bound each one uses.

    python tools/device_audio_time.py > profiles/device_audio.txt
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
import _wave_view_cases as WC                                 # noqa: E402
from semireward_amd import ops                               # noqa: E402
from semireward_amd.data import device_audio as DA           # noqa: E402

DEV = "cuda:0"
B, S, RATE = 8, 64000, 16000


def per_launch(f, launches):
    ts = []
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            f()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / launches)
    return float(np.median(ts[1:]))


def clips(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [WC.clip(seed + i, int(k)) for i, k in enumerate(rng.integers(int(3.0 * RATE), int(6.0 * RATE), size=n))]      # 3 .. 6 s: cropped and padded rows


def kernel_alone(launches):
    ds = DA.DeviceWaveDataset(clips(64, 100), None, DEV)
    rng = np.random.Generator(np.random.PCG64(1))
    rows = rng.integers(0, len(ds), size=B)
    crop = DA.crop_offsets(rng, ds.row_len_host[rows], S)
    r, c = torch.from_numpy(rows).to(DEV), torch.from_numpy(crop).to(DEV)
    moved = 4.0 * (np.minimum(ds.row_len_host[rows] - crop, S).sum() + B * S)
    print("srhip_wave_view alone, B = %d, S = %d, crop_off %% 4 = %s, samples read per row %s" % (B, S, (crop % 4).tolist(),
                                                                                                 np.minimum(ds.row_len_host[rows] - crop, S).tolist()))
    for normalize in (False, True):
        t = per_launch(lambda: ops.wave_view(ds.store, ds.row_off, ds.row_len, r, c, S, normalize), launches)
        print("  normalize %-5s  %8.2f us per launch (HIP events around %d launches, output allocation included)   %.1f GB/s of the %.2f MB a view "
              "reads once and writes" % (normalize, t, launches, moved / t * 1e-3, moved * 1e-6))


def loader_host_time(epochs):
    lb, ulb = clips(100, 200), clips(512, 400)
    rng = np.random.Generator(np.random.PCG64(2))
    var = [[WC.clip(9000 + 1000 * v + i, int(len(c) * (0.8, 1.25)[v])) for i, c in enumerate(ulb)] for v in range(2)]
    dl = DA.DeviceWaveDataset(lb, rng.integers(0, 10, size=len(lb)), DEV)
    du = DA.DeviceWaveDataset(ulb, None, DEV, data_s=var)
    steps = 32
    ld_l = DA.WaveTrainLoader(dl, B, DA.EpochSampler(len(dl), steps * B, 1, 0), S, True, keys=("idx_lb", "x_lb", "y_lb"), seed=(0, 0, 0))
    ld_u = DA.WaveTrainLoader(du, B, DA.EpochSampler(len(du), steps * B, 1, 0), S, True, keys=("idx_ulb", "x_ulb_w", "x_ulb_s"), seed=(0, 0, 1))
    first, rest = [], []
    for e in range(epochs + 1):
        ld_l.set_epoch(e), ld_u.set_epoch(e)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        it_l, it_u = iter(ld_l), iter(ld_u)
        a, b = next(it_l), next(it_u)
        t1 = time.perf_counter()
        ts = []
        for _ in range(steps - 1):
            t2 = time.perf_counter()
            a, b = next(it_l), next(it_u)
            ts.append(time.perf_counter() - t2)
        torch.cuda.synchronize()
        if e:                                                 # (epoch 0: first launches, allocator warm-up)
            first.append(t1 - t0)
            rest += ts
    rest = np.array(rest) * 1e6
    print("train loaders, host time (no device synchronise inside the window), batch %d labelled + %d unlabelled, three views of %d samples per step" % (B, B, S))
    print("  per step             median %8.1f us   p10 %8.1f   p90 %8.1f   (n = %d; three launches, no host-to-device copy)" % (
        np.median(rest), np.percentile(rest, 10), np.percentile(rest, 90), len(rest)))
    print("  first step of an epoch  median %8.1f us   (the epoch's draws, its table and ONE copy per loader, + the step)" % (np.median(first) * 1e6))
    return lb, ulb, var


def collator_time(lb, ulb, var, steps=16):
    try:
        import random
        from transformers import Wav2Vec2FeatureExtractor
    except Exception as e:      # noqa: BLE001
        print("reference collator on the CPU: not measured (transformers not importable here: %s)" % type(e).__name__)
        return
    fe = Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=RATE, padding_value=0.0, do_normalize=True, return_attention_mask=False)

    def sub(w):
        if len(w) <= S:
            return w
        o = random.randint(0, len(w) - S - 1)
        return w[o:o + S]
    rng = np.random.Generator(np.random.PCG64(3))
    ts = []
    for t in range(steps + 2):
        il, iu = rng.integers(0, len(lb), size=B), rng.integers(0, len(ulb), size=B)
        t0 = time.perf_counter()
        for wins, pad in (([sub(lb[i]) for i in il], True), ([sub(ulb[i]) for i in iu], True), ([sub(var[t % 2][i]) for i in iu], "max_length")):
            fe(wins, padding=pad, max_length=S, sampling_rate=RATE, truncation=True, return_tensors="pt")["input_values"]
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts[2:]) * 1e6
    print("reference collator on this box's CPU (random_subsample + Wav2Vec2FeatureExtractor in numpy, main process, the same three views; the sox "
          "effect chain of its strong view and the copy to the device not included)")
    print("  per step             median %8.1f us   p10 %8.1f   p90 %8.1f   (n = %d)" % (np.median(ts), np.percentile(ts, 10), np.percentile(ts, 90), len(ts)))


def headroom():
    g = np.load(os.path.join(ROOT, "tests", "golden", "device_audio.npz"))
    print("kernel cases against the float64 oracle: d_ref (float32 extractor, CPU), the kernel's largest error, the bound 4 d_ref + 4 ulp_fp32(max |out|)")
    worst = 0.0
    for case in WC.kernel_cases():
        d_ref = float(g["kernel/%s/d_ref" % case["name"]])
        err, tol = WC.verify(case, d_ref, DEV)
        worst = max(worst, err / tol)
        print("  %-14s d_ref %.3e  kernel %.3e  bound %.3e  used %.3f" % (case["name"], d_ref, err, tol, err / tol))
    print("  largest share of a bound used: %.3f" % worst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--epochs", type=int, default=4)
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    print("device_audio; %s (%s, %d CUs), torch %s" % (torch.cuda.get_device_name(0), p.gcnArchName, p.multi_processor_count, torch.__version__))
    kernel_alone(a.launches)
    lb, ulb, var = loader_host_time(a.epochs)
    collator_time(lb, ulb, var)
    headroom()


if __name__ == "__main__":
    main()
