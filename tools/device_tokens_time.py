#!/usr/bin/env python
"""What ``device_tokens: True`` costs per batch (semireward_amd/data/device_tokens.py, csrc/token_view.hip), and what it replaces, on one box:

  * srhip_token_view alone at B = 8, L = 512 (the usb_nlp yamls' batch and max_length): HIP events around ``--launches`` back-to-back launches,
    us per launch (execution + dispatch), median of 5 windows after one warm-up window -- the raw entry on preallocated outputs, and beside it
    ``ops.token_view``, which also allocates ids and key_len;
  * the train loaders' HOST time per step: time.perf_counter around ``next()`` of both loaders without a device synchronise (three views per
    step: x_lb, x_ulb_w, x_ulb_s), and separately the first step of an epoch (the draws, the table, its one copy);
  * beside them the two paths replaced, on the same rows: ``tokenizer.pad`` of the already-tokenised lists on this box's CPU (the collator
    without its per-step tokenisation, main process; skipped with a note when transformers is not importable), and ``TokenBatch.from_dict`` of
    the padded host tensors (the copy to the device + the cast + srhip_mask_lengths), host time per step and, with events, device-side time.

Row lengths are a handful of values (128, 256, 384, 512).  Nothing here is a pass / fail number.

    python tools/device_tokens_time.py > profiles/device_tokens.txt
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _token_view_cases as TC                                # noqa: E402
from semireward_amd import ops                               # noqa: E402
from semireward_amd.data import device_tokens as DT          # noqa: E402
from semireward_amd.data.device_loader import EpochSampler   # noqa: E402
from semireward_amd.nets.bert import TokenBatch              # noqa: E402

DEV = "cuda:0"
B, L, VOCAB, LENGTHS = 8, 512, 30522, (128, 256, 384, 512)


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


def rows(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [np.concatenate([[TC.CLS], rng.integers(5, VOCAB, size=int(LENGTHS[k]) - 2), [TC.SEP]]).astype(np.int32) for k in rng.integers(0, len(LENGTHS), size=n)]


def kernel_alone(launches):
    ds = DT.DeviceTokenDataset(rows(64, 100), None, DEV, max_length=L)
    src = np.random.Generator(np.random.PCG64(1)).integers(0, len(ds), size=B)
    r = torch.from_numpy(src).to(DEV)
    n = ds.row_len_host[src]
    print("srhip_token_view alone, B = %d, L = %d, tokens per row %s" % (B, L, n.tolist()))
    ids, kl = torch.empty(B, L, dtype=torch.int64, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
    a = (ops._p(ds.store), ops._p(ds.row_off), ops._p(ds.row_len), len(ds.row_len_host), ops._p(r), B, L, 0, ops._p(ids), L, ops._p(kl), ops._s())
    t = per_launch(lambda: ops._call("srhip_token_view", *a), launches)
    print("  the entry, outputs preallocated    %8.2f us per launch (HIP events around %d back-to-back launches); a view reads %.1f KB and writes %.1f KB"
          % (t, launches, 4e-3 * n.sum(), 8e-3 * B * L))
    t = per_launch(lambda: ops.token_view(ds.store, ds.row_off, ds.row_len, r, L), launches)
    print("  ops.token_view (+ two torch.empty) %8.2f us per launch" % t)


def loader_host_time(epochs):
    lb, ulb = rows(100, 200), rows(512, 400)
    rng = np.random.Generator(np.random.PCG64(2))
    var = [[r[:max(2, int(len(r) * f))].copy() for r in ulb] for f in (0.75, 1.0)]
    dl = DT.DeviceTokenDataset(lb, rng.integers(0, 2, size=len(lb)), DEV, max_length=L)
    du = DT.DeviceTokenDataset(ulb, None, DEV, data_s=var, max_length=L)
    steps = 32
    ld_l = DT.TokenTrainLoader(dl, B, EpochSampler(len(dl), steps * B, 1, 0), keys=("idx_lb", "x_lb", "y_lb"), seed=(0, 0, 0))
    ld_u = DT.TokenTrainLoader(du, B, EpochSampler(len(du), steps * B, 1, 0), keys=("idx_ulb", "x_ulb_w", "x_ulb_s"), seed=(0, 0, 1))
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
    print("train loaders, host time (no device synchronise inside the window), batch %d labelled + %d unlabelled, three views per step, each padded to "
          "its own longest row (of %s)" % (B, B, LENGTHS))
    print("  per step             median %8.1f us   p10 %8.1f   p90 %8.1f   (n = %d; three launches, no host-to-device copy)" % (
        np.median(rest), np.percentile(rest, 10), np.percentile(rest, 90), len(rest)))
    print("  first step of an epoch  median %8.1f us   (the epoch's draws, its table and ONE copy per loader, + the step)" % (np.median(first) * 1e6))
    return lb, ulb, var


def replaced_paths(lb, ulb, var, steps=32):
    rng = np.random.Generator(np.random.PCG64(3))
    picks = [(rng.integers(0, len(lb), size=B), rng.integers(0, len(ulb), size=B), t % 2) for t in range(steps + 2)]
    lists = [[[lb[i].tolist() for i in il], [ulb[i].tolist() for i in iu], [var[v][i].tolist() for i in iu]] for il, iu, v in picks]
    padded = None
    try:
        from transformers import BertTokenizerFast
        with tempfile.TemporaryDirectory() as d:
            tok = BertTokenizerFast.from_pretrained(TC.write_vocab_dir(d), local_files_only=True)      # pad() needs the pad id and side only
        ts, padded = [], []
        for views in lists:
            t0 = time.perf_counter()
            out = [tok.pad([{"input_ids": r} for r in v], padding=True, max_length=None, return_tensors="pt") for v in views]
            ts.append(time.perf_counter() - t0)
            padded.append([{"input_ids": o["input_ids"], "attention_mask": o["attention_mask"]} for o in out])
        ts = np.array(ts[2:]) * 1e6
        print("tokenizer.pad on the already-tokenised lists on this box's CPU (the collator WITHOUT its per-step tokenisation of every sentence; main "
              "process, the same three views)")
        print("  per step             median %8.1f us   p10 %8.1f   p90 %8.1f   (n = %d)" % (np.median(ts), np.percentile(ts, 10), np.percentile(ts, 90), len(ts)))
    except Exception as e:      # noqa: BLE001
        print("tokenizer.pad on the CPU: not measured (transformers not usable here: %s)" % type(e).__name__)
    if padded is None:                                        # the same padded host tensors from numpy
        padded = []
        for views in lists:
            step = []
            for v in views:
                ids, mask = TC.padded_batch([np.asarray(r) for r in v], range(len(v)))
                step.append({"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(mask)})
            padded.append(step)
    ts, dev = [], []
    for step in padded:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for x in step:
            TokenBatch.from_dict(x, DEV)
        e1.record()
        ts.append(time.perf_counter() - t0)
        e1.synchronize()
        dev.append(e0.elapsed_time(e1) * 1e3)
    ts, dev = np.array(ts[2:]) * 1e6, np.array(dev[2:])
    print("TokenBatch.from_dict of the padded host tensors (pageable memory: two copies to the device per view, the cast, srhip_mask_lengths), the same three views")
    print("  per step, host       median %8.1f us   p10 %8.1f   p90 %8.1f   (n = %d)" % (np.median(ts), np.percentile(ts, 10), np.percentile(ts, 90), len(ts)))
    print("  per step, events     median %8.1f us   p10 %8.1f   p90 %8.1f   (first copy issued to last launch finished)" % (
        np.median(dev), np.percentile(dev, 10), np.percentile(dev, 90)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--epochs", type=int, default=4)
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    print("device_tokens; %s (%s, %d CUs), torch %s" % (torch.cuda.get_device_name(0), p.gcnArchName, p.multi_processor_count, torch.__version__))
    kernel_alone(a.launches)
    lb, ulb, var = loader_host_time(a.epochs)
    replaced_paths(lb, ulb, var)


if __name__ == "__main__":
    main()
