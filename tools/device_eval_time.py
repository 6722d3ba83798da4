#!/usr/bin/env python
"""Wall time and launch count of ``alg.evaluate("eval")`` with and without ``device_eval: True`` (csrc/eval.hip), on the same weights in one
process: ViT-S/2@32 with 100 classes over 2048 evaluation images at eval_batch_size 16 (the usb_cv yamls' value) and 128, and BERT-base with
2 classes (configs/usb_nlp_srsoftmatch_aclImdb_20_bert_base.yaml) over 512 sequences of 128 tokens at batch 16.  The batches are resident on
the device, so the time is the forward plus the evaluation tail.  time.perf_counter around the call (it ends with the copy to the host,
which waits for the device); median of ``--runs`` calls after ``--warmup``.  Launches: entries of libsrhip called (ops._call) and aten
operators dispatched, per evaluate().  ``--step-ms``: the training step time of the same box (bench.py), for evaluation's share of a
num_eval_iter = 2048 window.

    python tools/device_eval_time.py --step-ms 4.9 > profiles/device_eval.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semireward_amd import config as srconfig                # noqa: E402
from semireward_amd import ops                               # noqa: E402
from semireward_amd.algorithms import get_algorithm          # noqa: E402
from semireward_amd.nets import bert, vit                    # noqa: E402

DEV = "cuda:0"


class _CountAten(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def count(alg, loader):
    real, n = ops._call, [0]

    def counting(name, *a):
        n[0] += 1
        return real(name, *a)
    ops._call = counting
    try:
        with _CountAten() as c:
            alg.evaluate("eval", loader=loader)
    finally:
        ops._call = real
    return n[0], c.n


def timed(alg, loader, runs, warm):
    for _ in range(warm):
        alg.evaluate("eval", loader=loader)
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        alg.evaluate("eval", loader=loader)
        ts.append(time.perf_counter() - t0)
    return np.array(ts) * 1e3


def measure(name, alg, loader, n_batches, a, step_ms):
    alg.print_fn = lambda s: None
    res = {}
    out = {}
    for flag in (False, True, False, True):                   # interleaved: off, on, off, on
        alg.device_eval = flag
        res.setdefault(flag, []).append(timed(alg, loader, a.runs, a.warmup))
        out[flag] = alg.evaluate("eval", loader=loader)
    same = all(out[False][k] == out[True][k] for k in out[False] if k != "eval/loss")
    print(name)
    for flag in (False, True):
        alg.device_eval = flag
        ts = np.concatenate(res[flag])
        lib, aten = count(alg, loader)
        line = "  device_eval %-5s  median %8.3f ms   p10 %8.3f   p90 %8.3f   (n = %d)   libsrhip entries %5d  aten ops %5d  per evaluate(), %d batches" % (
            flag, np.median(ts), np.percentile(ts, 10), np.percentile(ts, 90), len(ts), lib, aten, n_batches)
        if step_ms:
            line += "   share of a 2048-step window at %.2f ms / step: %.3f %%" % (step_ms, 100 * np.median(ts) / (2048 * step_ms + np.median(ts)))
        print(line)
    print("  metrics equal: %s   eval/loss off %.9g on %.9g" % (same, out[False]["eval/loss"], out[True]["eval/loss"]))


def kernel_alone(launches=200):
    """HIP-event time per launch of srhip_eval_accumulate beside srhip_masked_ce (the launch it replaces; its torch companions not counted)."""
    print("launch alone, us per launch (HIP events around %d back-to-back launches, median of 5 after 1)" % launches)
    g = torch.Generator(device=DEV).manual_seed(0)

    def per_launch(f):
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
    for B, C, same in ((16, 100, False), (128, 100, False), (1024, 100, False), (16, 2, False), (128, 2, False), (128, 2, True), (128, 1000, False)):
        z = 3.0 * torch.randn(B, C, device=DEV, generator=g)
        y = torch.zeros(B, dtype=torch.int64, device=DEV) if same else torch.randint(0, C, (B,), device=DEV, generator=g)
        if same:
            z[:, 0] = 50.0                                    # every row counts in ONE confusion cell
        _, state, confusion = ops.eval_accumulator(C, DEV)
        loss, dl, w = torch.empty(1, device=DEV), torch.empty(B, C, device=DEV), torch.ones(B, device=DEV)
        t_new = per_launch(lambda: ops.eval_accumulate(z, y, confusion, state))
        t_old = per_launch(lambda: ops.masked_ce(z, y, w, None, 1.0, loss, dl, B, C))
        print("  B = %4d  C = %4d%s   eval_accumulate %7.2f us   masked_ce %7.2f us" % (B, C, "  (one hot cell)" if same else "", t_new, t_old))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-ms", type=float, default=0.0)
    ap.add_argument("--skip-bert", action="store_true")
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    print("evaluate('eval') wall time; %s (%s, %d CUs), torch %s" % (torch.cuda.get_device_name(0), p.gcnArchName, p.multi_processor_count,
                                                                      torch.__version__))
    rng = np.random.Generator(np.random.PCG64(0))
    C, n = 100, 2048
    mk = lambda k: rng.integers(0, 256, size=(k, 32, 32, 3)).astype(np.uint8)      # noqa: E731
    for ebs in (16, 128):
        dd = {"train_lb": {"data": mk(16), "targets": rng.integers(0, C, size=16)}, "train_ulb": {"data": mk(64), "targets": None},
              "eval": {"data": mk(n), "targets": rng.integers(0, C, size=n)}}
        args = argparse.Namespace(
            algorithm="srflexmatch", num_classes=C, num_train_iter=64, epoch=1, ema_m=0.0, ulb_loss_ratio=1.0, use_cat=True, amp=False, lr=5e-4,
            weight_decay=5e-4, layer_decay=0.5, num_warmup_iter=0, optim="AdamW", T=0.5, p_cutoff=0.95, hard_label=True, thresh_warmup=True,
            N_k=10, start_timing=20, feature_dim=384, sr_lr=5e-4, sr_ema=False, sr_ema_m=0.99, gpu=0, rank=0, world_size=1, distributed=False,
            seed=0, dataset="cifar100", img_size=32, crop_ratio=0.875, batch_size=8, uratio=1, eval_batch_size=ebs,
            train_sampler="RandomSampler", device_data=True, dataset_dict=dd)
        alg = get_algorithm(args, vit.vit_small_patch2_32)
        alg.print_fn = lambda s: None
        measure("ViT-S/2@32, %d classes, %d images, eval_batch_size %d (device loader)" % (C, n, ebs), alg, None, -(-n // ebs), a,
                a.step_ms if ebs == 16 else 0.0)
        del alg
    if a.skip_bert:
        kernel_alone()
        return
    L, nb, B = 128, 32, 16
    args = srconfig.get_config(os.path.join(ROOT, "configs", "usb_nlp_srsoftmatch_aclImdb_20_bert_base.yaml"),
                               overrides=dict(gpu=0, rank=0, world_size=1, distributed=False))
    alg = get_algorithm(args, bert.bert_base_uncased)
    g = torch.Generator().manual_seed(1)
    loader = [{"x_lb": {"input_ids": torch.randint(1, 30522, (B, L), generator=g).to(DEV),
                        "attention_mask": torch.ones(B, L, dtype=torch.int64).to(DEV)},
               "y_lb": torch.randint(0, args.num_classes, (B,), generator=g).to(DEV)} for _ in range(nb)]
    measure("BERT-base, %d classes, %d sequences of %d tokens, batch %d (hot 2 x 2 confusion cells)" % (args.num_classes, nb * B, L, B), alg,
            loader, nb, a, 0.0)
    del alg
    kernel_alone()


if __name__ == "__main__":
    main()
