#!/usr/bin/env python
"""What ``device_tokens_strong: True`` costs (semireward_amd/data/device_tokens.py, csrc/token_strong.hip), on one GPU:

  (a) srhip_token_strong alone at B = 8 rows of 512 and of 64 tokens, per op pair class (copy only, delete + delete, swap + mask, and the
      other two ops) at the default rate, beside srhip_token_view on the same rows in the same process: HIP events around ``--launches``
      back-to-back launches on preallocated outputs, us per launch (execution + dispatch), median of 5 windows after one warm-up window;
  (b) the train loaders' HOST time per step for the three views (x_lb, x_ulb_w, x_ulb_s) with the key and with ``data_s``: time.perf_counter
      around ``next()`` of both loaders without a device synchronise, and the first step of an epoch (the draws, the table, its one copy);
  (c) the SRSoftMatch step on the tiny BERT and on BERT-base fed by the key's loader against a ``data_s`` loader over the same sentences: ONE
      algorithm object, interleaved rounds, wall ms per step with a synchronise at the end of a round, medians and the spread between the
      rounds of one setting.  The rounds replay an epoch that was run once before (the loaders replay their draws), so every shape has met
      the BERT engine: the key's strong view meets more padded lengths than ``data_s`` (when profiles/token_strong.txt was taken the
      engine kept one workspace set per distinct (B, L); its arenas are sized by the largest batch now), and the first pass is reported on
      its own line;
  (d) ``--bench-lines FILE``: lines "this {json}" / "parent {json}" of alternating ``bench.py --gpus 1`` runs of this tree and of the parent
      commit's tree on the same box -> the ratio of medians beside the parent's own run-to-run spread.

Nothing here is a pass / fail number.

    python tools/token_strong_time.py > profiles/token_strong.txt
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
import _token_strong_cases as TS                              # noqa: E402
from semireward_amd import ops                               # noqa: E402
from semireward_amd.data import device_tokens as DT          # noqa: E402
from semireward_amd.data.device_loader import EpochSampler   # noqa: E402

DEV = "cuda:0"
B, RATE = 8, DT.STRONG_RATE
ULB_KEYS = ("idx_ulb", "x_ulb_w", "x_ulb_s")


def windows(f, launches):
    ts = []
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            f()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / launches)
    return ts[1:]


def rows(n, lengths, vocab, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [np.concatenate([[TS.CLS], rng.integers(5, vocab, size=int(lengths[k]) - 2), [TS.SEP]]).astype(np.int32) for k in rng.integers(0, len(lengths), size=n)]


def kernel_alone(launches):
    print("(a) srhip_token_strong alone beside srhip_token_view, B = %d, outputs preallocated, counts at rate %.1f (c = floor(rate * ni)); us per launch, "
          "median (min .. max) of 5 windows of %d back-to-back launches" % (B, RATE, launches))
    for n in (512, 64):
        ds = DT.DeviceTokenDataset(rows(B, (n,), 30522, 100 + n), None, DEV, max_length=n)
        r = torch.arange(B, dtype=torch.int64, device=DEV)
        ids, kl = torch.empty(B, n, dtype=torch.int64, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
        head = (ops._p(ds.store), ops._p(ds.row_off), ops._p(ds.row_len), B, ops._p(r))
        tail = (ops._p(ids), n, ops._p(kl), ops._s())
        ts = windows(lambda: ops._call("srhip_token_view", *head, B, n, 0, *tail), launches)
        print("  %d x %3d  %-22s %7.2f  (%.2f .. %.2f)" % (B, n, "srhip_token_view", np.median(ts), min(ts), max(ts)))
        c0 = int(RATE * (n - 2))
        for name, (op0, op1) in (("copy + copy", (TS.COPY, TS.COPY)), ("delete + delete", (TS.DELETE, TS.DELETE)), ("swap + mask", (TS.SWAP, TS.MASK)),
                                 ("cutoff + cutoff", (TS.CUTOFF, TS.CUTOFF)), ("mask + delete", (TS.MASK, TS.DELETE))):
            n1 = int(ops.token_strong_len(n, op0, c0))
            s0 = ops.pack_token_slot(np.full(B, op0), np.full(B, c0 if op0 else 0), np.arange(B) + 17)
            s1 = ops.pack_token_slot(np.full(B, op1), np.full(B, int(RATE * (n1 - 2)) if op1 else 0), np.arange(B) + 99)
            d0, d1 = torch.from_numpy(s0).to(DEV), torch.from_numpy(s1).to(DEV)
            ops.check_token_strong(np.arange(B), np.stack([s0, s1]), n, ds.row_len_host, n)
            ts = windows(lambda: ops._call("srhip_token_strong", *head, ops._p(d0), ops._p(d1), B, n, n, 0, 103, *tail), launches)
            print("  %d x %3d  %-22s %7.2f  (%.2f .. %.2f)" % (B, n, name, np.median(ts), min(ts), max(ts)))


def loaders(steps, lengths, vocab, max_length, mask_id=103):
    """(labelled loader, unlabelled loader with data_s, unlabelled loader with the key) over the same sentences."""
    lb, ulb = rows(100, lengths, vocab, 200), rows(512, lengths, vocab, 400)
    rng = np.random.Generator(np.random.PCG64(2))
    var = [[r[:max(2, int(len(r) * f))].copy() for r in ulb] for f in (0.75, 1.0)]
    dl = DT.DeviceTokenDataset(lb, rng.integers(0, 2, size=len(lb)), DEV, max_length=max_length)
    du_s, du = DT.DeviceTokenDataset(ulb, None, DEV, data_s=var, max_length=max_length), DT.DeviceTokenDataset(ulb, None, DEV, max_length=max_length)
    ld_l = DT.TokenTrainLoader(dl, B, EpochSampler(len(dl), steps * B, 1, 0), keys=("idx_lb", "x_lb", "y_lb"), seed=(0, 0, 0))
    ld_s = DT.TokenTrainLoader(du_s, B, EpochSampler(len(du_s), steps * B, 1, 0), keys=ULB_KEYS, seed=(0, 0, 1))
    ld_k = DT.TokenTrainLoader(du, B, EpochSampler(len(du), steps * B, 1, 0), keys=ULB_KEYS, seed=(0, 0, 1), device_strong=True, mask_id=mask_id)
    return ld_l, ld_s, ld_k


def loader_host_time(epochs, steps=32):
    lengths = (128, 256, 384, 512)
    ld_l, ld_s, ld_k = loaders(steps, lengths, 30522, 512)
    print("(b) train loaders, host time (no device synchronise inside the window), batch %d labelled + %d unlabelled, three views per step, each padded "
          "to its own longest row (sentences of %s tokens)" % (B, B, lengths))
    for name, ld_u in (("data_s", ld_s), ("key", ld_k)):
        first, rest = [], []
        for e in range(epochs + 1):
            ld_l.set_epoch(e), ld_u.set_epoch(e)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            it_l, it_u = iter(ld_l), iter(ld_u)
            next(it_l), next(it_u)
            t1 = time.perf_counter()
            ts = []
            for _ in range(steps - 1):
                t2 = time.perf_counter()
                next(it_l), next(it_u)
                ts.append(time.perf_counter() - t2)
            torch.cuda.synchronize()
            if e:                                                 # (epoch 0: first launches, allocator warm-up)
                first.append(t1 - t0)
                rest += ts
        rest = np.array(rest) * 1e6
        print("  %-6s  per step median %7.1f us  p10 %7.1f  p90 %7.1f  (n = %d; three launches, no copy)   first step of an epoch median %7.1f us "
              "(the draws, the table, ONE copy per loader)" % (name, np.median(rest), np.percentile(rest, 10), np.percentile(rest, 90), len(rest),
                                                              np.median(first) * 1e6))


def step_ab(which_net, n, rounds):
    from semireward_amd.algorithms import get_algorithm
    from semireward_amd.nets import bert
    net = dict(tiny=dict(builder=bert.bert_tiny_test, vocab=120, lengths=(16, 32, 48, 64), feature_dim=128, lr=5e-4, mask_id=4),
               base=dict(builder=bert.bert_base_uncased, vocab=30522, lengths=(128, 256, 384, 512), feature_dim=768, lr=5e-5, mask_id=103))[which_net]
    total, L = n * rounds, max(net["lengths"])
    ld_l, ld_s, ld_k = loaders(total, net["lengths"], net["vocab"], L, net["mask_id"])
    dd = {"train_lb": ld_l.dataset, "train_ulb": ld_k.dataset}
    args = argparse.Namespace(
        algorithm="srsoftmatch", num_classes=2, num_train_iter=1024, epoch=1, ema_m=0.0, ulb_loss_ratio=1.0, use_cat=False, amp=False, lr=net["lr"],
        weight_decay=5e-4, layer_decay=0.75, num_warmup_iter=0, optim="AdamW", T=0.5, hard_label=True, N_k=10, start_timing=0, feature_dim=net["feature_dim"],
        sr_lr=5e-4, sr_ema=False, sr_ema_m=0.99, gpu=0, rank=0, world_size=1, distributed=False, seed=0, dataset="synthetic_tokens", max_length=L,
        batch_size=B, uratio=1, eval_batch_size=B, train_sampler="RandomSampler", device_tokens=True, device_tokens_strong=True,
        device_tokens_mask_id=net["mask_id"], dataset_dict=dd, dist_align=True, dist_uniform=True, per_class=False, ema_p=0.999, n_sigma=2)
    m = get_algorithm(args, net["builder"])
    m.it = 100
    m.model.train()
    print("(c) srsoftmatch step on %s (K = %d), batch %d / %d, sentences of %s tokens, fed by the loaders; ONE object, unlabelled batches from the "
          "key's loader against data_s, interleaved rounds" % (net["builder"].__name__, m.sr_decay(), B, B, net["lengths"]))

    def steps(il, iu, k):
        for _ in range(k):
            a, b = next(il), next(iu)
            m.out_dict, m.log_dict = m.train_step(**m.process_batch(x_lb=a["x_lb"], y_lb=a["y_lb"], x_ulb_w=b["x_ulb_w"], x_ulb_s=b["x_ulb_s"]))
            m.call_hook("after_train_step")
            m.it += 1
    its, lens = {}, {}
    for which, ld in (("data_s", ld_s), ("key", ld_k)):       # the first pass: every (B, L) of the epoch meets the engine once
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps(iter(ld_l), iter(ld), total)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        lens[which] = sorted(set(ld.draws["x_ulb_s"][1].tolist()))
        print("  first pass, %-6s %8.3f ms per step over %d steps (workspaces of new (B, L) allocated on the way); the strong view met %d distinct "
              "padded lengths (%d .. %d)" % (which, 1e3 * dt / total, total, len(lens[which]), lens[which][0], lens[which][-1]))
        its[which] = (iter(ld_l), iter(ld))                   # the same epoch again: the loaders replay their draws
    wall, host = {"data_s": [], "key": []}, {"data_s": [], "key": []}
    for _ in range(rounds):
        for which in wall:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(*its[which], n)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            wall[which].append(1e3 * (t2 - t0) / n)
            host[which].append(1e3 * (t1 - t0) / n)
    assert np.isfinite(float(m.log_dict["train/total_loss"]))
    print("  replayed epoch, %d rounds of %d steps per setting, ms per step (the loaders' launches and the host work of next() included)" % (rounds, n))
    for which in wall:
        w, h = np.array(wall[which]), np.array(host[which])
        print("    %-6s  wall median %.3f  min %.3f  max %.3f   host enqueue median %.3f   rounds: %s" % (
            which, np.median(w), w.min(), w.max(), np.median(h), " ".join("%.3f" % v for v in w)))
    d = np.median(wall["key"]) - np.median(wall["data_s"])
    over = min(wall["key"]) <= max(wall["data_s"]) and min(wall["data_s"]) <= max(wall["key"])
    print("    key - data_s: wall %+.1f us per step (%+.2f %%); spread (max - min) of the data_s rounds %.1f us, of the key rounds %.1f us; the rounds of "
          "the two settings %s.  (The two settings do not do equal work: the key's rows are up to two deletions shorter, a data_s row is the sentence "
          "or its first three quarters.)" % (1e3 * d, 100 * d / np.median(wall["data_s"]), 1e3 * (max(wall["data_s"]) - min(wall["data_s"])),
                                             1e3 * (max(wall["key"]) - min(wall["key"])), "overlap" if over else "do not overlap"))
    print("    device memory: %.2f GB allocated, %.2f GB reserved at the end" % (torch.cuda.memory_allocated() / 2 ** 30, torch.cuda.memory_reserved() / 2 ** 30))


def bench_lines(path):
    import json
    vals = {"this": [], "parent": []}
    for ln in open(path):
        label, _, js = ln.strip().partition(" ")
        try:
            d = json.loads(js)
        except ValueError:
            continue
        if label in vals and "value" in d:
            vals[label].append(float(d["value"]))
    print("(d) bench.py --gpus 1 (the key is never set), this tree against the parent commit's tree, alternating runs on the same box")
    for label in ("parent", "this"):
        v = np.array(vals[label])
        if v.size:
            print("    %-6s  runs: %s   median %.1f   spread (max - min) %.1f = %.2f %%" % (
                label, " ".join("%.1f" % x for x in v), np.median(v), v.max() - v.min(), 100 * (v.max() - v.min()) / np.median(v)))
    if vals["this"] and vals["parent"]:
        print("    this / parent (medians): %.4f" % (np.median(vals["this"]) / np.median(vals["parent"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--nets", default="tiny,base", help="the nets of (c), comma separated; '' skips the steps")
    ap.add_argument("--bench-lines", default="")
    ap.add_argument("--only-bench-lines", action="store_true", help="print (d) alone (appended to the file by the caller once the runs are done)")
    a = ap.parse_args()
    if a.only_bench_lines:
        return bench_lines(a.bench_lines)
    p = torch.cuda.get_device_properties(0)
    print("device_tokens_strong; %s (%s, %d CUs), torch %s" % (torch.cuda.get_device_name(0), p.gcnArchName, p.multi_processor_count, torch.__version__))
    kernel_alone(a.launches)
    loader_host_time(a.epochs)
    for which in [w for w in a.nets.split(",") if w]:
        try:
            step_ab(which, a.steps, a.rounds)
        except torch.OutOfMemoryError as e:
            print("(c) %s: not measured, the device ran out of memory (%s)" % (which, str(e).splitlines()[0]))
        sys.stdout.flush()
    if a.bench_lines:
        bench_lines(a.bench_lines)


if __name__ == "__main__":
    main()
