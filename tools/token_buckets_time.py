#!/usr/bin/env python
"""What the token engine's arenas, the srhip_token_cat launch and ``token_len_bucket`` cost and save, on one GPU.  Every part runs in ONE tree
(``--tree DIR``: import the package from another checkout, e.g. the parent commit built beside this one) and prints labelled lines; parts that
compare two trees are run alternately, tree by tree, on the same box, and their lines collected into profiles/token_buckets.txt.

  memory   (a) ``torch.cuda.memory_allocated()`` while 200 BERT-base SRSoftMatch steps run over a replayed epoch of rows of every length
           2 .. 512 (what ``examples/train_device_tokens.py --lengths free`` makes; 100 steps, run twice), every 20 steps; an out-of-memory error ends the part and
           the step at which it struck is printed.
  step     (b) the BERT-base SRSoftMatch step on three views of ONE padded length (512: the bench shape, TokenBatch.cat's equal-length path;
           and 64), wall ms per step, ``--rounds`` rounds of ``--n`` steps with a synchronise at the end of a round.
  cat      (c) joining three views of 8 rows (24 x 512 and 24 x 64 ids out; the views 3/4, 7/8 and 1/1 of that length): ``TokenBatch.cat`` as the
           tree has it, and -- where the tree has it -- the srhip_token_cat launch on preallocated outputs; HIP events around ``--launches``
           back-to-back calls, us per call, median of 5 windows after one warm-up window.
  buckets  (d) the step over the replayed free-length epoch with ``token_len_bucket`` absent, 16, 32 and 64: one algorithm object per setting
           in one process, interleaved rounds, wall ms per step.
  (e) is ``python bench.py --gpus 1 --net bert`` of both trees, alternating; ``--bench-lines FILE`` summarises lines "this {json}" / "parent {json}".

Nothing here is a pass / fail number.
"""
import argparse
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("part", choices=["memory", "step", "cat", "buckets", "bench-lines"])
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this")
ap.add_argument("--net", choices=["base", "tiny"], default="base")
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--n", type=int, default=10)
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--file", default=None)
A = ap.parse_args()
sys.path.insert(0, A.tree)
import torch                                                  # noqa: E402

DEV, B = "cuda:0", 8
CLS, SEP = 2, 3


def free_rows(n, vocab, max_length, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [np.concatenate([[CLS], rng.integers(5, vocab, size=int(m) - 2), [SEP]]).astype(np.int32)[:int(m)] for m in rng.integers(2, max_length + 1, size=n)]


def algorithm(total, bucket=None, strong_rows=None):
    from semireward_amd.algorithms import get_algorithm
    from semireward_amd.nets import bert
    net = dict(tiny=dict(builder=bert.bert_tiny_test, vocab=120, L=64, feature_dim=128, lr=5e-4),
               base=dict(builder=bert.bert_base_uncased, vocab=30522, L=512, feature_dim=768, lr=5e-5))[A.net]
    lb, ulb = free_rows(100, net["vocab"], net["L"], 200), free_rows(512, net["vocab"], net["L"], 400)
    var = [free_rows(512, net["vocab"], net["L"], 600 + v) for v in (0, 1)]
    rng = np.random.Generator(np.random.PCG64(2))
    dd = {"train_lb": {"data": lb, "targets": rng.integers(0, 2, size=len(lb))}, "train_ulb": {"data": ulb, "targets": None, "data_s": var}}
    kw = {} if bucket is None else dict(token_len_bucket=bucket)
    args = argparse.Namespace(
        algorithm="srsoftmatch", num_classes=2, num_train_iter=total, epoch=1, ema_m=0.0, ulb_loss_ratio=1.0, use_cat=False, amp=False, lr=net["lr"],
        weight_decay=5e-4, layer_decay=0.75, num_warmup_iter=0, optim="AdamW", T=0.5, hard_label=True, N_k=10, start_timing=0,
        feature_dim=net["feature_dim"], sr_lr=5e-4, sr_ema=False, sr_ema_m=0.99, gpu=0, rank=0, world_size=1, distributed=False, seed=0,
        dataset="synthetic_tokens", max_length=net["L"], batch_size=B, uratio=1, eval_batch_size=B, train_sampler="RandomSampler", device_tokens=True,
        dataset_dict=dd, dist_align=True, dist_uniform=True, per_class=False, ema_p=0.999, n_sigma=2, **kw)
    m = get_algorithm(args, net["builder"])
    m.it = 100
    m.num_train_iter = 1                                      # sr_decay() = max(8, 1 + num_train_iter / it): K = 8 at every step, bench.py's regime
    m.model.train()
    return m, net


def run_steps(m, batches, k):
    for _ in range(k):
        a, b = next(batches)
        m.out_dict, m.log_dict = m.train_step(**m.process_batch(x_lb=a["x_lb"], y_lb=a["y_lb"], x_ulb_w=b["x_ulb_w"], x_ulb_s=b["x_ulb_s"]))
        m.call_hook("after_train_step")
        m.it += 1


def epoch_forever(m):
    while True:                                               # the loaders replay their draws: the same epoch again and again
        for a, b in zip(m.loader_dict["train_lb"], m.loader_dict["train_ulb"]):
            yield a, b


def part_memory():
    m, net = algorithm(A.steps // 2)                          # an epoch of steps / 2 batches, run twice
    print("(a) %s: %s srsoftmatch (K = %d), batch %d + %d + %d, rows of every length 2 .. %d, %d steps; memory_allocated after a synchronise"
          % (A.label, net["builder"].__name__, m.sr_decay(), B, B, B, net["L"], A.steps), flush=True)
    it, lengths, done = epoch_forever(m), set(), 0
    torch.cuda.synchronize()
    print("    %-6s before the first step: %.2f GB" % (A.label, torch.cuda.memory_allocated() / 2 ** 30), flush=True)
    try:
        while done < A.steps:
            run_steps(m, it, 20)
            done += 20
            torch.cuda.synchronize()
            print("    %-6s after %3d steps: %7.2f GB allocated, %7.2f GB reserved" % (A.label, done, torch.cuda.memory_allocated() / 2 ** 30,
                                                                                         torch.cuda.memory_reserved() / 2 ** 30), flush=True)
    except torch.cuda.OutOfMemoryError as e:
        print("    %-6s OUT OF MEMORY between step %d and %d: %s" % (A.label, done, done + 20, str(e).splitlines()[0][:160]), flush=True)
        return
    for k in ("x_lb", "x_ulb_w", "x_ulb_s"):
        ld = m.loader_dict["train_lb" if k == "x_lb" else "train_ulb"]
        lengths |= set(ld.draws[k][1].tolist())
    print("    %-6s distinct padded lengths of the views in the epoch: %d; arena allocations: %s" % (
        A.label, len(lengths), getattr(m.model, "arena_allocations", "n/a (one buffer set per (B, L))")), flush=True)


def part_step():
    from semireward_amd.nets.bert import TokenBatch
    m, net = algorithm(64)
    g = torch.Generator().manual_seed(1)
    print("(b) %s: %s srsoftmatch step (K = %d) on three views of ONE padded length, 24 sequences; %d rounds of %d steps, wall ms per step"
          % (A.label, net["builder"].__name__, m.sr_decay(), A.rounds, A.n), flush=True)
    for L in ((512, 64) if A.net == "base" else (64, 16)):
        def view():
            return TokenBatch(torch.randint(5, net["vocab"], (B, L), generator=g).to(DEV), torch.full((B,), L, dtype=torch.int32, device=DEV))
        y = torch.randint(0, 2, (B,), generator=g).to(DEV)
        batch = ({"x_lb": view(), "y_lb": y}, {"x_ulb_w": view(), "x_ulb_s": view()})
        same = iter(lambda: batch, None)
        run_steps(m, same, 12)                                # workspaces, plans and the deferred-row tuner settle
        ws = []
        for _ in range(A.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_steps(m, same, A.n)
            torch.cuda.synchronize()
            ws.append(1e3 * (time.perf_counter() - t0) / A.n)
        print("    %-6s 24 x %3d  median %.3f  min %.3f  max %.3f   rounds: %s" % (A.label, L, np.median(ws), min(ws), max(ws), " ".join("%.3f" % w for w in ws)),
              flush=True)


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


def part_cat():
    from semireward_amd import ops
    from semireward_amd.nets.bert import TokenBatch
    g = torch.Generator().manual_seed(1)
    print("(c) %s: three views of 8 rows joined into 24 x L ids; us per call (execution + dispatch + what the call allocates), median (min .. max) of 5 windows "
          "of %d back-to-back calls" % (A.label, A.launches), flush=True)
    for L in (512, 64):
        views = [TokenBatch(torch.randint(5, 30000, (B, l), generator=g).to(DEV), torch.full((B,), l, dtype=torch.int32, device=DEV))
                 for l in (3 * L // 4, 7 * L // 8, L)]
        ts = windows(lambda: TokenBatch.cat(views), A.launches)
        print("    %-6s 24 x %3d  TokenBatch.cat (allocating)       %7.2f  (%.2f .. %.2f)" % (A.label, L, np.median(ts), min(ts), max(ts)), flush=True)
        if hasattr(ops, "token_cat"):
            from semireward_amd.nets.bert import TokenCatBuffer
            buf = TokenCatBuffer(DEV)
            ts = windows(lambda: TokenBatch.cat(views, out=buf), A.launches)
            print("    %-6s 24 x %3d  TokenBatch.cat into the buffer    %7.2f  (%.2f .. %.2f)" % (A.label, L, np.median(ts), min(ts), max(ts)), flush=True)
            src, out = [(v.ids, v.key_len, None) for v in views], buf.take(24, L)
            ts = windows(lambda: ops.token_cat(src, L, 0, out=out), A.launches)
            print("    %-6s 24 x %3d  ops.token_cat, outputs passed in  %7.2f  (%.2f .. %.2f)" % (A.label, L, np.median(ts), min(ts), max(ts)), flush=True)


def part_buckets():
    settings = (None, 16, 32, 64)
    algs = {}
    for bk in settings:
        m, net = algorithm(64, bucket=bk)                     # an epoch of 64 steps, replayed
        it = epoch_forever(m)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_steps(m, it, 64)                                  # the first pass: every shape of the epoch meets the engine once
        torch.cuda.synchronize()
        algs[bk] = (m, it)
        print("(d) token_len_bucket %-4s first pass %.3f ms per step over 64 steps" % (bk, 1e3 * (time.perf_counter() - t0) / 64), flush=True)
    print("(d) %s srsoftmatch step over the replayed free-length epoch (rows of 2 .. %d tokens, 64 steps), one object per setting, %d interleaved "
          "rounds of 64 steps, wall ms per step" % (net["builder"].__name__, net["L"], A.rounds), flush=True)
    wall = {bk: [] for bk in settings}
    for _ in range(A.rounds):
        for bk in settings:
            m, it = algs[bk]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_steps(m, it, 64)
            torch.cuda.synchronize()
            wall[bk].append(1e3 * (time.perf_counter() - t0) / 64)
    for bk in settings:
        w = wall[bk]
        shapes = len({(k, v) for k in ("x_lb", "x_ulb_w", "x_ulb_s") for v in algs[bk][0].loader_dict["train_lb" if k == "x_lb" else "train_ulb"].draws[k][1].tolist()})
        print("    bucket %-4s median %.3f  min %.3f  max %.3f   rounds: %s   (view lengths before bucketing: %d distinct)"
              % (bk, np.median(w), min(w), max(w), " ".join("%.3f" % v for v in w), shapes), flush=True)
    print("    device memory with the four objects alive: %.2f GB allocated" % (torch.cuda.memory_allocated() / 2 ** 30), flush=True)


def part_bench_lines():
    import json
    vals = {"this": [], "parent": []}
    for ln in open(A.file):
        label, _, js = ln.strip().partition(" ")
        try:
            d = json.loads(js)
        except ValueError:
            continue
        if label in vals and "value" in d:
            vals[label].append(float(d["value"]))
    print("(e) bench.py --gpus 1 --net bert (three views of 512 tokens: the equal-length path), this tree against the parent commit's tree, alternating runs")
    for label in ("parent", "this"):
        v = np.array(vals[label])
        if v.size:
            print("    %-6s  runs: %s   median %.2f   spread (max - min) %.2f = %.2f %%" % (
                label, " ".join("%.2f" % x for x in v), np.median(v), v.max() - v.min(), 100 * (v.max() - v.min()) / np.median(v)))
    if vals["this"] and vals["parent"]:
        print("    this / parent (medians): %.4f" % (np.median(vals["this"]) / np.median(vals["parent"])))


{"memory": part_memory, "step": part_step, "cat": part_cat, "buckets": part_buckets, "bench-lines": part_bench_lines}[A.part]()
