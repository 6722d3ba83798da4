#!/usr/bin/env python
"""What the opt-in reward filter (``reward_filter: topk``, csrc/score_filter.hip: reward_topk_kernel) costs, on one GPU:

  (a) srhip_reward_topk_mask and srhip_reward_mask2 alone: HIP events around back-to-back launches, (groups, B) = (8, 8), (8, 64), (8, 448)
      and (8, 4096), top-k with no peer table and with a synthetic table of 8 peers (B * 8 <= 65536); beside them the Rewarder's scoring
      launch of 8 groups of 448 rows, the launch the filter follows in a step;
  (b) the headline SRFlexMatch step of bench.py (ViT-S/2@32, 8 / 8 / 8, K = 8) with ``reward_filter: topk`` against the same object with the
      filter taken away (its ``reward_filter`` replaced by the mean rule an object without the key has), rounds interleaved mean / topk / ...;
      per round the wall time of ``--steps`` steps between two device fences and the host time to enqueue a step;
  (c) (optional, ``--bench-lines FILE``) bench.py result lines of this tree (key absent) and of the parent commit's tree, run alternately on
      the same box by the caller: one "<label> <json>" per line, label = this | parent (tools/pl_monitor_time.py shows the loop).

    python tools/reward_filter_time.py [--bench-lines FILE] > profiles/reward_filter.txt
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                    # noqa: E402
from semireward_amd import ops                                 # noqa: E402
from semireward_amd.algorithms import get_algorithm            # noqa: E402
from semireward_amd.algorithms import srflexmatch as SF        # noqa: E402
from semireward_amd.algorithms.reward_filter import RewardFilter   # noqa: E402
from semireward_amd.algorithms.semireward import Rewarder, label_dim   # noqa: E402
from semireward_amd.nets import vit                            # noqa: E402
from semireward_amd.utils import synth                         # noqa: E402

DEV = "cuda:0"


def timed(fn, launches):
    ts = []
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / launches)
    return float(np.median(ts[1:])), min(ts[1:]), max(ts[1:])


def launches_alone(launches=200):
    print("(a) us per launch (HIP events around %d back-to-back launches, median of 5 after 1; min, max of the 5)" % launches)
    g = torch.Generator(device=DEV).manual_seed(0)
    res = {}
    for groups, B in ((8, 8), (8, 64), (8, 448), (8, 4096)):
        r = torch.rand(groups * B, device=DEV, generator=g)
        m = torch.empty_like(r)
        peers = torch.rand(8, groups * B, device=DEV, generator=g)
        peers[3].copy_(r)
        k = max(1, B // 4)
        rows = [("srhip_reward_mask2", lambda: ops.reward_mask2(r, m, None, groups, B)),
                ("srhip_reward_topk_mask, 1 peer", lambda: ops.reward_topk_mask(r, m, groups, B, k)),
                ("srhip_reward_topk_mask, 8 peers", lambda: ops.reward_topk_mask(r, m, groups, B, 8 * k, peers=peers, self_peer=3))]
        for name, fn in rows:
            res[(name, B)] = timed(fn, launches)
            print("  groups = %d  B = %4d  %-34s %7.2f us   (min %.2f, max %.2f)" % ((groups, B, name) + res[(name, B)]))
    F, C, groups, B = 384, 100, 8, 448
    rw = Rewarder(label_dim(C), 128, F, device=torch.device(DEV))
    feats = torch.randn(groups * B, F, device=DEV, generator=g)
    labels = torch.randint(0, C, (groups * B,), device=DEV, generator=g)
    rw.eval()
    sc = timed(lambda: rw.score(feats, labels, groups=groups), 50)
    print("  groups = %d  B = %4d  %-34s %7.2f us   (min %.2f, max %.2f)" % ((groups, B, "Rewarder.score (all its launches)") + sc))
    tk = res[("srhip_reward_topk_mask, 1 peer", 448)][0]
    print("  at (8, 448) the top-k launch takes %s than the Rewarder scoring it follows (%.2f against %.2f us)%s" % (
        "LONGER" if tk > sc[0] else "less", tk, sc[0],
        ": 448 x 448 compares per group on two workgroups per group are more work than the scoring" if tk > sc[0] else ""))
    ops.check_label_errors()


def make():
    common = dict(gpu=0, rank=0, world_size=1, distributed=False, reward_filter="topk", reward_topk=2)
    m = get_algorithm(argparse.Namespace(**common, **dict(bench.NS, algorithm="srflexmatch")), vit.vit_small_patch2_32)
    m.model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_params(m.model.names_shapes, 0).items()})
    b = synth.synth_batch(100, 8, 8, 32, 100, 50000)
    batch = m.process_batch(**{k: torch.from_numpy(v) for k, v in b.items()})
    m.model.seed = 1234
    m.defer_share = SF._DEFER_SEED                                # one fixed step schedule: no tuning steps
    m.it = bench.START_IT
    m.optimizer.sched_step = m.it
    m.model.train()
    return m, batch


def steps(m, batch, n):
    for _ in range(n):
        m.out_dict, m.log_dict = m.train_step(**batch)
        m.call_hook("after_train_step")
        m.it += 1


def ab(n, rounds, warm):
    m, batch = make()
    filters = {"mean": RewardFilter(), "topk": m.reward_filter}
    wall, host = {k: [] for k in filters}, {k: [] for k in filters}
    for name, f in filters.items():
        m.reward_filter = f
        steps(m, batch, warm)
    for _ in range(rounds):
        for name, f in filters.items():
            m.reward_filter = f
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(m, batch, n)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            wall[name].append(1e3 * (t2 - t0) / n)
            host[name].append(1e3 * (t1 - t0) / n)
    ops.check_label_errors()
    print("  one object, SR regime (K = %d), %d rounds of %d steps per setting, ms per step" % (m.sr_decay(), rounds, n))
    for name in filters:
        w, h = np.array(wall[name]), np.array(host[name])
        print("    %-5s wall median %.3f  min %.3f  max %.3f   host enqueue median %.3f  min %.3f  max %.3f   rounds: %s" % (
            name, np.median(w), w.min(), w.max(), np.median(h), h.min(), h.max(), " ".join("%.3f" % v for v in w)))
    d = np.median(wall["topk"]) - np.median(wall["mean"])
    print("    topk - mean: wall %+.1f us per step; spread (max - min) of the mean rounds %.1f us, of the topk rounds %.1f us; the rounds of the two "
          "settings %s" % (1e3 * d, 1e3 * (max(wall["mean"]) - min(wall["mean"])), 1e3 * (max(wall["topk"]) - min(wall["topk"])),
                           "overlap" if (min(wall["topk"]) <= max(wall["mean"]) and min(wall["mean"]) <= max(wall["topk"])) else "do not overlap"))


def bench_lines(path):
    vals = {"this": [], "parent": []}
    for ln in open(path):
        ln = ln.strip()
        if not ln or " " not in ln:
            continue
        label, js = ln.split(" ", 1)
        try:
            d = json.loads(js)
        except ValueError:
            continue
        if label in vals and "value" in d:
            vals[label].append(float(d["value"]))
    print("(c) bench.py --gpus 1 (key absent), this tree against the parent commit's tree, alternating runs on the same box, unlabeled images/s")
    for label in ("parent", "this"):
        v = np.array(vals[label])
        if v.size:
            print("    %-6s  runs: %s   median %.1f   spread (max - min) %.1f = %.2f %%" % (
                label, " ".join("%.1f" % x for x in v), np.median(v), v.max() - v.min(), 100 * (v.max() - v.min()) / np.median(v)))
    if vals["this"] and vals["parent"]:
        print("    this / parent (medians): %.4f" % (np.median(vals["this"]) / np.median(vals["parent"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--bench-lines", default="")
    ap.add_argument("--skip-steps", action="store_true")
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    print("reward_filter; %s (%s, %d CUs), torch %s" % (torch.cuda.get_device_name(0), p.gcnArchName, p.multi_processor_count, torch.__version__))
    launches_alone()
    if not a.skip_steps:
        print("(b) SRFlexMatch ViT-S/2@32, 100 classes, batch 8 / 8 / 8, eager launches, fixed deferred share %.3f, reward_filter: topk (reward_topk 2) "
              "against the mean rule on the same object, interleaved rounds" % SF._DEFER_SEED)
        ab(a.steps, a.rounds, a.warmup)
    if a.bench_lines:
        bench_lines(a.bench_lines)


if __name__ == "__main__":
    main()
