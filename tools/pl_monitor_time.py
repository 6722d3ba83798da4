#!/usr/bin/env python
"""What ``monitor_pseudo_labels: True`` costs (csrc/pl_monitor.hip, core/pl_monitor.py), on one GPU:

  (a) srhip_pl_monitor alone: HIP events around back-to-back launches on a preallocated state, 9 passes of 8, 56 and 448 unlabelled rows at
      100 classes, one pass (K = 0), and 3000 classes (per-class counters behind global atomics);
  (b) the training step with the key on against the key off: the headline SRFlexMatch step of bench.py (ViT-S/2@32, 8 / 8 / 8, K = 8) and the
      K = 0 regime, the same fixed step schedule, eager launches, rounds interleaved off / on / off / on ...; per round the wall time of
      ``--steps`` steps between two device fences, and the host time to enqueue a step.  Two designs:
        one object   ONE algorithm object built with the key; for the off rounds its ``pl_monitor`` attribute is taken away (exactly what
                     an object built without the key lacks), for the on rounds it is put back: same buffers, same streams, same queue;
        two objects  one object built with the key and one without, from the same seeded state, in one process -- also measures
                     whatever else differs between two objects (addresses, the hardware queue their side streams landed on);
  (c) (optional, ``--bench-lines FILE``) bench.py result lines of this tree (key off) and of the parent commit's tree, run alternately on the
      same box by the caller: one "<label> <json>" per line, label = this | parent.

    python tools/pl_monitor_time.py [--bench-lines FILE] > profiles/pl_monitor.txt

The file for (c): with the parent commit exported and built beside this tree (``git archive <parent> | tar -x -C ../parent`` and
``python -c "import __graft_entry__ as g; g.build()"`` in it), on the GPU box, from this tree's root:

    for i in 1 2 3 4; do
      for label in parent this; do
        if [ $label = parent ]; then dir=../parent; else dir=.; fi
        echo "$label $(cd $dir && python bench.py --gpus 1 --steps 300 --warmup 20 | grep '^{' | tail -n 1)" >> bench_lines.txt
      done
    done
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
from semireward_amd.core.pl_monitor import LOG_KEYS            # noqa: E402
from semireward_amd.nets import vit                            # noqa: E402
from semireward_amd.utils import synth                         # noqa: E402

DEV = "cuda:0"


def launch_alone(launches=200):
    print("(a) srhip_pl_monitor alone, us per launch (HIP events around %d back-to-back launches on a preallocated state, median of 5 after 1)" % launches)
    g = torch.Generator(device=DEV).manual_seed(0)
    for P, nu, C in ((9, 8, 100), (9, 56, 100), (9, 448, 100), (1, 448, 100), (9, 448, 3000)):
        K, n_ulb = P - 1, 50000
        tg = torch.randint(0, C, (n_ulb,), device=DEV, generator=g)
        idx = torch.randperm(n_ulb, device=DEV, generator=g)[:nu].contiguous()
        pseudo = torch.where(torch.rand(P * nu, device=DEV, generator=g) < 0.6, tg[idx].repeat(P), torch.randint(0, C, (P * nu,), device=DEV, generator=g))
        masks = (torch.rand(P, nu, device=DEV, generator=g) < 0.6).float()
        m2 = (torch.rand(max(K, 1) * nu, device=DEV, generator=g) < 0.5).float() if K else None
        r = torch.rand(max(K, 1) * nu, device=DEV, generator=g) if K else None
        ist = torch.zeros(ops.pl_monitor_words(C), dtype=torch.int64, device=DEV)
        fst = torch.zeros(ops.PL_SUMS, dtype=torch.float64, device=DEV)
        ts = []
        for _ in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                ops.pl_monitor(pseudo, masks[0], masks[K], m2, r, idx, tg, P, nu, C, ist, fst)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / launches)
        assert int(ist[0]) == 6 * launches
        print("  P = %d  nu = %3d  C = %4d   %6.2f us per launch   (min %.2f, max %.2f of the 5)" % (
            P, nu, C, float(np.median(ts[1:])), min(ts[1:]), max(ts[1:])))
    ops.check_label_errors()


def make(on, regime):
    common = dict(gpu=0, rank=0, world_size=1, distributed=False)
    extra = {}
    if on:
        extra = dict(monitor_pseudo_labels=True, ulb_targets=np.random.Generator(np.random.PCG64(5)).integers(0, 100, size=50000))
    m = get_algorithm(argparse.Namespace(**common, **dict(bench.NS, algorithm="srflexmatch"), **extra), vit.vit_small_patch2_32)
    m.model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_params(m.model.names_shapes, 0).items()})
    b = synth.synth_batch(100, 8, 8, 32, 100, 50000)
    batch = m.process_batch(**{k: torch.from_numpy(v) for k, v in b.items()})
    m.model.seed = 1234
    m.defer_share = SF._DEFER_SEED                                # one fixed step schedule for both objects: no tuning steps
    m.it = bench.START_IT if regime == "sr" else 1000
    m.optimizer.sched_step = m.it
    m.model.train()
    return m, batch


def steps(m, batch, n):
    for _ in range(n):
        m.out_dict, m.log_dict = m.train_step(**batch)
        m.call_hook("after_train_step")
        m.it += 1


def ab(regime, n, rounds, warm, one_object):
    if one_object:
        both = make(True, regime)
        objs = {False: both, True: both}
        monitor = both[0].pl_monitor
    else:
        objs = {False: make(False, regime), True: make(True, regime)}
    wall, host = {False: [], True: []}, {False: [], True: []}

    def select(flag):
        if one_object:                                            # off: the attribute an object built without the key does not have
            if flag:
                objs[True][0].pl_monitor = monitor
            elif hasattr(objs[True][0], "pl_monitor"):
                del objs[True][0].pl_monitor
    for flag in (False, True):
        select(flag)
        steps(*objs[flag], warm)
    for _ in range(rounds):
        for flag in (False, True):
            select(flag)
            m, batch = objs[flag]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(m, batch, n)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            wall[flag].append(1e3 * (t2 - t0) / n)
            host[flag].append(1e3 * (t1 - t0) / n)
    m_on = objs[True][0]
    assert len(m_on.log_dict) == 12                               # the last round ran with the key on
    line = {k: float(m_on.log_dict["train/" + k]) for k in LOG_KEYS}
    ops.check_label_errors()
    K = m_on.sr_decay() if regime == "sr" else 0
    print("  %s, %s regime (K = %d), %d rounds of %d steps per setting, ms per step" % (
        "one object" if one_object else "two objects", "SR" if regime == "sr" else "pre-start_timing", K, rounds, n))
    for flag in (False, True):
        w, h = np.array(wall[flag]), np.array(host[flag])
        print("    key %-3s  wall median %.3f  min %.3f  max %.3f   host enqueue median %.3f  min %.3f  max %.3f   rounds: %s" % (
            "on" if flag else "off", np.median(w), w.min(), w.max(), np.median(h), h.min(), h.max(), " ".join("%.3f" % v for v in w)))
    d = np.median(wall[True]) - np.median(wall[False])
    dh = np.median(host[True]) - np.median(host[False])
    print("    on - off: wall %+.1f us per step, host enqueue %+.1f us per step; spread (max - min) of the off rounds %.1f us, of the on rounds %.1f us; "
          "the rounds of the two settings %s" % (1e3 * d, 1e3 * dh, 1e3 * (max(wall[False]) - min(wall[False])), 1e3 * (max(wall[True]) - min(wall[True])),
                                                 "overlap" if (min(wall[True]) <= max(wall[False]) and min(wall[False]) <= max(wall[True])) else "do not overlap"))
    print("    the on run's last log line (one resident batch repeated, random true labels): " + "  ".join("%s %.4f" % (k, v) for k, v in line.items()))
    del objs


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
    print("(c) bench.py --gpus 1 (key off), this tree against the parent commit's tree, alternating runs on the same box, %s" % "unlabeled images/s")
    for label in ("parent", "this"):
        v = np.array(vals[label])
        if v.size:
            print("    %-6s  runs: %s   median %.1f   spread (max - min) %.1f = %.2f %%" % (
                label, " ".join("%.1f" % x for x in v), np.median(v), v.max() - v.min(), 100 * (v.max() - v.min()) / np.median(v)))
    if vals["this"] and vals["parent"]:
        a, b = np.median(vals["this"]), np.median(vals["parent"])
        print("    this / parent (medians): %.4f" % (a / b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--bench-lines", default="")
    ap.add_argument("--skip-steps", action="store_true")
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    print("monitor_pseudo_labels; %s (%s, %d CUs), torch %s" % (torch.cuda.get_device_name(0), p.gcnArchName, p.multi_processor_count, torch.__version__))
    launch_alone()
    if not a.skip_steps:
        print("(b) SRFlexMatch ViT-S/2@32, 100 classes, batch 8 / 8 / 8, eager launches, fixed deferred share %.3f, key on vs off in interleaved rounds" % SF._DEFER_SEED)
        for one_object in (True, False):
            for regime in ("sr", "pre"):
                ab(regime, a.steps, a.rounds, a.warmup, one_object)
    if a.bench_lines:
        bench_lines(a.bench_lines)


if __name__ == "__main__":
    main()
