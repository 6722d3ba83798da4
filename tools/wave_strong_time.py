#!/usr/bin/env python
"""What ``device_audio_strong: True`` costs (semireward_amd/data/device_audio.py, csrc/wave_strong.hip), on one GPU:

  (a) srhip_wave_effect alone, one op per launch, B = 8 rows of 64 000 samples (4 s at 16 kHz, the usb_audio yamls' batch), and the resample at
      8 x 480 000 (a 30 s clip): HIP events around back-to-back launches, us per launch, median of 5 windows after one warm-up window;
  (b) the strong view of a loader: the three launches of the key (two effect slots + srhip_wave_view) against the one srhip_wave_view launch on
      a stored variant that they replace -- device time per view (events) and host time to enqueue one;
  (c) the Wav2Vec2-base SRFreeMatch step of bench.py (configs/usb_audio_srfreematch_urbansound8k_100_wave2vecv2_base.yaml, batch 8 / 8,
      64 000 samples, K = 8) fed by the loaders: ONE algorithm object, its unlabelled batches from a loader with the key against a loader over
      the same clips with ``data_s``, rounds interleaved; per round the wall time between two device fences and the host time to enqueue;
  (d) (``--bench-lines FILE``) bench.py result lines of this tree (the key is never set) and of the parent commit's tree, run alternately on
      the same box by the caller: one "<label> <json>" per line, label = this | parent (tools/pl_monitor_time.py has the recipe);
  ``--headroom``: instead of the above, every kernel case of tests/_wave_strong_cases.py against its bound: the share each op uses.

    python tools/wave_strong_time.py [--bench-lines FILE] > profiles/wave_strong.txt
    python tools/wave_strong_time.py --headroom > profiles/wave_strong_headroom.txt
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
import _wave_strong_cases as WS                               # noqa: E402
import _wave_view_cases as WC                                 # noqa: E402
from semireward_amd import ops                               # noqa: E402
from semireward_amd.data import device_audio as DA           # noqa: E402

DEV = "cuda:0"
B, S, RATE = 8, 64000, 16000


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


def effect_alone():
    print("(a) srhip_wave_effect alone, one op for all rows, us per launch (HIP events around back-to-back launches, median of 5 windows after 1)")
    dl = ops.reverb_delays(RATE)
    for n, cases, launches in ((S, (("copy", WS.COPY, 0), ("gain -3 dB", WS.GAIN, WS.effect_of(1.0, 0.0, -3, 0)[1]), ("resample s = 0.5", WS.RESAMPLE, WS.step_of(0.5)),
                                    ("resample s = 0.75", WS.RESAMPLE, WS.step_of(0.75)), ("resample s = 2^(2/1200)", WS.RESAMPLE, WS.step_of(2.0 ** (2.0 / 1200.0))),
                                    ("resample s = 1.3", WS.RESAMPLE, WS.step_of(1.3)), ("resample s = 2.0", WS.RESAMPLE, WS.step_of(2.0)), ("reverb 16 kHz", WS.REVERB, 0)), 40),
                               (480000, (("resample s = 0.5", WS.RESAMPLE, WS.step_of(0.5)), ("resample s = 1.3", WS.RESAMPLE, WS.step_of(1.3)),
                                         ("resample s = 2.0", WS.RESAMPLE, WS.step_of(2.0)), ("reverb 16 kHz", WS.REVERB, 0)), 8)):
        ds = DA.DeviceWaveDataset([WS.clip(10 + i, n) for i in range(B)], None, DEV)
        rows = np.arange(B, dtype=np.int64)
        dst = torch.empty(B, 2 * n, dtype=torch.float32, device=DEV)
        for name, op, param in cases:
            h = (rows, np.full(B, op, dtype=np.int32), np.full(B, param, dtype=np.int64), None, ds.row_len_host)
            m = ops.wave_effect_len(ds.row_len_host, h[1], h[2]).astype(np.int32)
            h = h[:3] + (m,) + h[4:]
            d = [torch.from_numpy(x).to(DEV) for x in h[:4]]
            ts = windows(lambda: ops.wave_effect(ds.store, ds.row_off, ds.row_len, *d, dst, dl, host=h), launches)
            print("  %d x %6d  %-24s -> %6d samples  %9.1f us per launch   (min %.1f, max %.1f of the 5; %d launches a window)" % (
                B, n, name, m[0], float(np.median(ts)), min(ts), max(ts), launches))


def clips(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [WC.clip(seed + i, int(k)) for i, k in enumerate(rng.integers(int(3.0 * RATE), int(6.0 * RATE), size=n))]      # 3 .. 6 s: cropped and padded rows


def loaders(steps):
    """(labelled loader, unlabelled loader with data_s, unlabelled loader with the key) over the same clips."""
    lb, ulb = clips(100, 200), clips(256, 400)
    rng = np.random.Generator(np.random.PCG64(2))
    var = [[WC.clip(9000 + 1000 * v + i, int(len(c) * (0.8, 1.25)[v])) for i, c in enumerate(ulb)] for v in range(2)]
    dl = DA.DeviceWaveDataset(lb, rng.integers(0, 10, size=len(lb)), DEV)
    du_s, du = DA.DeviceWaveDataset(ulb, None, DEV, data_s=var), DA.DeviceWaveDataset(ulb, None, DEV)
    keys = ("idx_ulb", "x_ulb_w", "x_ulb_s")
    ld_l = DA.WaveTrainLoader(dl, B, DA.EpochSampler(len(dl), steps * B, 1, 0), S, True, keys=("idx_lb", "x_lb", "y_lb"), seed=(0, 0, 0))
    ld_s = DA.WaveTrainLoader(du_s, B, DA.EpochSampler(len(du_s), steps * B, 1, 0), S, True, keys=keys, seed=(0, 0, 1))
    ld_k = DA.WaveTrainLoader(du, B, DA.EpochSampler(len(du), steps * B, 1, 0), S, True, keys=keys, seed=(0, 0, 1), device_strong=True, sample_rate=RATE)
    return ld_l, ld_s, ld_k


def view_alone(steps=24):
    print("(b) one strong view of B = %d rows of %d samples from clips of 3 .. 6 s: the key's three launches against the one launch on a stored variant" % (B, S))
    _, ld_s, ld_k = loaders(steps)
    for name, ld in (("data_s: srhip_wave_view on a variant", ld_s), ("key: effect, effect, srhip_wave_view", ld_k)):
        table, where, N = ld._epoch_table()
        dev = ld._copy(torch.from_numpy(table))
        view = ld._view_fn(dev, where["x_ulb_s"], ld.draws["x_ulb_s"], "x_ulb_s")
        view(0, 0)
        torch.cuda.synchronize()
        dev_t, host_t = [], []
        for t in range(steps):                                  # every step's own draws: the ops differ from step to step
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            view(t * B, t)
            host_t.append(time.perf_counter() - t0)
            e1.record()
            e1.synchronize()
            dev_t.append(e0.elapsed_time(e1) * 1e3)
        d, h = np.array(dev_t), np.array(host_t) * 1e6
        print("  %-40s device median %8.1f us  p10 %8.1f  p90 %8.1f  max %8.1f   host enqueue median %6.1f us  p90 %6.1f   (n = %d views)" % (
            name, np.median(d), np.percentile(d, 10), np.percentile(d, 90), d.max(), np.median(h), np.percentile(h, 90), steps))
        if ld.makes_strong:
            sd = ld.strong_draws
            names = {WS.GAIN: "gain", WS.RESAMPLE: "resample", WS.REVERB: "reverb"}
            worst = int(np.argmax(d))
            print("    slowest view: step %d, its rows' slots %s" % (worst, " ".join("%s+%s" % (names[a], names[b]) for a, b in sd["op"][worst * B:worst * B + B].tolist())))


def step_ab(n, rounds, warm):
    from semireward_amd import config as srconfig
    from semireward_amd.algorithms import get_algorithm
    from semireward_amd.nets import wave2vec
    ypath = os.path.join(ROOT, "configs", "usb_audio_srfreematch_urbansound8k_100_wave2vecv2_base.yaml")
    args = srconfig.get_config(ypath, overrides=dict(gpu=0, rank=0, world_size=1, distributed=False))
    m = get_algorithm(args, wave2vec.wave2vecv2_base)
    m.model.seed, m.it = 1234, 90001                                  # bench.py's steady SR regime: sr_decay() = 8
    m.optimizer.sched_step = m.it
    m.model.train()
    total = warm + n * rounds
    ld_l, ld_s, ld_k = loaders(total)
    print("(c) %s Wav2Vec2-base step (K = %d), batch %d / %d of %d samples, fed by the loaders; ONE object, unlabelled batches from the key's loader "
          "against data_s, interleaved rounds" % (args.algorithm, m.sr_decay(), B, B, S))
    its = {k: (iter(ld_l), iter(ld)) for k, ld in (("data_s", ld_s), ("key", ld_k))}

    def steps(which, k):
        il, iu = its[which]
        for _ in range(k):
            a, b = next(il), next(iu)
            m.out_dict, m.log_dict = m.train_step(**m.process_batch(x_lb=a["x_lb"], y_lb=a["y_lb"], x_ulb_w=b["x_ulb_w"], x_ulb_s=b["x_ulb_s"]))
            m.call_hook("after_train_step")
            m.it += 1
    wall, host = {"data_s": [], "key": []}, {"data_s": [], "key": []}
    for which in wall:
        steps(which, warm)
    for _ in range(rounds):
        for which in wall:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(which, n)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            wall[which].append(1e3 * (t2 - t0) / n)
            host[which].append(1e3 * (t1 - t0) / n)
    assert np.isfinite(float(m.log_dict["train/total_loss"]))
    print("  %d rounds of %d steps per setting, ms per step (the loaders' launches and the host work of next() included)" % (rounds, n))
    for which in wall:
        w, h = np.array(wall[which]), np.array(host[which])
        print("    %-6s  wall median %.3f  min %.3f  max %.3f   host enqueue median %.3f  min %.3f  max %.3f   rounds: %s" % (
            which, np.median(w), w.min(), w.max(), np.median(h), h.min(), h.max(), " ".join("%.3f" % v for v in w)))
    d, dh = np.median(wall["key"]) - np.median(wall["data_s"]), np.median(host["key"]) - np.median(host["data_s"])
    over = min(wall["key"]) <= max(wall["data_s"]) and min(wall["data_s"]) <= max(wall["key"])
    print("    key - data_s: wall %+.1f us per step (%.2f %%), host enqueue %+.1f us per step; spread (max - min) of the data_s rounds %.1f us, of the key "
          "rounds %.1f us; the rounds of the two settings %s" % (1e3 * d, 100 * d / np.median(wall["data_s"]), 1e3 * dh,
                                                                 1e3 * (max(wall["data_s"]) - min(wall["data_s"])),
                                                                 1e3 * (max(wall["key"]) - min(wall["key"])), "overlap" if over else "do not overlap"))


def headroom():
    dl = list(WS.DELAYS_16K)
    print("kernel cases of tests/_wave_strong_cases.py against the float64 restatement: the largest share of its bound an element uses, per op and case")
    print("resample (bound_j = 32 u sum |x_k| + (taps + 2) u sum |x_k h_k|, u = 2^-24), n in %s per launch" % (WS.RESAMPLE_N,))
    for s in WS.RESAMPLE_S:
        step = WS.step_of(s)
        cl = [WS.clip(100 + n, max(n, 2))[:n] for n in WS.RESAMPLE_N]
        outs, _, _ = WS.launch(cl, [(WS.RESAMPLE, step)] * len(cl), dl, DEV)
        errs = [float(np.abs(o - WS.resample(c.astype(np.float64), step)[0]).max()) for c, o in zip(cl, outs)]
        print("  s = %.6f   used %.4f   largest |error| %.3e" % (s, max(WS.check_resample(c, step, o, s) for c, o in zip(cl, outs)), max(errs)))
    for s in (1.3, 2.0 ** (-2.0 / 1200.0)):
        x, step = WS.clip(77, WS.LONG_N), WS.step_of(s)
        (o,), _, _ = WS.launch([x], [(WS.RESAMPLE, step)], dl, DEV)
        print("  s = %.6f   n = %d   used %.4f   largest |error| %.3e" % (s, WS.LONG_N, WS.check_resample(x, step, o, s),
                                                                         float(np.abs(o - WS.resample(x.astype(np.float64), step)[0]).max())))
    print("gain (bound 1.5 ulp_fp32 of the float64 value before the clamp), 501 samples, the peak first / last / middle")
    for att in WS.GAIN_ATT:
        cl = [WS.gain_clip(10 * (att + 4) + i, 501 + att, w) for i, w in enumerate(("first", "last", "middle"))]
        outs, _, _ = WS.launch(cl, [(WS.GAIN, WS.gain_bits(att))] * 3, dl, DEV)
        print("  att = %+d dB   used %.4f (of 1.5 ulp: %.3f ulp)" % ((att,) + (lambda u: (u, 1.5 * u))(max(WS.check_gain(c, att, o, att) for c, o in zip(cl, outs)))))
    print("reverb (bound: the per-sample roundings through the network's l1 gains, tests/_wave_strong_cases.py:reverb_bound)")
    for rate, lens, d in ((16000, WS.REVERB_N_16K, WS.DELAYS_16K), (8000, WS.REVERB_N_8K, WS.DELAYS_8K)):
        cl = [WS.clip(300 + n, max(n, 2))[:n] for n in lens]
        outs, _, _ = WS.launch(cl, [(WS.REVERB, 0)] * len(cl), d, DEV)
        g = WS.reverb_gains(tuple(d), WS.ir_length(rate))
        errs = [float(np.abs(o - WS.reverb(c.astype(np.float64), list(d))).max()) for c, o in zip(cl, outs)]
        print("  %5d Hz   sum |h| = %.2f   bound %.3e per unit of max |x|   used %.5f   largest |error| %.3e (max |out| %.3f)" % (
            rate, g["G"], WS.reverb_bound(list(d), 1.0, WS.ir_length(rate)), max(WS.check_reverb(c, list(d), rate, o, rate) for c, o in zip(cl, outs)),
            max(errs), max(float(np.abs(o).max()) for o in outs)))


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
    print("(d) bench.py --gpus 1 (the key is never set), this tree against the parent commit's tree, alternating runs on the same box, unlabeled images/s")
    for label in ("parent", "this"):
        v = np.array(vals[label])
        if v.size:
            print("    %-6s  runs: %s   median %.1f   spread (max - min) %.1f = %.2f %%" % (
                label, " ".join("%.1f" % x for x in v), np.median(v), v.max() - v.min(), 100 * (v.max() - v.min()) / np.median(v)))
    if vals["this"] and vals["parent"]:
        print("    this / parent (medians): %.4f" % (np.median(vals["this"]) / np.median(vals["parent"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--bench-lines", default="")
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--headroom", action="store_true")
    ap.add_argument("--only-bench-lines", action="store_true", help="print (d) alone (appended to the file by the caller once the runs are done)")
    a = ap.parse_args()
    if a.only_bench_lines:
        return bench_lines(a.bench_lines)
    p = torch.cuda.get_device_properties(0)
    print("device_audio_strong; %s (%s, %d CUs), torch %s" % (torch.cuda.get_device_name(0), p.gcnArchName, p.multi_processor_count, torch.__version__))
    if a.headroom:
        return headroom()
    effect_alone()
    view_alone()
    if not a.skip_steps:
        step_ab(a.steps, a.rounds, a.warmup)
    if a.bench_lines:
        bench_lines(a.bench_lines)


if __name__ == "__main__":
    main()
