#!/usr/bin/env python
"""End-to-end on one MI355X through the library's waveform input pipeline (``device_audio: True``): synthetic clips of ragged length (a class is a
pair of tones; 0.6 .. 1.8 times the training window long), a tiny Wav2Vec2, SRPseudoLabel or SRFreeMatch.  The clips go in as a plain
``dataset_dict``; the engine packs them into one flat fp32 store on the device, builds the reference's sampler stream, and every view of a batch --
crop, zero padding, the feature extractor's normalisation -- is one launch (data/device_audio.py, csrc/wave_view.hip).  ``alg.train()`` /
``alg.evaluate()`` run with no hand-written batch generator.

SRFreeMatch takes a strong view: the unlabelled set carries V = 2 pre-augmented variants of every clip (``data_s``), here a numpy stand-in for the
reference's sox chain (gain, a speed change by resampling, additive noise).  With ``--device-strong`` (``device_audio_strong: True``) there is no
``data_s``: SRFlexMatch trains on strong views the engine makes on the device from the clean clips, two freshly drawn effects per sample and epoch
(csrc/wave_strong.hip).

    python examples/train_device_audio.py --steps 60
    python examples/train_device_audio.py --steps 60 --algorithm srfreematch
    python examples/train_device_audio.py --steps 60 --device-strong  # srflexmatch, the strong views made on the device
    python examples/train_device_audio.py --steps 60 --run-hooks     # the reference's evaluation / checkpoint / logging hooks drive the run
"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semireward_amd.algorithms import get_algorithm          # noqa: E402
from semireward_amd.core.hooks import Hook                   # noqa: E402
from semireward_amd.nets import wave2vec                     # noqa: E402

RATE, SECONDS = 1000, 2.0                                     # L = 2000 samples


def synth_clips(n, num_classes, seed):
    """n float32 clips of 0.6 L .. 1.8 L samples: two tones whose frequencies depend on the class, a random phase, noise; + labels."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y = rng.integers(0, num_classes, size=n)
    L = int(round(RATE * SECONDS))
    out = []
    for c in y:
        t = np.arange(int(rng.integers(int(0.6 * L), int(1.8 * L)))) / RATE
        f1, f2 = 20.0 + 9.0 * c, 150.0 - 11.0 * c
        w = np.sin(2 * np.pi * f1 * t + rng.uniform(0, 6.28)) + 0.5 * np.sin(2 * np.pi * f2 * t + rng.uniform(0, 6.28))
        out.append((0.1 * w + 0.03 * rng.standard_normal(t.size)).astype(np.float32))
    return out, y.astype(np.int64)


def strong_variant(w, rng):
    """A stand-in for WaveformTransforms: gain in [-5, 5] dB, speed in [0.8, 1.25] by linear resampling, noise."""
    speed = rng.uniform(0.8, 1.25)
    pos = np.arange(0, w.size - 1, speed)
    v = np.interp(pos, np.arange(w.size), w) * 10.0 ** (rng.uniform(-5, 5) / 20.0)
    return (v + 0.02 * rng.standard_normal(v.size)).astype(np.float32)


class PrintHook(Hook):
    def after_train_step(self, alg):
        if alg.it % 10 == 0 or alg.it == alg.num_train_iter - 1:
            print("it %3d  epoch %d  sup %.3f  unsup %.3f  util %.2f" % (alg.it, alg.epoch, float(alg.log_dict["train/sup_loss"]),
                                                                        float(alg.log_dict["train/unsup_loss"]),
                                                                        float(alg.log_dict["train/util_ratio"])), flush=True)


ALGORITHMS = {"srpseudolabel": dict(unsup_warm_up=0.4),
              "srflexmatch": dict(thresh_warmup=True),
              "srfreematch": dict(ema_p=0.9, use_quantile=True, clip_thresh=False, ent_loss_ratio=0.01)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--algorithm", choices=sorted(ALGORITHMS), default="srpseudolabel")
    ap.add_argument("--run-hooks", action="store_true",
                    help="run_hooks + device_eval: evaluate and checkpoint every 20 steps (into a temporary save_dir), log every 10")
    ap.add_argument("--device-strong", action="store_true",
                    help="device_audio_strong: the strong views are made on the device, no data_s (srflexmatch unless --algorithm names a strong-view one)")
    a = ap.parse_args()
    if a.device_strong and a.algorithm == "srpseudolabel":
        a.algorithm = "srflexmatch"
    C = a.classes
    x_lb, y_lb = synth_clips(10 * C, C, 1)
    x_ulb, _ = synth_clips(512, C, 2)
    x_te, y_te = synth_clips(128, C, 3)
    ulb = {"data": x_ulb, "targets": None}
    if a.algorithm != "srpseudolabel" and not a.device_strong:   # its train_step takes x_ulb_s: V = 2 pre-augmented variants per clip
        rng = np.random.Generator(np.random.PCG64(4))
        ulb["data_s"] = [[strong_variant(w, rng) for w in x_ulb] for _ in range(2)]
    steps = max(a.steps, a.epochs) // a.epochs * a.epochs
    args = argparse.Namespace(
        algorithm=a.algorithm, num_classes=C, num_train_iter=steps, epoch=a.epochs, ema_m=0.0, ulb_loss_ratio=1.0, use_cat=False, amp=False,
        lr=5e-4, weight_decay=5e-4, layer_decay=0.75, num_warmup_iter=5, optim="AdamW", T=0.5, p_cutoff=0.95, hard_label=True, N_k=10, start_timing=20,
        feature_dim=128, sr_lr=5e-4, sr_ema=False, sr_ema_m=0.99, gpu=0, rank=0, world_size=1, distributed=False, seed=0,
        # the input pipeline: what a usb_audio yaml says (window, rate, batch sizes, sampler) + the clips + the option
        dataset="synthetic_tones", sample_rate=RATE, max_length_seconds=SECONDS, batch_size=a.batch, uratio=1, eval_batch_size=16,
        train_sampler="RandomSampler", device_audio=True, audio_do_normalize=True, device_audio_strong=a.device_strong,
        dataset_dict={"train_lb": {"data": x_lb, "targets": y_lb}, "train_ulb": ulb, "eval": {"data": x_te, "targets": y_te}},
        **ALGORITHMS[a.algorithm])
    if a.run_hooks:
        with tempfile.TemporaryDirectory() as save_dir:
            vars(args).update(run_hooks=True, device_eval=True, num_eval_iter=20, num_log_iter=10, save_dir=save_dir, save_name="example")
            alg = get_algorithm(args, wave2vec.wave2vecv2_tiny_test)
            alg.train()
            print("results:", alg.results_dict, " files:", sorted(os.listdir(os.path.join(save_dir, "example"))))
            ev = alg.evaluate("eval")
    else:
        alg = get_algorithm(args, wave2vec.wave2vecv2_tiny_test)
        alg.register_hook(PrintHook(), "PrintHook", "LOWEST")
        alg.train()
        ev = alg.evaluate("eval")
    print("eval:", {k: round(float(v), 4) for k, v in ev.items()})
    return ev


if __name__ == "__main__":
    main()
