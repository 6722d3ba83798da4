#!/usr/bin/env python
"""What scoring a whole unlabelled set costs (csrc/score_rows.hip, core/pl_table.py), on one GPU:

  (a) srhip_score_rows and srhip_score_commit alone: HIP events around back-to-back launches on preallocated outputs, [256, 100] and
      [256, 1000] logits, every threshold rule;
  (b) the whole pass: ``score_unlabeled()`` over ``--rows`` synthetic 32 x 32 images resident on the device (``device_data: True``) on
      ViT-S/2 at batch 16 and 256, next to ``evaluate()`` with ``device_eval: True`` over the same rows at the same batch size -- the same
      inference forward followed by one accumulating launch, a path this feature does not touch, so the difference is what the scoring tail
      (score_rows, the Rewarder's forward, reward_mask2, score_commit) adds.  Wall time between two device fences, ``--repeats`` passes each,
      interleaved; and the host time to enqueue a pass.

    python tools/score_unlabeled_time.py > profiles/score_unlabeled.txt
    python tools/score_unlabeled_time.py --tree ../parent --evaluate-only     # the yardstick alone, from another built tree (the parent commit's)
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv[1:-1]:                                  # the package of another built tree, decided before it is imported
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, ROOT)
from semireward_amd import ops                                 # noqa: E402
from semireward_amd.algorithms import get_algorithm            # noqa: E402
try:
    from semireward_amd.core import pl_table as PT             # noqa: E402
except ImportError:                                            # a tree from before this feature: --evaluate-only
    PT = None
from semireward_amd.data.augment import GpuAugment             # noqa: E402
from semireward_amd.data.device_loader import DeviceEvalLoader, dataset_stats      # noqa: E402
from semireward_amd.nets import vit                            # noqa: E402
from semireward_amd.utils import synth                         # noqa: E402

DEV = "cuda:0"


def timed(fn, launches, rounds=6):
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / launches)
    return ts[1:]


def launches_alone(launches=200):
    print("(a) the launches alone, us per launch (HIP events around %d back-to-back launches on preallocated outputs, median of 5 after 1)" % launches)
    g = torch.Generator(device=DEV).manual_seed(0)
    B = 256
    for C in (100, 1000):
        z = torch.randn(B, C, device=DEV, generator=g) * 3
        out = {k: torch.empty(B, dtype=dt, device=DEV) for k, dt in ops.SCORE_COLUMNS}
        pm = torch.rand(C, device=DEV, generator=g) + 0.1
        pm /= pm.sum()
        st = dict(fixed=dict(p_cutoff=0.95), flex=dict(p_cutoff=0.95, classwise_acc=torch.rand(C, device=DEV, generator=g)),
                  free=dict(time_p=torch.tensor([0.7], device=DEV), p_model=pm), soft=dict(mu_var=torch.tensor([0.6, 0.05], device=DEV), n_sigma=2),
                  soft_aligned=dict(mu_var=torch.tensor([0.6, 0.05], device=DEV), n_sigma=2, da_p_model=pm,
                                    da_p_target=torch.full((C,), 1.0 / C, device=DEV), da_inited=torch.ones(1, dtype=torch.int32, device=DEV)))
        for name, kw in st.items():
            ts = timed(lambda: ops.score_rows(z, name.split("_")[0], out, **kw), launches)
            print("  score_rows   [%d, %4d]  %-12s %6.2f us per launch   (min %.2f, max %.2f of the 5)" % (B, C, name, float(np.median(ts)), min(ts), max(ts)))
        n = 50000
        table = PT.PseudoLabelTable(n, DEV, C)
        reward, keep = torch.rand(B, device=DEV, generator=g), (torch.rand(B, device=DEV, generator=g) < 0.5).float()
        idx = torch.randperm(n, device=DEV, generator=g)[:B].contiguous()
        for name, kw in (("row_offset", dict(row_offset=1000)), ("idx", dict(idx=idx))):
            ts = timed(lambda: ops.score_commit(out, reward, keep, table.columns, B, **kw), launches)
            print("  score_commit [%d] -> table of %d, %-10s %6.2f us per launch   (min %.2f, max %.2f of the 5)" % (
                B, n, name, float(np.median(ts)), min(ts), max(ts)))
    ops.check_label_errors()


def whole_pass(rows, repeats, evaluate_only=False):
    rng = np.random.Generator(np.random.PCG64(0))
    C = 100
    x = rng.integers(0, 256, size=(rows, 32, 32, 3)).astype(np.uint8)
    y = rng.integers(0, C, size=rows).astype(np.int64)
    args = argparse.Namespace(
        algorithm="srflexmatch", num_classes=C, num_train_iter=1000, epoch=1, ema_m=0.0, ulb_loss_ratio=1.0, use_cat=True, amp=False, lr=5e-4,
        weight_decay=5e-4, layer_decay=0.5, num_warmup_iter=0, optim="AdamW", T=0.5, p_cutoff=0.95, hard_label=True, thresh_warmup=True, N_k=10,
        start_timing=20, feature_dim=384, sr_lr=5e-4, sr_ema=False, sr_ema_m=0.99, gpu=0, rank=0, world_size=1, distributed=False, seed=0,
        dataset="cifar100", img_size=32, crop_ratio=0.875, batch_size=8, uratio=1, eval_batch_size=256, train_sampler="RandomSampler",
        device_data=True, device_eval=True, overlap_grad_rows=False,
        dataset_dict={"train_lb": {"data": x[:64], "targets": y[:64]}, "train_ulb": {"data": x, "targets": None}, "eval": {"data": x, "targets": y}})
    alg = get_algorithm(args, vit.vit_small_patch2_32)
    alg.model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_params(alg.model.names_shapes, 0).items()})
    alg.model.refresh_operands()
    alg.print_fn = lambda *a, **k: None
    mean, std = dataset_stats(args)
    print("(b) the whole pass over %d resident 32 x 32 rows, ViT-S/2, 100 classes, reward groups of 8 rows (batch_size * uratio): ms per pass between two "
          "device fences (host: ms until the pass is enqueued), %d passes per setting after one warm-up, interleaved" % (rows, repeats))
    for bs in (16, 256):
        ev_loader = DeviceEvalLoader(alg.dataset_dict["eval"], bs, GpuAugment(32, 0, mean, std, device=alg.device))
        runs = {"evaluate(device_eval)": lambda: alg.evaluate("eval", loader=ev_loader)}
        if not evaluate_only:
            runs["score_unlabeled"] = lambda: alg.score_unlabeled(batch_size=bs)
        wall, host = {k: [] for k in runs}, {k: [] for k in runs}
        for r in range(repeats + 1):
            for name, fn in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = fn()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if r:
                    wall[name].append(1e3 * (t2 - t0))
                    host[name].append(1e3 * (t1 - t0))
        batches = -(-rows // bs)
        for name in runs:
            w, h = np.array(wall[name]), np.array(host[name])
            print("  batch %3d  %-22s wall median %9.1f  min %9.1f  max %9.1f   host median %9.1f   = %7.1f us per batch   passes: %s" % (
                bs, name, np.median(w), w.min(), w.max(), np.median(h), 1e3 * np.median(w) / batches, " ".join("%.1f" % v for v in w)))
        if evaluate_only:
            continue
        a, b = np.median(wall["score_unlabeled"]), np.median(wall["evaluate(device_eval)"])
        print("  batch %3d  score_unlabeled / evaluate = %.3f; the scoring tail adds %.1f us per batch over evaluate's one accumulating launch" % (
            bs, a / b, 1e3 * (a - b) / batches))
    if not evaluate_only:
        c = res.read()
        assert (c["count"] == 1).all()
    ops.check_label_errors()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-pass", action="store_true")
    ap.add_argument("--evaluate-only", action="store_true", help="time evaluate() alone (no launches of this feature): works on a tree without it")
    ap.add_argument("--tree", default=None, help="root of the built tree whose package is timed (default: this one)")
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    print("score_unlabeled; %s (%s, %d CUs), torch %s; package of %s" % (torch.cuda.get_device_name(0), p.gcnArchName, p.multi_processor_count,
                                                                     torch.__version__, "this tree" if a.tree is None else "the tree at --tree"))
    if not a.evaluate_only:
        launches_alone()
    if not a.skip_pass:
        whole_pass(a.rows, a.repeats, a.evaluate_only)


if __name__ == "__main__":
    main()
