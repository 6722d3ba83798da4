"""ms per step of SRFlexMatch on wrn_28_2 at the classic_cv batch (64 labelled + 448 + 448 unlabelled 32 x 32 images, CIFAR-100), for K = 0 and
K = 8, what the step allocates, and the SRPseudoLabel leg (64 + 64, K = 8) on the same device.  Writes profiles/wrn_strong_steps.txt.

    python tools/wrn_strong_step_time.py [--rounds 7] [--steps 5] [--out profiles/wrn_strong_steps.txt]

Method: every leg is built and warmed first; then ROUNDS rounds, each timing STEPS steps of every leg in turn (interleaved, so drift of the
device's clocks hits all legs alike); a step = train_step + ParamUpdateHook, timed with device events around the STEPS steps; reported: the
median over the rounds and their min .. max.  Memory, per leg: what the leg keeps allocated once it is warm (parameters, optimizer state and
the buffer sets of its launches: allocated after its warm-up minus allocated before it was built), and the allocator's peak above that during
one more step."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semireward_amd import config as srconfig  # noqa: E402
from semireward_amd.algorithms import get_algorithm  # noqa: E402
from semireward_amd.nets import wrn  # noqa: E402
from semireward_amd.utils import synth  # noqa: E402


def leg(yaml, it, Bl, Bu):
    args = srconfig.get_config(os.path.join(ROOT, "configs", yaml), overrides=dict(gpu=0, rank=0, world_size=1, distributed=False, ulb_dest_len=50000))
    alg = get_algorithm(args, wrn.wrn_28_2)
    alg.it = it
    alg.optimizer.sched_step = it
    b = synth.synth_batch(300, Bl, Bu, 32, 100, 50000)
    batch = alg.process_batch(**{k: torch.from_numpy(v) for k, v in b.items()})
    batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}

    def step():
        alg.out_dict, alg.log_dict = alg.train_step(**batch)
        alg.call_hook("after_train_step")
    return alg, step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wrn_strong_steps.txt"))
    a = ap.parse_args()
    flex, pl = "classic_cv/srflexmatch_cifar100_400_wrn_28_2.yaml", "classic_cv_srpseudolabel_cifar100_400_wrn_28_2.yaml"
    # it = 200001: past start_timing (100000), sr_decay() = max(8, 1 + 1048576 / it) = 8, not an N_k step; it = 50001: K = 0, stage-1 update
    specs = [("srflexmatch 64/448/448 K=0 (it 50001)", flex, 50001, 64, 448),
             ("srflexmatch 64/448/448 K=8 (it 200001)", flex, 200001, 64, 448),
             ("srpseudolabel 64/64 K=8 (it 200001)", pl, 200001, 64, 64)]
    legs, mem = {}, {}
    for name, yaml, it, Bl, Bu in specs:           # built and warmed one after the other: a leg's memory is the growth it causes
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        legs[name] = alg, step = leg(yaml, it, Bl, Bu)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        mem[name] = ((base - before) / 2 ** 20, (torch.cuda.max_memory_allocated() - base) / 2 ** 20)
    ms = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, (alg, step) in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.steps)
    lines = ["WideResNet steps of the strong-view SemiReward algorithms: wrn_28_2, CIFAR-100 shapes (tools/wrn_strong_step_time.py)",
             "device: %s; %d interleaved rounds x %d steps per leg, a step = train_step + ParamUpdateHook (SGD + EMA); median [min .. max] ms per step"
             % (torch.cuda.get_device_name(0), a.rounds, a.steps),
             "memory per leg: kept allocated once warm (parameters, optimizer state, the buffer sets of its launches) | allocator peak above that",
             "during one more step (MiB)", ""]
    for name in legs:
        v = ms[name]
        lines.append("%-42s %8.3f ms  [%.3f .. %.3f]   keeps %8.1f MiB | step peak +%8.1f MiB"
                     % (name, statistics.median(v), min(v), max(v), mem[name][0], mem[name][1]))
    k0, k8 = statistics.median(ms[list(legs)[0]]), statistics.median(ms[list(legs)[1]])
    lines += ["", "K = 8 over K = 0: %.2fx (9 statistics groups of 960 images share every launch; two whole-batch backwards instead of one)" % (k8 / k0),
              "K = 8 keeps %.1f GiB more than K = 0: the activations of all K + 1 statistics groups stay allocated."
              % ((mem[list(legs)[1]][0] - mem[list(legs)[0]][0]) / 1024),
              "The two whole-batch backwards of K = 8 do not share launches; their cost is not separated here.",
              "No target is set for these numbers: this file is where the first measurement goes."]
    txt = "\n".join(lines) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
