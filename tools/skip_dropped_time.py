#!/usr/bin/env python
"""Isolated launch timings behind ``vit._SKIP_DROPPED_BRANCHES`` (profiles/skip_dropped_branches.txt), ViT-S width, N = 257, Hd = 1536, one GPU:

  (1) is the row map free?  srhip_mlp_fused_proj_planned with an identity plan (n_mlp = B, order = 0 .. B-1) against srhip_mlp_fused_proj at
      B = 100 (201 tiles, one round);
  (2) does launch time follow the heavy-tile count?  the planned launch at B = 800 (1607 tiles = 6.3 rounds of 256 workgroups) with n_mlp
      from 800 down to 640;
  (3) srhip_attn_block_fused at B = 100 with 0, 10 and 20 images whose out_scale is 0;
  (4) srhip_vit_droppath_plan (one per forward: two per step) at depth 12, B = 100 and 800.

HIP events around back-to-back launches on preallocated operands; the settings of one comparison interleaved; median of the rounds after the first.

    python tools/skip_dropped_time.py > timings.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semireward_amd import ops                                  # noqa: E402

DEV = "cuda:0"
D, HD, N = 384, 1536, 257
BF = torch.bfloat16
KEPT = 1.0 / 0.85


def timed(fns, launches, rounds):
    """fns: {label: callable}; us per launch of each, interleaved rounds."""
    ts = {k: [] for k in fns}
    for _ in range(rounds + 1):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e3 / launches)
    return {k: (float(np.median(v[1:])), min(v[1:]), max(v[1:])) for k, v in ts.items()}


def show(res, note=None):
    for k, (med, lo, hi) in res.items():
        print("    %-34s %8.2f us per launch   (min %.2f, max %.2f)%s" % (k, med, lo, hi, ("   " + note[k]) if note else ""))


def mlp_operands(B, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)      # noqa: E731
    M = B * N
    return dict(x=r(M, D), xo=torch.empty(M, D, device=DEV), ao=r(M, D).to(BF), Wp=(r(D, D) * 0.05).to(BF), bp=r(D) * 0.1,
                gam=torch.rand(D, generator=g, device=DEV) + 0.5, bet=r(D) * 0.2, W1=(r(HD, D) * 0.05).to(BF), b1=r(HD) * 0.1,
                W2=(r(D, HD) * 0.03).to(BF), b2=r(D) * 0.1, ln=torch.empty(M, D, dtype=BF, device=DEV))


def mlp_launch(t, B, s1, s2, plan):
    def fn():
        ops.mlp_fused_proj(t["x"], t["ao"], t["Wp"], t["bp"], s1, t["gam"], t["bet"], 1e-6, t["W1"], t["b1"], t["W2"], t["b2"], s2, N, B * N, D, HD,
                           x_out=t["xo"], ln_next=t["ln"], next_gamma=t["gam"], next_beta=t["bet"], ao_scaled=True, plan_row=plan)
    return fn


def plan_of(s2):
    keep = (s2 != 0).cpu().numpy()
    row = np.concatenate([[int(keep.sum())], np.argsort(~keep, kind="stable")]).astype(np.int32)
    return torch.from_numpy(row).to(DEV)


def row_map(launches, rounds):
    B = 100
    print("(1) the row map: planned launch with an identity plan against the dense launch, B = %d (%d tiles), all factors %.4f" % (B, -(-B * N // 128), KEPT))
    t = mlp_operands(B, 1)
    s = torch.full((B,), KEPT, device=DEV)
    show(timed({"dense": mlp_launch(t, B, s, s, None), "planned, identity plan": mlp_launch(t, B, s, s, plan_of(s))}, launches, rounds))


def heavy_count(launches, rounds):
    B = 800
    tiles = -(-B * N // 128)
    print("(2) planned launch at B = %d (%d tiles on 256 workgroups), the dropped images spread evenly; dense = the same factors, no plan" % (B, tiles))
    t = mlp_operands(B, 2)
    s1 = torch.full((B,), KEPT, device=DEV)
    fns, note = {}, {}
    for n_mlp in (800, 760, 720, 680, 640):
        s2 = torch.full((B,), KEPT, device=DEV)
        if n_mlp < B:
            s2[torch.linspace(0, B - 1, B - n_mlp, device=DEV).round().long()] = 0.0
        assert int((s2 != 0).sum()) == n_mlp
        fns["planned n_mlp = %d" % n_mlp] = mlp_launch(t, B, s1, s2, plan_of(s2))
        note["planned n_mlp = %d" % n_mlp] = "heavy tiles %d of %d" % (-(-n_mlp * N // 128), tiles)
        if n_mlp in (800, 640):
            fns["dense   n_mlp = %d" % n_mlp] = mlp_launch(t, B, s1, s2, None)
            note["dense   n_mlp = %d" % n_mlp] = ""
    show(timed(fns, launches, rounds), note)


def attention(launches, rounds):
    B = 100
    print("(3) srhip_attn_block_fused, N = %d, B = %d (2 head groups per image: %d workgroups), images with out_scale 0 spread evenly" % (N, B, 2 * B))
    g = torch.Generator(device=DEV).manual_seed(3)
    xn = torch.randn(B * N, D, generator=g, device=DEV).to(BF)
    W = (torch.randn(3 * D, D, generator=g, device=DEV) * 0.05).to(BF)
    bias = torch.randn(3 * D, generator=g, device=DEV) * 0.1
    qkvx = torch.empty(B, 3 * D, dtype=BF, device=DEV)
    out = torch.empty(B * N, D, dtype=BF, device=DEV)
    fns = {}
    for nd in (0, 10, 20):
        osc = torch.full((B,), KEPT, device=DEV)
        if nd:
            osc[torch.linspace(0, B - 1, nd, device=DEV).round().long()] = 0.0
        fns["%2d dropped (incl. the 257th-token GEMM)" % nd] = (
            lambda osc=osc: ops.attn_block_fused(xn, W, bias, out, B, N, D, 6, 0.125, qkv_extra=qkvx, out_scale=osc))
    show(timed(fns, launches, rounds))


def plan_launch(launches, rounds):
    print("(4) srhip_vit_droppath_plan, depth 12 (one launch per forward: two per step)")
    fns = {}
    for B in (100, 800):
        dp = torch.where(torch.rand(12, 2, B, device=DEV) < 0.1, 0.0, KEPT)
        plan = torch.empty(12, 1 + B, dtype=torch.int32, device=DEV)
        fns["B = %d" % B] = (lambda dp=dp, plan=plan, B=B: ops.vit_droppath_plan(dp, 12, B, plan))
    show(timed(fns, launches, rounds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    print("skip dropped branches, isolated launches; %s (%s, %d CUs), torch %s; %d launches per round, median of %d rounds" % (
        torch.cuda.get_device_name(0), p.gcnArchName, p.multi_processor_count, torch.__version__, a.launches, a.rounds))
    row_map(a.launches, a.rounds)
    heavy_count(max(10, a.launches // 5), a.rounds)
    attention(a.launches, a.rounds)
    plan_launch(a.launches, a.rounds)


if __name__ == "__main__":
    main()
