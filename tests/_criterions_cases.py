"""The cases of tests/golden/criterions.npz and their seeded inputs, shared by the generator (tools/gen_criterions_golden.py) and the tests
(tests/test_{cpu,gpu}_criterions.py): the fixture stores only what the reference computed; every input is rebuilt from its seed.

A case: kind 'hard' | 'soft' (ce_loss) or 'mse' | 'l1' (consistency_loss); B, C; logit gain (1, and 24 which saturates the softmax);
hard / soft: reduction none | mean | sum, soft target kinds 'prob' (softmax at temperature 0.5), 'onehot', 'raw' (un-normalised, >= 0);
mse / l1: masks 'nomask' | 'mask' | 'mask2' (mask and mask2, both with zero rows) and one 'allzero' case each; 'l1' targets carry a few
exact ties z == t."""
import numpy as np

CS = (2, 10, 100, 1000)
BS = (1, 8, 67, 1024)
GAINS = (1, 24)
REDUCTIONS = ("none", "mean", "sum")
SOFT_KINDS = ("prob", "onehot", "raw")
MASK_KINDS = ("nomask", "mask", "mask2")
GRAD_SAMPLES = 192          # gradients larger than 1024 elements are stored as a strided sample of about this many
_FAMILY = {"hard": 0, "soft": 1, "mse": 2, "l1": 3}


def cases():
    out = []
    for C in CS:
        for B in BS:
            for gain in GAINS:
                s = dict(B=B, C=C, gain=gain)
                for r in REDUCTIONS:
                    out.append(dict(s, kind="hard", reduction=r, tkind="int", mkind="nomask"))
                    for tk in SOFT_KINDS:
                        out.append(dict(s, kind="soft", reduction=r, tkind=tk, mkind="nomask"))
                for kind in ("mse", "l1"):
                    for mk in MASK_KINDS:
                        out.append(dict(s, kind=kind, reduction="mean", tkind="prob" if kind == "mse" else "logit", mkind=mk))
    for kind in ("mse", "l1"):
        out.append(dict(B=67, C=100, gain=1, kind=kind, reduction="mean", tkind="prob" if kind == "mse" else "logit", mkind="allzero"))
    for c in out:
        c["id"] = "{kind}/B{B}_C{C}_g{gain}/{reduction}_{tkind}_{mkind}".format(**c)
    return out


def _softmax64(x, T):
    x = x.astype(np.float64) / T
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def inputs(c):
    """numpy inputs of a case: logits fp32 [B, C], targets (int64 [B] or fp32 [B, C]), mask / mask2 (fp32 [B] or None)."""
    B, C, gain = c["B"], c["C"], c["gain"]
    rng = np.random.Generator(np.random.PCG64([C, B, gain, _FAMILY[c["kind"]], SOFT_KINDS.index(c["tkind"]) if c["tkind"] in SOFT_KINDS else 0]))
    logits = (gain * rng.standard_normal((B, C))).astype(np.float32)
    y = rng.integers(0, C, size=(B,), dtype=np.int64)
    weak = (gain * rng.standard_normal((B, C))).astype(np.float32)
    if c["tkind"] == "int":
        targets = y
    elif c["tkind"] == "prob":
        targets = _softmax64(weak, 0.5)
    elif c["tkind"] == "onehot":
        targets = np.zeros((B, C), np.float32)
        targets[np.arange(B), y] = 1.0
    elif c["tkind"] == "raw":
        targets = (2.0 * rng.random((B, C))).astype(np.float32)
    else:                                                    # 'logit' ('l1'): logit-like targets with a few exact ties
        targets = weak.copy()
        flat = rng.choice(B * C, size=min(5, B * C // 2), replace=False)
        targets.reshape(-1)[flat] = logits.reshape(-1)[flat]
    mask = mask2 = None
    if c["mkind"] in ("mask", "mask2", "allzero"):
        mask = rng.random(B).astype(np.float32)
        mask[rng.random(B) < 0.3] = 0.0
        if B >= 2:
            mask[0] = 0.0
        if c["mkind"] == "allzero":
            mask[:] = 0.0
    if c["mkind"] == "mask2":
        mask2 = (rng.random(B) < 0.6).astype(np.float32)
        if B >= 2:
            mask2[1] = 0.0
    return dict(logits=logits, targets=targets, mask=mask, mask2=mask2)


def grad_stride(n):
    """Stride of the stored gradient sample of an n-element gradient (1 = stored whole); odd, so that every column is visited."""
    return 1 if n <= 1024 else (n // GRAD_SAMPLES) | 1


def load(z):
    """{case id: dict(loss, grad, stride, gmax)} from the arrays of criterions.npz (anything indexable by name)."""
    lo, go = z["loss_off"], z["grad_off"]
    return {str(i): dict(loss=z["loss"][lo[k]:lo[k + 1]], grad=z["grad"][go[k]:go[k + 1]], stride=int(z["stride"][k]), gmax=float(z["gmax"][k]))
            for k, i in enumerate(z["ids"])}


def restate64(c, inp):
    """The case in float64 torch, written from the formulas (not from the reference's code): (loss or per-row losses, d/d logits)."""
    import torch
    z = torch.from_numpy(inp["logits"]).double().requires_grad_(True)
    t = torch.from_numpy(inp["targets"])
    lsm = z - torch.logsumexp(z, dim=1, keepdim=True)
    if c["kind"] == "hard":
        rows = -lsm.gather(1, t.view(-1, 1)).squeeze(1)
    elif c["kind"] == "soft":
        rows = -(t.double() * lsm).sum(dim=1)
    elif c["kind"] == "mse":
        rows = ((lsm.exp() - t.double()) ** 2).sum(dim=1) / c["C"]
    else:
        rows = (z - t.double()).abs().sum(dim=1) / c["C"]
    for m in (inp["mask"], inp["mask2"]):
        if m is not None:
            rows = rows * torch.from_numpy(m).double()
    if c["reduction"] == "none":
        out = rows
    elif c["reduction"] == "sum" and c["kind"] == "hard":
        out = rows.sum()
    else:                                                    # 'mean', and the reference's soft-target branch for 'sum' too (cross_entropy.py:25-28)
        out = rows.sum() / c["B"]
    out.sum().backward()
    return out.detach().numpy(), z.grad.numpy()
