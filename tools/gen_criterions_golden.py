"""Write tests/golden/criterions.npz with the REFERENCE's ce_loss / consistency_loss (build container only).

TEST INFRASTRUCTURE: imports the reference headless through oracle/_ref_import.py (as oracle/gen_golden.py does) and never runs on the GPU
machine.  Every case of tests/_criterions_cases.py runs on the CPU in fp32 with autograd.  Recorded per case: ``loss`` (the scalar, or the
[B] vector for reduction='none'), ``grad`` (d sum(loss) / d logits: whole up to 1024 elements, else the strided sample
``grad.ravel()[::stride]``), ``stride`` and ``gmax`` (the largest |gradient| of the case) -- concatenated over the cases (``ids``, ``loss_off``,
``grad_off``; tests/_criterions_cases.load splits them again).  Inputs are not stored: they are rebuilt from the seed.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_criterions_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import _ref_import as R  # noqa: E402
import _criterions_cases as CC  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "criterions.npz")


def main():
    ce_loss = R.mod("semilearn.core.criterions.cross_entropy").ce_loss
    consistency_loss = R.mod("semilearn.core.criterions.consistency").consistency_loss
    torch.set_num_threads(1)                                 # one summation order, whatever the machine
    ids, losses, grads, strides, gmax = [], [], [], [], []
    for c in CC.cases():
        inp = CC.inputs(c)
        z = torch.from_numpy(inp["logits"]).requires_grad_(True)
        t = torch.from_numpy(inp["targets"])
        if c["kind"] in ("hard", "soft"):
            loss = ce_loss(z, t, reduction=c["reduction"])
        else:
            m, m2 = (None if v is None else torch.from_numpy(v) for v in (inp["mask"], inp["mask2"]))
            loss = consistency_loss(z, t, c["kind"], m, m2)
        loss.sum().backward()
        g = z.grad.numpy()
        s = CC.grad_stride(g.size)
        ids.append(c["id"])
        losses.append(loss.detach().numpy().astype(np.float32).reshape(-1))
        grads.append(g.reshape(-1)[::s].copy())
        strides.append(s)
        gmax.append(np.abs(g).max())
    off = lambda parts: np.cumsum([0] + [p.size for p in parts]).astype(np.int64)   # noqa: E731
    np.savez_compressed(OUT, ids=np.array(ids), loss=np.concatenate(losses), loss_off=off(losses), grad=np.concatenate(grads),
                        grad_off=off(grads), stride=np.array(strides, np.int64), gmax=np.array(gmax, np.float32))
    print("wrote %s: %d cases, %d bytes" % (OUT, len(CC.cases()), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
