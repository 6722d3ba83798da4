"""Write tests/golden/device_data.npz: what the device loaders (semireward_amd/data/device_loader.py, csrc/resize.hip) are pinned to.

TEST INFRASTRUCTURE (build container only, like tools/gen_pretrained_golden.py): needs Pillow and the reference tree; the tests and everything
that runs on the GPU machine read only the fixture.  Arrays only:

  * resize/<n>/meta = (synth_image seed, H0, S, kind), resize/<n>/out = Image.resize((S, S), BILINEAR) of Pillow (version recorded in
    meta/pillow) on oracle.gen_golden.synth_image(seed, H0, H0, kind) -- transforms.Resize(S) of the reference's transforms on a PIL image;
  * sampler/<n>/meta = (n, total, replicas, rank, epoch), sampler/<n>/idx = list(iter(DistributedSampler)) of the reference's own class
    (semilearn/datasets/samplers/sampler.py) after set_epoch(epoch).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_device_data_golden.py
"""
import importlib.util
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import _ref_import as R  # noqa: E402
from oracle.gen_golden import synth_image  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "device_data.npz")
RESIZE_PAIRS = [(64, 32), (28, 32), (96, 32), (64, 96)]
SAMPLER_CASES = [            # (n, total, replicas, rank, epoch)
    (40, 24, 1, 0, 0),       # total < n
    (40, 24, 1, 0, 3),
    (40, 100, 1, 0, 0),      # total > 2 n, total % n != 0
    (40, 100, 4, 0, 3),
    (40, 100, 4, 1, 3),
    (40, 100, 4, 2, 3),
    (40, 100, 4, 3, 3),
    (2048, 640, 1, 0, 0),
    (2048, 640, 4, 2, 0),
    (37, 111, 1, 0, 3),      # total == 3 n: the truncated permutation is empty
    (50, 120, 4, 3, 0),
]


def reference_sampler_class():
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("_ref_sampler", os.path.join(R.REF, "semilearn", "datasets", "samplers", "sampler.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.DistributedSampler


def main():
    out = {"meta/pillow": np.array(PIL.__version__)}
    n = 0
    for H0, S in RESIZE_PAIRS:
        for kind in (0, 1, 2):                               # 0 = random noise, 1 = low-contrast texture, 2 = gradient + noise
            seed = 7000 + 10 * n + kind
            im = synth_image(seed, H0, H0, kind)
            out[f"resize/{n}/meta"] = np.array([seed, H0, S, kind], dtype=np.int64)
            out[f"resize/{n}/out"] = np.asarray(Image.fromarray(im).resize((S, S), Image.BILINEAR))
            n += 1
    out["meta/n_resize"] = np.array(n)
    DS = reference_sampler_class()
    for t, (nn, total, reps, rank, epoch) in enumerate(SAMPLER_CASES):
        s = DS(range(nn), num_replicas=reps, rank=rank, num_samples=total)
        s.set_epoch(epoch)
        out[f"sampler/{t}/meta"] = np.array([nn, total, reps, rank, epoch], dtype=np.int64)
        out[f"sampler/{t}/idx"] = np.array(list(iter(s)), dtype=np.int64)
    out["meta/n_sampler"] = np.array(len(SAMPLER_CASES))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
