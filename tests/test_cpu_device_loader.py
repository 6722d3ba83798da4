"""device_data (semireward_amd/data/device_loader.py, csrc/resize.hip) without a GPU: the C ABI entry and its wrappers, the host coefficient
tables against Pillow's recorded outputs (tests/golden/device_data.npz, written by tools/gen_device_data_golden.py), the epoch sampler against
the reference's own DistributedSampler streams, the vectorised GpuAugment.pack against the loop it replaces, the loaders' bookkeeping with
the pixel launch stubbed, the new kernel's register budget, and the option's wiring into AlgorithmBase (refusals; nothing changes without it)."""
import argparse
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle.gen_golden import synth_image
from semireward_amd.core.algorithmbase import AlgorithmBase
from semireward_amd.core.hooks import DistSamplerSeedHook, EMAHook, ParamUpdateHook, TimerHook
from semireward_amd.data import augment as AUG
from semireward_amd.data import device_loader as DL
from semireward_amd.data.augment import DPN, IPN, OPS, RANGES, GpuAugment
from semireward_amd.data.resize import apply_tables, resize_tables
from semireward_amd.nets import bert, vit, wave2vec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)


# ---- 1. C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_resize_entry_and_ops_wraps_it():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srhip.h")).read(), flags=re.S)
    assert re.search(r"\bsrhip_resize_bilinear_u8\b", src)
    from semireward_amd import _lib, ops
    res, argtypes = _lib.SIGNATURES["srhip_resize_bilinear_u8"]
    decl = re.search(r"int\s+srhip_resize_bilinear_u8\s*\(([^)]*)\)", src).group(1)
    assert res is _lib.I and len(argtypes) == len(decl.split(","))
    assert callable(ops.resize_bilinear_u8)
    with pytest.raises(ValueError, match="square"):                       # refused on the Python side, before any launch
        ops.resize_bilinear_u8(torch.zeros(1, 8, 6, 3, dtype=torch.uint8), 4)
    with pytest.raises(ValueError, match="uint8"):
        ops.resize_bilinear_u8(torch.zeros(1, 8, 8, 3), 4)


# ---- 2. host tables == Pillow ---------------------------------------------------------------------------------------------------------------
def test_host_tables_reproduce_the_recorded_pillow_outputs(golden):
    g = golden("device_data")
    pairs = set()
    for n in range(int(g["meta/n_resize"])):
        seed, H0, S, kind = [int(v) for v in g[f"resize/{n}/meta"]]
        got = apply_tables(synth_image(seed, H0, H0, kind), S)
        assert np.array_equal(got, g[f"resize/{n}/out"]), (H0, S, kind)
        pairs.add((H0, S))
    assert pairs == {(64, 32), (28, 32), (96, 32), (64, 96)}


def test_host_tables_shape_and_identity():
    b, c, k = resize_tables(64, 32)                 # shrinking by 2: support 2, 5 taps, weights sum to 2^22 up to rounding
    assert k == 5 and b.shape == (32, 2) and c.shape == (32, 5) and b.dtype == c.dtype == np.int32
    assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= 64).all() and (b[:, 1] <= k).all()
    assert np.abs(c.sum(1) - (1 << 22)).max() <= k
    b, c, k = resize_tables(28, 32)                 # enlarging: support 1, 3 taps
    assert k == 3 and (b[:, 0] + b[:, 1] <= 28).all()
    im = synth_image(3, 32, 32, 0)
    assert np.array_equal(apply_tables(im, 32), im)  # H0 == S: Pillow skips both passes


def test_host_tables_against_live_pillow():
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    rng = np.random.Generator(np.random.PCG64(11))
    for H0, S in [(64, 32), (28, 32), (96, 32), (64, 96), (32, 224), (50, 17), (17, 50)]:
        im = rng.integers(0, 256, size=(H0, H0, 3), dtype=np.uint8)
        want = np.asarray(Image.fromarray(im).resize((S, S), Image.BILINEAR))
        assert np.array_equal(apply_tables(im, S), want), (H0, S, PIL.__version__)


# ---- 3. sampler -------------------------------------------------------------------------------------------------------------------------------
def test_epoch_sampler_equals_the_reference_streams(golden):
    g = golden("device_data")
    seen = set()
    for t in range(int(g["meta/n_sampler"])):
        n, total, reps, rank, epoch = [int(v) for v in g[f"sampler/{t}/meta"]]
        s = DL.EpochSampler(n, total, reps, rank)
        s.set_epoch(epoch)
        want = g[f"sampler/{t}/idx"]
        assert np.array_equal(s.indices(), want) and list(iter(s)) == want.tolist() and len(s) == len(want), (n, total, reps, rank, epoch)
        seen.add((total < n, total % n != 0, total > 2 * n, reps, epoch))
    assert {r for *_, r, _ in seen} == {1, 4} and {e for *_, e in seen} == {0, 3}
    assert any(a for a, *_ in seen) and any(b for _, b, *_ in seen) and any(c for _, _, c, *_ in seen)


def test_epoch_sampler_ranks_partition_and_epochs_differ():
    n, total, reps = 40, 96, 4
    whole = DL.EpochSampler(n, total, 1, 0)
    whole.set_epoch(2)
    parts = []
    for r in range(reps):
        s = DL.EpochSampler(n, total, reps, r)
        s.set_epoch(2)
        parts.append(s.indices())
        assert len(parts[-1]) == total // reps
    inter = np.stack(parts, 1).reshape(-1)                     # rank r holds stream[r::reps]
    assert np.array_equal(inter, whole.indices())
    other = DL.EpochSampler(n, total, 1, 0)
    other.set_epoch(3)
    assert not np.array_equal(other.indices(), whole.indices())
    # labelled and unlabelled samplers of one epoch share the seed: with equal n, the shorter stream is a prefix of the longer one
    lb, ulb = DL.EpochSampler(n, 16, 1, 0), DL.EpochSampler(n, 32, 1, 0)
    lb.set_epoch(5), ulb.set_epoch(5)
    assert np.array_equal(lb.indices(), ulb.indices()[:16])
    with pytest.raises(ValueError, match="evenly"):
        DL.EpochSampler(n, 10, 4, 0)
    with pytest.raises(ValueError, match="positive"):
        DL.EpochSampler(n, 0, 1, 0)


# ---- 4. pack: the loop it replaces, verbatim, as the yardstick -------------------------------------------------------------------------------
def _fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def _affine_matrix(op, v, S):
    name = OPS[op]
    if name == "Rotate":                    # Image.rotate: inverse matrix about the centre, entries rounded to 15 decimals
        ang = -math.radians(v % 360.0)
        m = [round(math.cos(ang), 15), round(math.sin(ang), 15), 0.0, round(-math.sin(ang), 15), round(math.cos(ang), 15), 0.0]
        c = S / 2.0
        m[2] = m[0] * (-c) + m[1] * (-c) + m[2]
        m[5] = m[3] * (-c) + m[4] * (-c) + m[5]
        m[2] += c; m[5] += c
        return m
    return {"ShearX": [1, v, 0, 0, 1, 0], "ShearY": [1, 0, 0, v, 1, 0], "TranslateX": [1, 0, v * S, 0, 1, 0],
            "TranslateY": [1, 0, 0, 0, 1, v * S]}[name]


def _pack_loop(S, d, src_index=None):
    B = len(d["i"])
    ip, dp = np.zeros((B, IPN), dtype=np.int32), np.zeros((B, DPN), dtype=np.float64)
    ip[:, 0], ip[:, 1], ip[:, 2] = d["i"], d["j"], d["flip"]
    ip[:, 4] = -1
    ip[:, 8] = np.arange(B) if src_index is None else src_index
    if "ops" in d:
        n = d["ops"].shape[1]
        ip[:, 3] = n
        for b in range(B):
            for k in range(n):
                op, v = int(d["ops"][b, k]), float(d["vals"][b, k])
                q, e = ip[b, 16 + 12 * k:], dp[b, 8 * k:]
                q[0], e[0] = op, v
                if OPS[op] == "Posterize":
                    q[8] = ~(2 ** (8 - max(1, int(v))) - 1) & 0xFF
                elif OPS[op] in ("Rotate", "ShearX", "ShearY", "TranslateX", "TranslateY"):
                    a = _affine_matrix(op, v, S)
                    if a[1] == 0 and a[3] == 0:            # Pillow: ImagingScaleAffine (float64 walk)
                        q[1], e[1], e[2], e[3], e[4] = 1, a[2] + a[0] * 0.5, a[5] + a[4] * 0.5, a[0], a[4]
                    else:                                  # Pillow: affine_fixed (16.16)
                        q[2:8] = [_fix(a[0]), _fix(a[1]), _fix(a[2] + a[0] * 0.5 + a[1] * 0.5), _fix(a[3]), _fix(a[4]),
                                  _fix(a[5] + a[3] * 0.5 + a[4] * 0.5)]
            cv = float(d["cut_v"][b])                      # Cutout / CutoutAbs (randaugment.py:116-146)
            if cv > 0.0:
                v = cv * S
                x0, y0 = int(max(0, float(d["ux"][b]) - v / 2.0)), int(max(0, float(d["uy"][b]) - v / 2.0))
                ip[b, 4:8] = [x0, y0, int(min(S, x0 + v)), int(min(S, y0 + v))]
    return ip, dp


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()        # bit for bit (the sign of a zero included)


@pytest.mark.parametrize("S,pad,n_ops", [(32, 4, 3), (96, 12, 3), (224, 28, 4), (32, 4, 1)])
def test_vectorised_pack_equals_the_loop(S, pad, n_ops):
    assert AUG.OPS == OPS and (IPN, DPN) == (64, 32)
    aug = GpuAugment(S, pad, MEAN, STD, n_ops=n_ops, device="cpu", seed=S + n_ops)
    total = 0
    for rep in range(4):
        B = 160
        d = aug.draw(B, True)
        if rep == 1:            # every op in turn; Rotate at multiples of 90 degrees (sin / cos round to 0 / +-1: the float64 walk) and near
            d["ops"] = (np.arange(B * n_ops).reshape(B, n_ops) + rep) % len(OPS)
            lo = np.array([a for a, _ in RANGES], dtype=np.float64)[d["ops"]]
            hi = np.array([b for _, b in RANGES], dtype=np.float64)[d["ops"]]
            d["vals"] = lo + (hi - lo) * aug.rng.random((B, n_ops))        # magnitudes of the ops' own ranges
            rot = d["ops"] == OPS.index("Rotate")
            d["vals"][rot] = np.resize(np.array([0.0, 90.0, 180.0, 270.0, 360.0, -90.0, -180.0, 1e-13, 89.99999999999999, 30.0, -30.0]), rot.sum())
        if rep == 2:            # zero magnitudes (Shear 0 is the float64 walk; Translate 0), range ends, zero / full cutout
            lo = np.array([a for a, _ in RANGES], dtype=np.float64)[d["ops"]]
            hi = np.array([b for _, b in RANGES], dtype=np.float64)[d["ops"]]
            d["vals"] = np.where(np.arange(B)[:, None] % 3 == 0, 0.0, np.where(np.arange(B)[:, None] % 3 == 1, lo, hi))
            d["vals"][d["ops"] == OPS.index("Posterize")] = np.resize(np.array([4.0, 4.999, 5.0, 7.999, 8.0, 1.0, 0.0]),
                                                                       (d["ops"] == OPS.index("Posterize")).sum())
            d["cut_v"][::2] = 0.0
            d["cut_v"][1::4] = 0.5
            d["ux"][::5], d["uy"][::7] = 0.0, float(S)
        src = None if rep % 2 else aug.rng.integers(0, 1000, size=B)
        got, want = aug.pack(d, src), _pack_loop(S, d, src)
        assert _same(got[0], want[0]) and _same(got[1], want[1]), (S, rep, np.argwhere(got[0] != want[0])[:4], np.argwhere(got[1] != want[1])[:4])
        total += B * n_ops
    d = aug.draw(16, False)                                     # weak view: no op blocks
    assert all(_same(a, b) for a, b in zip(aug.pack(d), _pack_loop(S, d)))
    assert total >= 4 * 160


def test_pack_refuses_coefficients_outside_int32_like_the_loop():
    aug = GpuAugment(32, 4, MEAN, STD, n_ops=1, device="cpu")
    d = aug.draw(2, True)
    d["ops"][:] = OPS.index("ShearX")
    d["vals"][:] = 1e6
    with pytest.raises(OverflowError):
        _pack_loop(32, d)
    with pytest.raises(OverflowError):
        aug.pack(d)


def test_vectorised_pack_draw_count():
    """>= 2000 random draws in one go, every op present."""
    aug = GpuAugment(32, 4, MEAN, STD, n_ops=3, device="cpu", seed=99)
    d = aug.draw(1000, True)
    assert set(np.unique(d["ops"])) == set(range(len(OPS))) and d["ops"].size >= 2000
    got, want = aug.pack(d), _pack_loop(32, d)
    assert _same(got[0], want[0]) and _same(got[1], want[1])


# ---- 5. loader bookkeeping, pixel launch stubbed -------------------------------------------------------------------------------------------------
class _StubAugment(GpuAugment):
    """GpuAugment with the launch replaced by a record: what would be drawn and launched, and a stand-in view that names its sources."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.calls = []

    def __call__(self, src_u8, strong, draws=None, src_index=None, return_u8=False):
        d = draws if draws is not None else self.draw(len(src_index), strong, tuple(src_u8.shape[1:3]))
        self.calls.append((bool(strong), np.array(src_index), d))
        return torch.as_tensor(np.array(src_index), dtype=torch.float32).view(-1, 1, 1, 1).expand(-1, 3, self.size, self.size)


def _dataset(n, S=8, labelled=True, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return DL.DeviceImageDataset(rng.integers(0, 256, size=(n, S, S, 3), dtype=np.uint8), rng.integers(0, 10, size=n) if labelled else None, S, "cpu")


def test_train_loader_chunks_the_sampler_stream():
    ds = _dataset(20)
    aug = _StubAugment(8, 1, MEAN, STD, device="cpu")
    ld = DL.DeviceTrainLoader(ds, 6, DL.EpochSampler(20, 45, 1, 0), aug, strong=True, keys=("idx_lb", "x_lb", "y_lb"), seed=(1, 0, 0))
    assert len(ld) == 45 // 6                                   # drop_last
    for epoch in (0, 2):
        ld.set_epoch(epoch)
        ref = DL.EpochSampler(20, 45, 1, 0)
        ref.set_epoch(epoch)
        stream = ref.indices()
        aug.calls.clear()
        got = list(ld)
        assert len(got) == len(ld) == 7
        for t, b in enumerate(got):
            assert list(b) == ["idx_lb", "x_lb", "y_lb"]
            assert np.array_equal(b["idx_lb"].numpy(), stream[6 * t:6 * t + 6]) and b["idx_lb"].dtype == torch.int64
            assert np.array_equal(b["y_lb"].numpy(), ds.targets_host[stream[6 * t:6 * t + 6]]) and b["y_lb"].dtype == torch.int64
            assert b["x_lb"].shape == (6, 3, 8, 8) and np.array_equal(b["x_lb"][:, 0, 0, 0].numpy(), stream[6 * t:6 * t + 6])
        assert [c[0] for c in aug.calls] == [False] * 7         # one weak launch per step
    first = [c[2]["i"].copy() for c in aug.calls]
    aug.calls.clear()
    list(ld)                                                    # the same epoch again: the same draws
    assert all(np.array_equal(a, c[2]["i"]) for a, c in zip(first, aug.calls))
    ld.set_epoch(3)
    aug.calls.clear()
    list(ld)
    assert not all(np.array_equal(a, c[2]["i"]) for a, c in zip(first, aug.calls))


def test_unlabelled_loader_views_follow_the_step_signature():
    ds = _dataset(30, labelled=False)
    keys = ("idx_ulb", "x_ulb_w", "x_ulb_s")
    aug = _StubAugment(8, 1, MEAN, STD, device="cpu")
    ld = DL.DeviceTrainLoader(ds, 4, DL.EpochSampler(30, 12, 1, 0), aug, strong=True, keys=keys, seed=(1, 0, 1))
    got = list(ld)
    assert len(got) == 3 and all(list(b) == list(keys) for b in got)
    assert [c[0] for c in aug.calls] == [False, True] * 3      # weak then strong: two independent draws on the same stored images
    for w, s in zip(aug.calls[0::2], aug.calls[1::2]):
        assert np.array_equal(w[1], s[1]) and "ops" in s[2] and "ops" not in w[2]
    aug2 = _StubAugment(8, 1, MEAN, STD, device="cpu")
    ld2 = DL.DeviceTrainLoader(ds, 4, DL.EpochSampler(30, 12, 1, 0), aug2, strong=False, keys=keys, seed=(1, 0, 1))
    got2 = list(ld2)
    assert all(list(b) == ["idx_ulb", "x_ulb_w"] for b in got2) and [c[0] for c in aug2.calls] == [False] * 3      # no strong view: not drawn, not launched
    assert all(np.array_equal(a["idx_ulb"].numpy(), b["idx_ulb"].numpy()) for a, b in zip(got, got2))
    with pytest.raises(ValueError, match="labelled"):
        DL.DeviceTrainLoader(ds, 4, DL.EpochSampler(30, 12, 1, 0), aug, keys=("idx_lb", "x_lb", "y_lb"))


def test_eval_loader_keeps_the_partial_batch():
    ds = _dataset(11)
    aug = _StubAugment(8, 0, MEAN, STD, device="cpu")
    ld = DL.DeviceEvalLoader(ds, 4, aug)
    for _ in range(2):                                          # re-iterable, one augment object for every batch
        aug.calls.clear()
        got = list(ld)
        assert len(ld) == 3 and [int(b["y_lb"].shape[0]) for b in got] == [4, 4, 3] and all(list(b) == ["x_lb", "y_lb"] for b in got)
        assert np.array_equal(np.concatenate([b["y_lb"].numpy() for b in got]), ds.targets_host)
        assert np.array_equal(np.concatenate([c[1] for c in aug.calls]), np.arange(11))
        for strong, _, d in aug.calls:                          # transform_val: no crop shift, no flip, no op
            assert not strong and not d["i"].any() and not d["j"].any() and not d["flip"].any() and "ops" not in d
    with pytest.raises(ValueError, match="labelled"):
        DL.DeviceEvalLoader(_dataset(5, labelled=False), 4, aug)


def test_device_image_dataset_inputs():
    rng = np.random.Generator(np.random.PCG64(1))
    u8 = rng.integers(0, 256, size=(5, 8, 8, 3), dtype=np.uint8)
    ds = DL.DeviceImageDataset(torch.from_numpy(u8), torch.arange(5), 8, "cpu")
    assert len(ds) == 5 and ds.data.dtype == torch.uint8 and np.array_equal(ds.data.numpy(), u8) and ds.targets.dtype == torch.int64

    class Ref:                                                  # duck-typed reference dataset: an unlabelled split carries no targets
        data, targets, is_ulb = u8, [1, 2, 3, 4, 5], True
    assert DL.DeviceImageDataset.from_reference(Ref, 8, "cpu").targets is None
    Ref.is_ulb = False
    assert DL.DeviceImageDataset.from_reference(Ref, 8, "cpu").targets.tolist() == [1, 2, 3, 4, 5]
    assert DL.DeviceImageDataset.from_reference({"data": u8, "targets": None}, 8, "cpu").targets is None
    assert DL.DeviceImageDataset.from_reference(ds, 8, "cpu") is ds
    with pytest.raises(ValueError, match="uint8"):
        DL.DeviceImageDataset(u8.astype(np.float32), None, 8, "cpu")
    with pytest.raises(ValueError, match="decoded uint8"):           # a dataset that keeps file paths (the reference's EuroSat): refused with the reason
        DL.DeviceImageDataset(np.array(["a/0.jpg", "a/1.jpg"]), None, 8, "cpu")
    with pytest.raises(ValueError, match="decoded uint8"):
        DL.DeviceImageDataset(["a/0.jpg", "a/1.jpg"], None, 8, "cpu")
    with pytest.raises(ValueError, match="uint8"):
        DL.DeviceImageDataset(torch.zeros(2, 8, 8, 3), None, 8, "cpu")
    with pytest.raises(ValueError, match="square"):
        DL.DeviceImageDataset(u8[:, :, :6], None, 8, "cpu")
    with pytest.raises(ValueError, match=r"\[n, H, W, 3\]"):
        DL.DeviceImageDataset(u8[..., :1], None, 8, "cpu")
    with pytest.raises(ValueError, match="one label per image"):
        DL.DeviceImageDataset(u8, [0, 1], 8, "cpu")


# ---- 6. register budget ------------------------------------------------------------------------------------------------------------------------
def test_resize_kernel_keeps_its_register_budget(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "semireward_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-c",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "o.o"), os.path.join(csrc, "resize.hip")],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    k = {n: v for n, v in out.items() if "resize_bilinear_u8_kernel" in n}
    assert len(k) == 1 and len(out) == 2, sorted(out)
    for n, v in out.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (n, v)


# ---- 7. wiring -----------------------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    d = dict(algorithm="hostonly", num_classes=10, num_train_iter=6, epoch=2, ema_m=0.0, ulb_loss_ratio=1.0, use_cat=True, amp=False, lr=5e-4,
             num_eval_iter=0, num_log_iter=0, gpu=None, rank=0, world_size=1, distributed=False, dataset="eurosat", num_labels=12, batch_size=4,
             uratio=2, eval_batch_size=4, train_sampler="RandomSampler", img_size=8, crop_ratio=0.875, seed=3, data_functions=(None, None))
    d.update(kw)
    return argparse.Namespace(**d)


def _dicts(S=8, dtype=np.uint8, W=None):
    rng = np.random.Generator(np.random.PCG64(2))
    mk = lambda n: rng.integers(0, 256, size=(n, S, W or S, 3)).astype(dtype)      # noqa: E731
    return {"train_lb": {"data": mk(12), "targets": rng.integers(0, 10, size=12)}, "train_ulb": {"data": mk(40), "targets": None},
            "eval": {"data": mk(6), "targets": rng.integers(0, 10, size=6)}, "test": None}


class _HostOnly(AlgorithmBase):
    """The base class's wiring with a backbone that is never launched (CPU device) and no optimizer."""
    net = staticmethod(lambda nc: vit.VisionTransformer(vit.VitConfig(img_size=8, patch_size=2, embed_dim=128, depth=2, num_heads=2, num_classes=nc),
                                                        device="cpu"))

    def set_model(self):
        return self.net(self.num_classes)

    def set_ema_model(self):
        return self.model

    def set_optimizer(self):
        return None, None

    def train_step(self, x_lb, y_lb, idx_ulb, x_ulb_w, x_ulb_s):
        raise AssertionError("not stepped")


class _HostOnlyWeak(_HostOnly):
    def train_step(self, x_lb, y_lb, x_ulb_w):
        raise AssertionError("not stepped")


def test_option_absent_changes_nothing():
    for kw in (dict(), dict(device_data=False)):
        alg = _HostOnly(_args(dataset=None, **kw), None)
        assert alg.dataset_dict is None and alg.loader_dict is None
        assert [type(h) for h in alg.hooks_dict.values()] == [ParamUpdateHook, EMAHook, TimerHook]
        assert list(alg.hooks_dict) == ["ParamUpdateHook", "EMAHook", "TimerHook"]
    ld = {"train_lb": [], "train_ulb": []}
    assert _HostOnly(_args(dataset=None, loader_dict=ld), None).loader_dict is ld
    with pytest.raises(RuntimeError, match="get_data_loader"):                       # a dataset_dict without the option: today's error
        _HostOnly(_args(dataset_dict=_dicts()), None)


def test_option_builds_the_device_loaders_and_the_seed_hook():
    a = _args(device_data=True, dataset_dict=_dicts())
    alg = _HostOnly(a, None)
    assert a.ulb_dest_len == 40 and a.lb_dest_len == 12
    assert set(alg.loader_dict) == {"train_lb", "train_ulb", "eval"}
    lb, ulb, ev = alg.loader_dict["train_lb"], alg.loader_dict["train_ulb"], alg.loader_dict["eval"]
    assert isinstance(lb, DL.DeviceTrainLoader) and isinstance(ev, DL.DeviceEvalLoader)
    assert (lb.batch_size, ulb.batch_size, ev.batch_size) == (4, 8, 4) and len(lb) == len(ulb) == 3         # 6 iterations over 2 epochs
    assert (lb.sampler.total, ulb.sampler.total) == (3 * 4, 3 * 8)
    assert lb.keys == ("idx_lb", "x_lb", "y_lb") and ulb.keys == ("idx_ulb", "x_ulb_w", "x_ulb_s")
    assert (lb.aug.size, lb.aug.pad, ev.aug.pad) == (8, int(8 * (1 - 0.875)), 0) and lb.aug is not ulb.aug
    assert tuple(lb.aug.mean) == (0.5, 0.5, 0.5)                                                            # eurosat statistics
    assert lb.seed == (3, 0, 0) and ulb.seed == (3, 0, 1)
    assert [type(h) for h in alg.hooks_dict.values()].count(DistSamplerSeedHook) == 1 and len(alg.hooks_dict) == 4
    alg.epoch = 1
    alg.call_hook("before_train_epoch")
    assert lb.epoch == ulb.epoch == lb.sampler.epoch == ulb.sampler.epoch == 1
    # a train_step without x_ulb_s (srpseudolabel): the strong view is not part of the loader
    assert _HostOnlyWeak(_args(device_data=True, dataset_dict=_dicts()), None).loader_dict["train_ulb"].keys == ("idx_ulb", "x_ulb_w")
    # statistics: args.dataset_mean / dataset_std win; an unknown dataset without them is refused
    a2 = _args(device_data=True, dataset_dict=_dicts(), dataset="mine", dataset_mean=(0.1, 0.2, 0.3), dataset_std=(0.4, 0.5, 0.6))
    assert tuple(round(float(v), 6) for v in _HostOnly(a2, None).loader_dict["eval"].aug.std) == (0.4, 0.5, 0.6)
    assert DL.dataset_stats(_args(dataset="cifar100"))[0] == [x / 255 for x in (129.3, 124.1, 112.4)]


def test_option_refusals_name_their_reason():
    with pytest.raises(NotImplementedError, match="train_sampler 'WeightedRandomSampler'"):
        _HostOnly(_args(device_data=True, dataset_dict=_dicts(), train_sampler="WeightedRandomSampler"), None)
    with pytest.raises(ValueError, match="uint8"):
        _HostOnly(_args(device_data=True, dataset_dict=_dicts(dtype=np.float32)), None)
    with pytest.raises(ValueError, match="square"):
        _HostOnly(_args(device_data=True, dataset_dict=_dicts(W=6)), None)
    with pytest.raises(RuntimeError, match="needs the dataset arrays"):
        _HostOnly(_args(device_data=True, dataset=None), None)
    with pytest.raises(ValueError, match="no Normalize statistics"):
        _HostOnly(_args(device_data=True, dataset_dict=_dicts(), dataset="mine"), None)

    class Tokens(_HostOnly):
        net = staticmethod(lambda nc: bert.ClassificationBert(bert.BertConfig(vocab=120, hidden=128, layers=2, heads=2, inter=512, max_pos=64,
                                                                             num_classes=nc), device="cpu"))

    class Waves(_HostOnly):
        net = staticmethod(lambda nc: wave2vec.ClassificationWave2Vec(
            wave2vec.W2vConfig(hidden=128, layers=2, heads=2, inter=256, conv_dim=(128, 128, 128), conv_kernel=(10, 3, 2), conv_stride=(5, 2, 2),
                               pos_k=16, pos_groups=4, num_classes=nc), device="cpu"))
    # decided from the yaml's net name, before the dataset is looked at (a usb_nlp / usb_audio dataset_dict holds no image arrays)
    for net, why in (("bert_base_uncased", "token batches"), ("wave2vecv2_base", "waveforms"), ("hubert_base", "waveforms")):
        with pytest.raises(NotImplementedError, match=why):
            _HostOnly(_args(device_data=True, net=net, dataset_dict={"train_lb": {"data": ["some text"], "targets": [0]}}), None)
    assert _HostOnly(_args(device_data=True, net="vit_small_patch2_32", dataset_dict=_dicts()), None).loader_dict is not None
    # ... and from the model, for a builder handed in without a net name
    with pytest.raises(NotImplementedError, match="token batches"):
        Tokens(_args(device_data=True, dataset_dict=_dicts()), None)
    with pytest.raises(NotImplementedError, match="waveforms"):
        Waves(_args(device_data=True, dataset_dict=_dicts()), None)
