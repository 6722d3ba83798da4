"""device_audio (semireward_amd/data/device_audio.py, csrc/wave_view.hip) without a GPU: the C ABI entry, its wrapper and its argument refusals;
the float64 oracle of a view (tests/_wave_view_cases.py) against transformers' recorded float32 outputs and the reference's recorded
random_subsample offsets (tests/golden/device_audio.npz, written by tools/device_audio_golden.py); the store's packing; the loaders' bookkeeping
with the launch stubbed by the oracle; the option's wiring into AlgorithmBase (refusals; nothing changes without it); the kernel's registers."""
import argparse
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _wave_view_cases as WC
from semireward_amd import _lib, ops
from semireward_amd.core.algorithmbase import AlgorithmBase
from semireward_amd.core.hooks import DistSamplerSeedHook, EMAHook, ParamUpdateHook, TimerHook
from semireward_amd.data import device_audio as DA
from semireward_amd.data.device_loader import EpochSampler
from semireward_amd.nets import hubert, vit, wave2vec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_signature_and_wrapper_agree(monkeypatch):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srhip.h")).read(), flags=re.S)
    decl = re.search(r"int\s+srhip_wave_view\s*\(([^)]*)\)", src).group(1)
    res, argtypes = _lib.SIGNATURES["srhip_wave_view"]
    assert res is _lib.I and len(argtypes) == len(decl.split(",")) == 12
    kinds = [_lib.P if "*" in a else _lib.I for a in decl.split(",")]
    assert kinds == argtypes                                                     # pointer / int, position by position
    sent = []
    monkeypatch.setattr(ops, "_call", lambda name, *a: sent.append((name, a)))
    monkeypatch.setattr(ops, "_p", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(ops, "_s", lambda: None)
    store, off, ln = torch.zeros(16), torch.tensor([0, 8]), torch.tensor([5, 8], dtype=torch.int32)
    out = ops.wave_view(store, off, ln, torch.tensor([1, 0, 1]), torch.tensor([0, 1, 2], dtype=torch.int32), 6, True,
                        host=(np.array([1, 0, 1]), np.array([0, 1, 2]), np.array([5, 8])))
    (name, a), = sent
    assert name == "srhip_wave_view" and len(a) == len(argtypes)
    assert a[3] == 2 and a[6:9] == (3, 6, 1) and a[10] == 8 and out.shape == (3, 6) and out.stride() == (8, 1)       # n_rows, B, S, normalize, ldo
    assert ops.wave_view(store, off, ln, torch.tensor([0]), torch.tensor([0], dtype=torch.int32), 8, False).is_contiguous() and sent[1][1][8] == 0
    for bad, why in (((np.array([2]), np.array([0]), np.array([5, 8])), "src_row outside"), ((np.array([-1]), np.array([0]), np.array([5, 8])), "src_row outside"),
                     ((np.array([0]), np.array([5]), np.array([5, 8])), "crop_off outside"), ((np.array([1]), np.array([-1]), np.array([5, 8])), "crop_off outside")):
        with pytest.raises(IndexError, match=why):                               # refused on the host, where the draws are produced
            ops.check_wave_rows(*bad)
    with pytest.raises(ValueError, match="int64"):
        ops.wave_view(store, off, ln, torch.tensor([0], dtype=torch.int32), torch.tensor([0], dtype=torch.int32), 8, False)
    with pytest.raises(ValueError, match="fp32"):
        ops.wave_view(store.double(), off, ln, torch.tensor([0]), torch.tensor([0], dtype=torch.int32), 8, False)


def test_entry_refuses_each_bad_argument():
    f = _lib.lib().srhip_wave_view
    buf = (ctypes.c_float * 64)()
    a = (ctypes.addressof(buf) + 15) & ~15                                       # a 16-byte aligned host address: never dereferenced, every call is refused first
    ok = dict(store=a, row_off=a, row_len=a, n_rows=2, src_row=a, crop_off=a, B=2, S=6, normalize=1, out=a, ldo=8, stream=None)

    def rc(**kw):
        return f(*{**ok, **kw}.values())
    for k in ("store", "row_off", "row_len", "src_row", "crop_off", "out"):
        assert rc(**{k: None}) == -1, k                                          # SR_EINVAL
    for kw in (dict(B=0), dict(B=-3), dict(B=65536), dict(S=0), dict(S=-1), dict(S=9), dict(ldo=4), dict(ldo=7), dict(S=5, ldo=6), dict(out=a + 4),
               dict(out=a + 8), dict(n_rows=0), dict(normalize=2), dict(S=(1 << 30) + 4, ldo=(1 << 30) + 4)):
        assert rc(**kw) == -1, kw


# ---- 2. the oracle against the recorded extractor outputs and the reference's offsets ----------------------------------------------------------
@pytest.mark.parametrize("name", sorted(WC.FIXTURE_BATCHES))
def test_oracle_equals_the_recorded_extractor_outputs(golden, name):
    """The bound here is the extractor's own float32 arithmetic: a pairwise mean, a subtraction, a pairwise second moment, an addition, a
    square root and a divide, each within an ulp of the largest magnitude involved -- 16 ulp_fp32(max |out|) in all (printed: what it measures)."""
    g, f = golden("device_audio"), WC.FIXTURE_BATCHES[name]
    S, clips, offs = f["S"], WC.fixture_clips(name), g[f"fx/{name}/offsets"]
    rows, crop = np.arange(len(clips)), offs[0]

    def check(got, r, width, what):
        want = WC.oracle(clips, r, crop[r], width, True)
        assert got.dtype == np.float32 and got.shape == want.shape, what
        d, tol = np.abs(got - want).max(), 16 * WC.ulp32(np.abs(want).max())
        print("%s %s: max |extractor - oracle| = %.3g (%.2f ulp), bound %.3g" % (name, what, d, d / WC.ulp32(np.abs(want).max()), tol))
        assert d <= tol, (what, d, tol)
        return want
    want = check(g[f"fx/{name}/pad_max"], rows, S, "pad_max")
    check(g[f"fx/{name}/pad_true"], rows, S, "pad_true")                          # the batch holds a clip of at least S samples: padding=True pads to S too
    short = np.array(f["short"])
    longest = max(len(clips[i]) for i in short)
    assert longest < S
    check(g[f"fx/{name}/pad_true_short"], short, longest, "pad_true_short")       # ... and to the batch's own longest row otherwise
    # the padded positions are normalised with the rest: -m / sigma, not 0
    for b, c in enumerate(clips):
        n = min(len(c) - crop[b], S)
        if n < S:
            v = np.zeros(S)
            v[:n] = c[crop[b]:crop[b] + n]
            m, sd = v.mean(), np.sqrt(v.var() + 1e-7)
            assert np.allclose(want[b, n:], -m / sd, rtol=1e-12, atol=0) and abs(m / sd) > 1e-3
            assert np.abs(g[f"fx/{name}/pad_max"][b, n:] - np.float32(-m / sd)).max() <= 16 * WC.ulp32(np.abs(want).max())


@pytest.mark.parametrize("name", sorted(WC.FIXTURE_BATCHES))
def test_offset_rule_is_the_references(golden, name):
    f, offs = WC.FIXTURE_BATCHES[name], golden("device_audio")[f"fx/{name}/offsets"]
    S, lens = f["S"], np.array(f["lens"])
    assert offs.shape == (WC.N_OFFSET_SEEDS, len(lens))
    for i, n in enumerate(lens):
        if n <= S:
            assert not offs[:, i].any()                                          # the clip whole
        else:
            assert offs[:, i].min() >= 0 and offs[:, i].max() <= n - S - 1       # the last window (offset len - L) is never drawn
            if n - S <= 16:
                assert set(offs[:, i].tolist()) == set(range(n - S))             # ... and every other one is (400 draws over <= 16 values)
    rng = np.random.Generator(np.random.PCG64(5))
    draws = np.stack([DA.crop_offsets(rng, lens, S) for _ in range(WC.N_OFFSET_SEEDS)])
    assert draws.dtype == np.int32
    for i, n in enumerate(lens):                                                 # the loader's rule: the same support
        assert (set(draws[:, i].tolist()) == {0}) if n <= S else (draws[:, i].min() >= 0 and draws[:, i].max() <= n - S - 1)
        if S < n <= S + 16:
            assert set(draws[:, i].tolist()) == set(range(n - S))
    assert int(draws[:, lens > S + 16].max()) > 16


def test_fixture_is_arrays_only_and_small(golden):
    g = golden("device_audio")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "device_audio.npz")) < 200 * 1024
    names = {c["name"] for c in WC.kernel_cases()}
    assert {k.split("/", 1)[1].rsplit("/", 1)[0] for k in g.keys("kernel/")} == names and len(names) == len(WC.KERNEL_S) * len(WC.GEOMETRIES)
    assert all(g[k].dtype.kind in "fiuU" for k in g.keys())
    for c in WC.kernel_cases():                                                  # the geometries promise: every phase, n = S, n < S, n = 1
        lens = np.array([len(x) for x in c["clips"]])
        n = np.minimum(lens[c["src_row"]] - c["crop_off"], c["S"])
        assert (n >= 1).all() and (c["crop_off"] < lens[c["src_row"]]).all()
        if c["name"].endswith("b5a"):
            assert set((c["crop_off"] % 4).tolist()) == {0, 1, 2, 3} and n.max() == c["S"] and n.min() == 1 and len(set(c["src_row"].tolist())) < 5
            assert c["S"] < 3 or (n < c["S"]).sum() >= 2


# ---- 3. packing ---------------------------------------------------------------------------------------------------------------------------------
def test_store_packing_and_refusals():
    clips = [WC.clip(i, n) for i, n in enumerate((5, 8, 1, 13))]
    var = [[WC.clip(10 * (v + 1) + i, n) for i, n in enumerate((7, 3, 2, 9))] for v in range(2)]
    ds = DA.DeviceWaveDataset(clips, [3, 1, 0, 2], "cpu", data_s=var)
    assert len(ds) == 4 and ds.n_variants == 2 and ds.store.dtype == torch.float32 and ds.row_off.dtype == torch.int64 and ds.row_len.dtype == torch.int32
    assert ds.row_len_host.tolist() == [5, 8, 1, 13, 7, 3, 2, 9, 7, 3, 2, 9] and (ds.row_off_host % 4 == 0).all()
    assert ds.row_off_host.tolist() == np.concatenate([[0], np.cumsum((ds.row_len_host + 3) // 4 * 4)[:-1]]).tolist()
    assert np.array_equal(ds.row_off.numpy(), ds.row_off_host) and np.array_equal(ds.row_len.numpy(), ds.row_len_host)
    flat = ds.store.numpy()
    assert flat.size == int(((ds.row_len_host + 3) // 4 * 4).sum())
    for r, c in enumerate(clips + var[0] + var[1]):                              # variants sit in their own rows, after the clips
        o = ds.row_off_host[r]
        assert np.array_equal(flat[o:o + c.size], c) and not flat[o + c.size:o + (c.size + 3) // 4 * 4].any()
    assert ds.strong_row([0, 1, 1], [2, 0, 3]).tolist() == [4 + 2, 8 + 0, 8 + 3]
    assert ds.targets.tolist() == [3, 1, 0, 2] and ds.targets.dtype == torch.int64
    back = WC.store_clips(ds)
    assert all(np.array_equal(a, b) for a, b in zip(back, clips + var[0] + var[1]))

    class Ref:                                                                   # duck-typed reference BasicDataset: an unlabelled split carries no targets
        data, targets, is_ulb = [c.astype(np.float64) for c in clips], [1, 2, 3, 0], True
    assert DA.DeviceWaveDataset.from_reference(Ref, "cpu").targets is None and DA.DeviceWaveDataset.from_reference(Ref, "cpu").n_variants == 0
    Ref.is_ulb = False
    assert DA.DeviceWaveDataset.from_reference(Ref, "cpu").targets.tolist() == [1, 2, 3, 0]
    assert DA.DeviceWaveDataset.from_reference({"data": clips, "targets": None, "data_s": var}, "cpu").n_variants == 2
    assert DA.DeviceWaveDataset.from_reference(ds, "cpu") is ds
    with pytest.raises(ValueError, match="float waveforms"):
        DA.DeviceWaveDataset([np.arange(4)], None, "cpu")
    with pytest.raises(ValueError, match="float waveforms"):                     # a dataset that keeps file paths
        DA.DeviceWaveDataset(["a/0.wav"], None, "cpu")
    with pytest.raises(ValueError, match="1-D"):
        DA.DeviceWaveDataset([np.zeros((2, 4), dtype=np.float32)], None, "cpu")
    with pytest.raises(ValueError, match="clip 1 of data is empty"):
        DA.DeviceWaveDataset([clips[0], np.zeros(0, dtype=np.float32)], None, "cpu")
    with pytest.raises(ValueError, match="one label per clip"):
        DA.DeviceWaveDataset(clips, [0, 1], "cpu")
    with pytest.raises(ValueError, match=r"data_s\[1\] must hold one variant of every clip"):
        DA.DeviceWaveDataset(clips, None, "cpu", data_s=[var[0], var[1][:3]])
    with pytest.raises(ValueError, match=r"clip 0 of data_s\[0\]"):
        DA.DeviceWaveDataset(clips, None, "cpu", data_s=[[np.arange(3)] * 4])


# ---- 4. loaders, the launch stubbed by the oracle -----------------------------------------------------------------------------------------------
@pytest.fixture
def stub(monkeypatch):
    """ops.wave_view replaced by the float64 oracle on host tensors (rounded to fp32); every call and every host-to-device copy is recorded."""
    calls, copies = [], []

    def wave_view(store, row_off, row_len, src_row, crop_off, S, normalize, host=None):
        flat = store.numpy()
        clips = [flat[o:o + n] for o, n in zip(row_off.tolist(), row_len.tolist())]
        assert src_row.dtype == torch.int64 and crop_off.dtype == torch.int32 and src_row.is_contiguous() and crop_off.is_contiguous()
        calls.append((src_row.numpy().copy(), crop_off.numpy().copy(), int(S), bool(normalize)))
        return torch.from_numpy(WC.oracle(clips, src_row.numpy(), crop_off.numpy(), S, normalize).astype(np.float32))
    monkeypatch.setattr(ops, "wave_view", wave_view)
    real = DA._h2d
    monkeypatch.setattr(DA, "_h2d", lambda t, d: (copies.append(tuple(t.shape)), real(t, d))[1])
    return calls, copies


def _numpy_batches(ld):
    return [{k: v.numpy().copy() for k, v in b.items()} for b in ld]


def test_train_loaders_follow_the_sampler_and_the_step_signature(stub):
    calls, copies = stub
    c, dd = WC.LOADER, WC.loader_dataset_dict()
    ld_l, ld_u = WC.loader_pair(dd, "cpu")
    L, B, BU = c["L"], c["batch_size"], c["batch_size"] * c["uratio"]
    assert len(ld_l) == len(ld_u) == 2 and ld_l.keys == ("idx_lb", "x_lb", "y_lb") and ld_u.keys == ("idx_ulb", "x_ulb_w", "x_ulb_s")
    clips_l, clips_u = WC.store_clips(ld_l.dataset), WC.store_clips(ld_u.dataset)
    n_u, seen_variants = len(ld_u.dataset), set()
    for epoch in (0, 1):
        ld_l.set_epoch(epoch), ld_u.set_epoch(epoch)
        sl, su = EpochSampler(len(ld_l.dataset), 2 * B, 1, 0), EpochSampler(n_u, 2 * BU, 1, 0)
        sl.set_epoch(epoch), su.set_epoch(epoch)
        sl, su = sl.indices(), su.indices()
        calls.clear(), copies.clear()
        steps = list(zip(ld_l, ld_u))
        assert len(steps) == 2 and len(copies) == 2                              # one copy per loader and epoch, none per step
        assert [x[2:] for x in calls] == [(L, True)] * 6                          # x_lb, x_ulb_w, x_ulb_s per step, all padded to L
        for t, (bl, bu) in enumerate(steps):
            il, iu = sl[B * t:B * t + B], su[BU * t:BU * t + BU]
            assert list(bl) == ["idx_lb", "x_lb", "y_lb"] and list(bu) == ["idx_ulb", "x_ulb_w", "x_ulb_s"]
            assert np.array_equal(bl["idx_lb"].numpy(), il) and bl["idx_lb"].dtype == torch.int64
            assert np.array_equal(bl["y_lb"].numpy(), np.asarray(dd["train_lb"]["targets"])[il]) and bl["y_lb"].dtype == torch.int64
            assert np.array_equal(bu["idx_ulb"].numpy(), iu)
            assert bl["x_lb"].shape == (B, L) and bu["x_ulb_w"].shape == bu["x_ulb_s"].shape == (BU, L) and bl["x_lb"].dtype == torch.float32
            (rl, ol), (rw, ow), (rs, os_) = ld_l.draws["x_lb"], ld_u.draws["x_ulb_w"], ld_u.draws["x_ulb_s"]
            assert np.array_equal(rl[B * t:B * t + B], il) and np.array_equal(rw[BU * t:BU * t + BU], iu)
            v = rs[BU * t:BU * t + BU] // n_u - 1                                 # the strong view: a variant's row of the same clip
            assert np.array_equal(rs[BU * t:BU * t + BU] % n_u, iu) and ((v >= 0) & (v < c["V"])).all()
            for x, clips, r, o, n in ((bl["x_lb"], clips_l, rl, ol, B), (bu["x_ulb_w"], clips_u, rw, ow, BU), (bu["x_ulb_s"], clips_u, rs, os_, BU)):
                want = WC.oracle(clips, r[n * t:n * t + n], o[n * t:n * t + n], L, True).astype(np.float32)
                assert np.array_equal(x.numpy(), want)
        for (r, o), clips in ((ld_l.draws["x_lb"], clips_l), (ld_u.draws["x_ulb_w"], clips_u), (ld_u.draws["x_ulb_s"], clips_u)):
            lens = np.array([len(clips[i]) for i in r])
            assert (o[lens <= L] == 0).all() and (o >= 0).all() and (o[lens > L] <= lens[lens > L] - L - 1).all() and o.dtype == np.int32
        seen_variants |= set((ld_u.draws["x_ulb_s"][0] // n_u - 1).tolist())
    assert seen_variants == {0, 1}                                                # both variants are drawn


def test_train_loader_replays_and_two_ranks_split_the_stream(stub):
    calls, copies = stub
    c, dd = WC.LOADER, WC.loader_dataset_dict()

    def same(a, b):
        return len(a) == len(b) and all(list(x) == list(y) and all(np.array_equal(x[k], y[k]) for k in x) for x, y in zip(a, b))
    a, b = WC.loader_pair(dd, "cpu")[1], WC.loader_pair(dd, "cpu")[1]
    e0, e0b = _numpy_batches(a), _numpy_batches(b)
    assert same(e0, e0b) and same(e0, _numpy_batches(a))                          # the same seed: the same batches; iterating again replays them
    a.set_epoch(1)
    e1 = _numpy_batches(a)
    assert not same(e0, e1)
    b.set_epoch(1)
    assert same(e1, _numpy_batches(b))
    a.set_epoch(0)
    assert same(e0, _numpy_batches(a))                                            # set_epoch addresses an epoch directly
    other = _numpy_batches(WC.loader_pair(dd, "cpu", seed=c["seed"] + 1)[1])     # another seed: the sampler's stream stays, the draws change
    assert all(np.array_equal(x["idx_ulb"], y["idx_ulb"]) for x, y in zip(e0, other)) and not same(e0, other)
    # no strong view: not drawn, not launched, the weak view unchanged
    calls.clear()
    weak = _numpy_batches(WC.loader_pair(dd, "cpu", strong=False)[1])
    assert all(list(x) == ["idx_ulb", "x_ulb_w"] for x in weak) and len(calls) == 2
    # two ranks: each takes every second index of the one-rank stream, drop_last on its own share
    ds = DA.DeviceWaveDataset.from_reference(dd["train_ulb"], "cpu")
    whole = EpochSampler(len(ds), 40, 1, 0)
    whole.set_epoch(3)
    for rank in (0, 1):
        ld = DA.WaveTrainLoader(ds, 6, EpochSampler(len(ds), 40, 2, rank), c["L"], True, keys=("idx_ulb", "x_ulb_w", "x_ulb_s"), seed=(0, rank, 1))
        ld.set_epoch(3)
        got = _numpy_batches(ld)
        assert len(ld) == len(got) == 20 // 6 and all(x["x_ulb_w"].shape == (6, c["L"]) for x in got)
        assert np.array_equal(np.concatenate([x["idx_ulb"] for x in got]), whole.indices()[rank::2][:18])
    r0, r1 = (DA.WaveTrainLoader(ds, 6, EpochSampler(len(ds), 40, 2, r), c["L"], True, keys=("idx_ulb", "x_ulb_w"), seed=(0, r, 1)) for r in (0, 1))
    r0._epoch_table(), r1._epoch_table()
    assert not np.array_equal(r0.draws["x_ulb_w"][1], r1.draws["x_ulb_w"][1])    # the rank is part of the seed
    with pytest.raises(ValueError, match="labelled"):
        DA.WaveTrainLoader(ds, 4, EpochSampler(len(ds), 12, 1, 0), c["L"], keys=("idx_lb", "x_lb", "y_lb"))
    with pytest.raises(ValueError, match="strong view must be precomputed"):
        DA.WaveTrainLoader(DA.DeviceWaveDataset(dd["train_ulb"]["data"], None, "cpu"), 4, EpochSampler(len(ds), 12, 1, 0), c["L"],
                           keys=("idx_ulb", "x_ulb_w", "x_ulb_s"))


def test_eval_loader_pads_each_batch_like_the_reference(stub, golden):
    calls, copies = stub
    g, c, dd = golden("device_audio"), WC.LOADER, WC.loader_dataset_dict()
    ds = DA.DeviceWaveDataset.from_reference(dd["eval"], "cpu")
    ld = DA.WaveEvalLoader(ds, c["eval_batch_size"], c["L"], True)
    want_len = g["loader/eval_lengths"].tolist()                                  # what the extractor padded the reference's batches to
    assert want_len == [799, 800, 350] and ld.batch_lengths() == want_len and len(ld) == 3
    for _ in range(2):                                                            # re-iterable
        calls.clear()
        got = list(ld)
        assert [tuple(b["x_lb"].shape) for b in got] == [(3, 799), (3, 800), (2, 350)] and all(list(b) == ["x_lb", "y_lb"] for b in got)
        assert np.array_equal(torch.cat([b["y_lb"] for b in got]).numpy(), np.asarray(dd["eval"]["targets"]))
        assert np.array_equal(np.concatenate([x[0] for x in calls]), np.arange(8)) and not np.concatenate([x[1] for x in calls]).any()
    assert not copies
    with pytest.raises(ValueError, match="labelled"):
        DA.WaveEvalLoader(DA.DeviceWaveDataset.from_reference(dd["train_ulb"], "cpu"), 4, c["L"])


# ---- 5. wiring -------------------------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    c = WC.LOADER
    d = dict(algorithm="hostonly", num_classes=c["num_classes"], num_train_iter=c["num_train_iter"], epoch=c["epoch"], ema_m=0.0, ulb_loss_ratio=1.0,
             use_cat=True, amp=False, lr=5e-4, num_eval_iter=0, num_log_iter=0, gpu=None, rank=0, world_size=1, distributed=False, dataset="urbansound8k",
             num_labels=10, batch_size=c["batch_size"], uratio=c["uratio"], eval_batch_size=c["eval_batch_size"], train_sampler="RandomSampler",
             sample_rate=c["sample_rate"], max_length_seconds=c["max_length_seconds"], seed=c["seed"], data_functions=(None, None))
    d.update(kw)
    return argparse.Namespace(**d)


_W2V = dict(hidden=128, layers=2, heads=2, inter=256, conv_dim=(128, 128, 128), conv_kernel=(10, 3, 2), conv_stride=(5, 2, 2), pos_k=16, pos_groups=4)


class _HostOnly(AlgorithmBase):
    """The base class's wiring with a backbone that is never launched (CPU device) and no optimizer."""
    net = staticmethod(lambda nc: wave2vec.ClassificationWave2Vec(wave2vec.W2vConfig(num_classes=nc, **_W2V), device="cpu"))

    def __init__(self, *a, **k):
        self.lines = []
        super().__init__(*a, **k)

    def set_model(self):
        self.print_fn = self.lines.append
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
    for kw in (dict(), dict(device_audio=False)):
        alg = _HostOnly(_args(dataset=None, **kw), None)
        assert alg.dataset_dict is None and alg.loader_dict is None and alg.device_audio is False
        assert [type(h) for h in alg.hooks_dict.values()] == [ParamUpdateHook, EMAHook, TimerHook]
    ld = {"train_lb": [], "train_ulb": []}
    assert _HostOnly(_args(dataset=None, loader_dict=ld), None).loader_dict is ld
    with pytest.raises(RuntimeError, match="get_data_loader"):                   # a dataset_dict without the option: today's error
        _HostOnly(_args(dataset_dict=WC.loader_dataset_dict()), None)
    with pytest.raises(NotImplementedError, match="waveforms"):                  # device_data with an audio net stays refused
        _HostOnly(_args(device_data=True, net="wave2vecv2_base", dataset_dict=WC.loader_dataset_dict()), None)


def test_option_builds_the_wave_loaders_and_the_seed_hook(stub):
    c = WC.LOADER
    lines = []
    a = _args(device_audio=True, dataset_dict=WC.loader_dataset_dict(), net="wave2vecv2_base", pretrain_path=None)
    os.environ["HF_HUB_CACHE"], old = "/nonexistent-hub-cache", os.environ.get("HF_HUB_CACHE")
    try:
        alg = _HostOnly(a, None, logger=argparse.Namespace(info=lines.append))
    finally:
        os.environ.pop("HF_HUB_CACHE") if old is None else os.environ.__setitem__("HF_HUB_CACHE", old)
    assert a.ulb_dest_len == c["n_ulb"] and a.lb_dest_len == len(c["lb_lens"]) and alg.device_audio
    assert set(alg.loader_dict) == {"train_lb", "train_ulb", "eval"}
    lb, ulb, ev = (alg.loader_dict[k] for k in ("train_lb", "train_ulb", "eval"))
    assert isinstance(lb, DA.WaveTrainLoader) and isinstance(ev, DA.WaveEvalLoader) and isinstance(alg.dataset_dict["train_ulb"], DA.DeviceWaveDataset)
    assert (lb.batch_size, ulb.batch_size, ev.batch_size) == (4, 8, 3) and len(lb) == len(ulb) == 2 and (lb.L, ulb.L, ev.L) == (800,) * 3
    assert (lb.sampler.total, ulb.sampler.total) == (2 * 4, 2 * 8)
    assert lb.keys == ("idx_lb", "x_lb", "y_lb") and ulb.keys == ("idx_ulb", "x_ulb_w", "x_ulb_s")
    assert lb.seed == (c["seed"], 0, 0) and ulb.seed == (c["seed"], 0, 1)
    assert lb.normalize and ulb.normalize and ev.normalize                       # no snapshot: True, and one warning line says so
    assert len([x for x in lines if x.startswith("warning:")]) == 1 and "do_normalize: True" in [x for x in lines if x.startswith("warning:")][0]
    assert [type(h) for h in alg.hooks_dict.values()].count(DistSamplerSeedHook) == 1 and len(alg.hooks_dict) == 4
    alg.epoch = 1
    alg.call_hook("before_train_epoch")
    assert lb.epoch == ulb.epoch == lb.sampler.epoch == ulb.sampler.epoch == 1
    # the same batches as loaders built by hand with the same seed
    by_hand = _numpy_batches(_with_epoch(WC.loader_pair(WC.loader_dataset_dict(), "cpu")[1], 1))
    got = _numpy_batches(ulb)
    assert all(np.array_equal(x[k], y[k]) for x, y in zip(got, by_hand) for k in x) and len(got) == len(by_hand) == 2
    # a train_step without x_ulb_s (srpseudolabel): no strong view, and no data_s needed
    dd = WC.loader_dataset_dict()
    del dd["train_ulb"]["data_s"]
    weak = _HostOnlyWeak(_args(device_audio=True, dataset_dict=dd, audio_do_normalize=False), None)
    assert weak.loader_dict["train_ulb"].keys == ("idx_ulb", "x_ulb_w") and not weak.loader_dict["train_lb"].normalize and not weak.loader_dict["eval"].normalize
    assert not [x for x in weak.lines if str(x).startswith("warning:")]
    # HuBERT is the same engine
    class Hub(_HostOnly):
        net = staticmethod(lambda nc: hubert.ClassificationHubert(wave2vec.W2vConfig(num_classes=nc, **_W2V), device="cpu"))
    assert Hub(_args(device_audio=True, dataset_dict=WC.loader_dataset_dict(), net="hubert_base", audio_do_normalize=True), None).loader_dict is not None


def _with_epoch(ld, epoch):
    ld.set_epoch(epoch)
    return ld


def test_normalize_comes_from_the_snapshots_preprocessor_config(tmp_path):
    snap = tmp_path / "snap"
    snap.mkdir()
    (snap / "config.json").write_text("{}")
    (snap / "model.safetensors").write_bytes(b"")
    lines = []
    a = _args(net="wave2vecv2_base", pretrain_path=str(snap))
    assert DA.resolve_normalize(a, lines.append) is True and len(lines) == 1 and lines[0].startswith("warning:")      # a snapshot without the file
    for pc, want in (({"do_normalize": False}, False), ({"do_normalize": True, "return_attention_mask": False}, True), ({}, True)):
        (snap / "preprocessor_config.json").write_text(json.dumps(pc))
        lines.clear()
        assert DA.resolve_normalize(a, lines.append) is want and not lines
    assert DA.resolve_normalize(_args(net="wave2vecv2_base", pretrain_path=str(snap), audio_do_normalize=False), lines.append) is False
    (snap / "preprocessor_config.json").write_text(json.dumps({"do_normalize": True, "return_attention_mask": True}))
    with pytest.raises(NotImplementedError, match="return_attention_mask: true"):
        DA.resolve_normalize(a, lines.append)
    assert DA.resolve_normalize(_args(net="wave2vecv2_base", pretrain_path=str(snap), audio_do_normalize=True), lines.append) is True    # the yaml key wins


def test_option_refusals_name_their_reason(stub):
    dd = WC.loader_dataset_dict
    ok = dict(device_audio=True, audio_do_normalize=True)
    with pytest.raises(ValueError, match="device_audio and device_data"):
        _HostOnly(_args(dataset_dict=dd(), device_data=True, img_size=8, **ok), None)
    for net in ("vit_small_patch2_32", "bert_base_uncased", "wrn_28_2"):
        with pytest.raises(NotImplementedError, match="does not take waveforms"):
            _HostOnly(_args(dataset_dict=dd(), net=net, **ok), None)

    class Images(_HostOnly):                                                     # ... and from the built model, for a builder handed in without a net name
        net = staticmethod(lambda nc: vit.VisionTransformer(vit.VitConfig(img_size=8, patch_size=2, embed_dim=128, depth=2, num_heads=2, num_classes=nc),
                                                            device="cpu"))
    with pytest.raises(NotImplementedError, match="VisionTransformer.*does not take waveforms"):
        Images(_args(dataset_dict=dd(), **ok), None)
    with pytest.raises(NotImplementedError, match="train_sampler 'WeightedRandomSampler'"):
        _HostOnly(_args(dataset_dict=dd(), train_sampler="WeightedRandomSampler", **ok), None)
    for missing in ("max_length_seconds", "sample_rate"):
        with pytest.raises(ValueError, match="needs args.max_length_seconds and args.sample_rate"):
            _HostOnly(_args(dataset_dict=dd(), **{missing: None}, **ok), None)
    with pytest.raises(ValueError, match=r"= 3 \(random_subsample's window\) differs from .* = 2 "):
        _HostOnly(_args(dataset_dict=dd(), sample_rate=10, max_length_seconds=0.29, **ok), None)       # round(2.9) = 3, int(2.9) = 2
    with pytest.raises(RuntimeError, match="needs the clips"):
        _HostOnly(_args(dataset=None, **ok), None)
    weak = dd()
    del weak["train_ulb"]["data_s"]
    with pytest.raises(ValueError, match="takes x_ulb_s but the unlabelled set has no data_s; the strong view must be precomputed.*WaveformTransforms"):
        _HostOnly(_args(dataset_dict=weak, **ok), None)
    bad = dd()
    bad["train_lb"]["data"][2] = np.arange(5)
    with pytest.raises(ValueError, match="float waveforms"):
        _HostOnly(_args(dataset_dict=bad, **ok), None)


# ---- 6. register budget -------------------------------------------------------------------------------------------------------------------------------
def test_wave_view_kernel_keeps_its_register_budget(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "semireward_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-c",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "o.o"), os.path.join(csrc, "wave_view.hip")],
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
    assert len(out) == 1 and "wave_view_kernel" in next(iter(out)), sorted(out)
    v = next(iter(out.values()))
    assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, v
    assert v["VGPRs"] <= 64 and v["LDS Size [bytes/block]"] == 32, v              # 8 waves per SIMD; four doubles of reduction scratch
