"""device_audio_strong (semireward_amd/data/device_audio.py, csrc/wave_strong.hip) without a GPU: the C ABI entry and every refusal of it and of
its wrapper; the option's wiring and refusals; the loader's draws (ranges, replay, the integer length rule, the weak view untouched, one copy per
epoch) with both launches stubbed by the float64 restatement; and the restatement of tests/_wave_strong_cases.py held to the conditions its
specification states (it is what the kernel is tested against: tests/test_gpu_wave_strong.py)."""
import argparse
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import _wave_strong_cases as WS
import _wave_view_cases as WC
from semireward_amd import _lib, ops
from semireward_amd.core.algorithmbase import AlgorithmBase
from semireward_amd.data import device_audio as DA
from semireward_amd.data.device_loader import EpochSampler
from semireward_amd.nets import wave2vec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_KEYS = ["x_lb", "y_lb", "idx_ulb", "x_ulb_w", "x_ulb_s"]               # the train_step signature of srflexmatch / srsoftmatch / srfreematch


def _args(**kw):
    c = WC.LOADER
    d = dict(algorithm="hostonly", num_classes=c["num_classes"], num_train_iter=c["num_train_iter"], epoch=c["epoch"], ema_m=0.0, ulb_loss_ratio=1.0,
             use_cat=True, amp=False, lr=5e-4, num_eval_iter=0, num_log_iter=0, gpu=None, rank=0, world_size=1, distributed=False, dataset="urbansound8k",
             num_labels=10, batch_size=c["batch_size"], uratio=c["uratio"], eval_batch_size=c["eval_batch_size"], train_sampler="RandomSampler",
             sample_rate=c["sample_rate"], max_length_seconds=c["max_length_seconds"], seed=c["seed"], data_functions=(None, None),
             device_audio=True, audio_do_normalize=True)
    d.update(kw)
    return argparse.Namespace(**d)


def _clean_dict():
    dd = WC.loader_dataset_dict()
    del dd["train_ulb"]["data_s"]
    return dd


# ---- 1. what fails without the feature ----------------------------------------------------------------------------------------------------------
def test_key_builds_strong_loaders_without_data_s():
    a = _args(device_audio_strong=True)
    dsets = DA.build_wave_datasets(a, _clean_dict(), "cpu")
    ld = DA.build_wave_loaders(a, dsets, STEP_KEYS, a.num_train_iter, a.epoch, 1, 0)
    ulb = ld["train_ulb"]
    assert ulb.keys == ("idx_ulb", "x_ulb_w", "x_ulb_s") and ulb.makes_strong and dsets["train_ulb"].n_variants == 0
    assert ulb.pitch == 4 * int(dsets["train_ulb"].row_len_host.max()) and ulb.pitch % 4 == 0
    assert [tuple(s.shape) for s in ulb._scratch] == [(ulb.batch_size, ulb.pitch)] * 2 and ulb.delays.tolist() == WS.delays(a.sample_rate)
    assert ld["train_lb"].keys == ("idx_lb", "x_lb", "y_lb") and not hasattr(ld["train_lb"], "pitch")       # nothing allocated where no strong view is made
    # an algorithm that does not take x_ulb_s makes no strong view, as without the key
    weak = DA.build_wave_loaders(a, dsets, ["x_lb", "y_lb", "x_ulb_w"], a.num_train_iter, a.epoch, 1, 0)["train_ulb"]
    assert weak.keys == ("idx_ulb", "x_ulb_w") and not hasattr(weak, "pitch")


def test_library_exports_the_entry_and_the_binding_matches_the_header():
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "srhip_wave_effect")
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srhip.h")).read(), flags=re.S)
    decl = re.search(r"int\s+srhip_wave_effect\s*\(([^)]*)\)", src).group(1).split(",")
    res, argtypes = _lib.SIGNATURES["srhip_wave_effect"]
    assert res is _lib.I and len(decl) == 16 and [_lib.P if "*" in a else _lib.I for a in decl] == argtypes
    assert (ops.WAVE_COPY, ops.WAVE_GAIN, ops.WAVE_RESAMPLE, ops.WAVE_REVERB) == (WS.COPY, WS.GAIN, WS.RESAMPLE, WS.REVERB) == (0, 1, 2, 3)
    assert re.search(r"SR_WAVE_COPY = 0, SR_WAVE_GAIN = 1, SR_WAVE_RESAMPLE = 2, SR_WAVE_REVERB = 3", src)


# ---- 2. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_entry_refuses_each_bad_argument():
    f = _lib.lib().srhip_wave_effect
    buf = (ctypes.c_float * 64)()
    a = (ctypes.addressof(buf) + 15) & ~15                                       # an aligned host address: never dereferenced as device memory, every call is refused first
    h_op, h_par, h_len = np.array([1, 2], dtype=np.int32), np.array([0, 1 << 32], dtype=np.int64), np.array([6, 8], dtype=np.int32)
    dl = np.array(WS.DELAYS_16K, dtype=np.int32)
    ok = dict(store=a, row_off=a, row_len=a, n_rows=2, src_row=a, op=a, param=a, dst_len=a, B=2, dst=a, pitch=8, h_op=h_op.ctypes.data,
              h_par=h_par.ctypes.data, h_len=h_len.ctypes.data, dl=dl.ctypes.data, stream=None)

    def rc(**kw):
        return f(*{**ok, **kw}.values())
    for k in ("store", "row_off", "row_len", "src_row", "op", "param", "dst_len", "dst", "h_op", "h_par", "h_len", "dl"):
        assert rc(**{k: None}) == -1, k                                          # SR_EINVAL
    for kw in (dict(B=0), dict(B=-1), dict(B=65536), dict(n_rows=0), dict(pitch=0), dict(pitch=6), dict(pitch=10), dict(pitch=4), dict(dst=a + 4),
               dict(dst=a + 8)):                                                  # pitch 4 is below dst_len 6 and 8
        assert rc(**kw) == -1, kw

    def host(op=(1, 2), par=(0, 1 << 32), ln=(6, 8), delays=WS.DELAYS_16K):
        arrs = np.array(op, dtype=np.int32), np.array(par, dtype=np.int64), np.array(ln, dtype=np.int32), np.array(delays, dtype=np.int32)
        return rc(h_op=arrs[0].ctypes.data, h_par=arrs[1].ctypes.data, h_len=arrs[2].ctypes.data, dl=arrs[3].ctypes.data)
    for kw in (dict(op=(1, 4)), dict(op=(-1, 2)), dict(ln=(6, 9)), dict(ln=(0, 8)), dict(ln=(6, -2)), dict(par=(0, (1 << 31) - 1)), dict(par=(0, (1 << 33) + 1)),
               dict(par=(0, 0)), dict(par=(0, -(1 << 32))), dict(delays=(0,) + WS.DELAYS_16K[1:]), dict(delays=WS.DELAYS_16K[:11] + (-3,)),
               dict(delays=(20000,) + WS.DELAYS_16K[1:]), dict(delays=tuple(WS.delays(44100)))):        # 44.1 kHz: 76 KB of delay lines
        assert host(**kw) == -1, kw


def _wrapper_args(pitch=16):
    store, off, ln = torch.zeros(24), torch.tensor([0, 8]), torch.tensor([5, 8], dtype=torch.int32)
    rows, op, par = np.array([1, 0, 1]), np.array([1, 2, 3], dtype=np.int32), np.array([0x3F800000, 1 << 31, 0], dtype=np.int64)
    m = np.array([8, 10, 8], dtype=np.int32)
    dev = [torch.from_numpy(x) for x in (rows, op, par, m)]
    return [store, off, ln] + dev + [torch.zeros(3, pitch), np.array(WS.DELAYS_16K, dtype=np.int32)], [rows, op, par, m, np.array([5, 8], dtype=np.int32)]


def test_wrapper_checks_on_the_host_what_the_kernel_cannot(monkeypatch):
    sent = []
    monkeypatch.setattr(ops, "_call", lambda name, *a: sent.append((name, a)))
    monkeypatch.setattr(ops, "_p", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(ops, "_s", lambda: None)
    a, h = _wrapper_args()
    assert ops.wave_effect(*a, host=h) is a[7]
    (name, sent_args), = sent
    assert name == "srhip_wave_effect" and len(sent_args) == 16 and sent_args[3] == 2 and sent_args[8] == 3 and sent_args[10] == 16     # n_rows, B, pitch

    def bad(exc, match, i=None, v=None, hi=None, hv=None):
        a, h = _wrapper_args()
        if i is not None:
            a[i] = v
        if hi is not None:
            h[hi] = hv
        with pytest.raises(exc, match=match):
            ops.wave_effect(*a, host=h)
    bad(IndexError, "src_row outside", hi=0, hv=np.array([1, 2, 1]))
    bad(IndexError, "src_row outside", hi=0, hv=np.array([1, -1, 1]))
    bad(ValueError, "op outside", hi=1, hv=np.array([1, 2, 4], dtype=np.int32))
    bad(ValueError, "resample step outside", hi=2, hv=np.array([0, (1 << 31) - 1, 0]))
    bad(ValueError, r"dst_len\[1\] = 9, but op 2 maps 5 samples to 10", hi=3, hv=np.array([8, 9, 8], dtype=np.int32))       # the resample's integer rule
    bad(ValueError, r"dst_len\[0\] = 7, but op 1 maps 8 samples to 8", hi=3, hv=np.array([7, 10, 8], dtype=np.int32))       # gain keeps the length
    bad(ValueError, "source row of 0 samples", hi=4, hv=np.array([0, 8], dtype=np.int32))
    bad(ValueError, "does not fit the destination's pitch 8", i=7, v=torch.zeros(3, 8))
    bad(ValueError, "pitch % 4", i=7, v=torch.zeros(3, 18))
    bad(ValueError, r"\[>= B, pitch\]", i=7, v=torch.zeros(2, 16))
    bad(ValueError, "contiguous", i=7, v=torch.zeros(3, 32)[:, :16])
    bad(ValueError, "12 reverb delays", i=8, v=np.arange(1, 12))
    bad(ValueError, "int64", i=3, v=torch.tensor([1, 0, 1], dtype=torch.int32))
    bad(ValueError, "fp32", i=0, v=torch.zeros(24, dtype=torch.float64))
    a, h = _wrapper_args()
    a[7] = a[0].view(-1)[:16].view(1, 16)                                        # a view of the store itself
    a[3:7], h[:4] = [x[:1] for x in a[3:7]], [x[:1] for x in h[:4]]
    with pytest.raises(ValueError, match="same buffer"):
        ops.wave_effect(*a, host=h)
    assert len(sent) == 1                                                         # nothing else reached the library


class _HostOnly(AlgorithmBase):
    """The base class's wiring with a backbone that is never launched (CPU device) and no optimizer."""
    _W2V = dict(hidden=128, layers=2, heads=2, inter=256, conv_dim=(128, 128, 128), conv_kernel=(10, 3, 2), conv_stride=(5, 2, 2), pos_k=16, pos_groups=4)

    def set_model(self):
        self.print_fn = lambda *a: None
        return wave2vec.ClassificationWave2Vec(wave2vec.W2vConfig(num_classes=self.num_classes, **self._W2V), device="cpu")

    def set_ema_model(self):
        return self.model

    def set_optimizer(self):
        return None, None

    def train_step(self, x_lb, y_lb, idx_ulb, x_ulb_w, x_ulb_s):
        raise AssertionError("not stepped")


def test_option_wiring_and_refusals():
    alg = _HostOnly(_args(device_audio_strong=True, dataset_dict=_clean_dict()), None)
    assert alg.loader_dict["train_ulb"].makes_strong and alg.loader_dict["train_ulb"].keys[-1] == "x_ulb_s"
    for kw in (dict(device_audio=False), dict(device_audio=False, device_data=True, img_size=8)):
        with pytest.raises(ValueError, match="device_audio_strong: True .* needs device_audio: True"):
            _HostOnly(_args(device_audio_strong=True, dataset_dict=_clean_dict(), **kw), None)
    with pytest.raises(ValueError, match="device_audio_strong.*needs device_audio"):
        DA.device_strong(argparse.Namespace(device_audio_strong=True))
    with pytest.raises(ValueError, match="device_audio_strong: the unlabelled set carries data_s .* one source of strong views"):
        _HostOnly(_args(device_audio_strong=True, dataset_dict=WC.loader_dataset_dict()), None)
    with pytest.raises(ValueError, match="has no data_s; the strong view must be precomputed"):      # without the key: today's refusal, word for word
        _HostOnly(_args(dataset_dict=_clean_dict()), None)
    ds = DA.DeviceWaveDataset(_clean_dict()["train_ulb"]["data"], None, "cpu")
    with pytest.raises(ValueError, match="one source of strong views"):          # the loader itself, handed both
        DA.WaveTrainLoader(DA.DeviceWaveDataset.from_reference(WC.loader_dataset_dict()["train_ulb"], "cpu"), 4, EpochSampler(24, 8, 1, 0), 800,
                           keys=("idx_ulb", "x_ulb_w", "x_ulb_s"), device_strong=True, sample_rate=200)
    with pytest.raises(ValueError, match="sample_rate"):
        DA.WaveTrainLoader(ds, 4, EpochSampler(24, 8, 1, 0), 800, keys=("idx_ulb", "x_ulb_w", "x_ulb_s"), device_strong=True)
    # the over-long clip: 4 x 2^28 + 4 samples would pass srhip_wave_view's 2^30 (a stand-in store: only the lengths are looked at)
    lens = np.array([1000, (1 << 28) + 1, 500], dtype=np.int32)
    big = types.SimpleNamespace(n=3, n_variants=0, targets=None, device=torch.device("cpu"), row_len_host=lens)
    with pytest.raises(ValueError, match=r"device_audio_strong: clip 1 holds 268435457 samples.*2\^30"):
        DA.WaveTrainLoader(big, 4, EpochSampler(3, 8, 1, 0), 800, keys=("idx_ulb", "x_ulb_w", "x_ulb_s"), device_strong=True, sample_rate=16000)
    lens[1] = 1 << 28                                                             # exactly 2^30 after both slots: accepted (the buffers are not made here)
    assert (DA.MAX_GROWTH * int(lens[1]) + 3) & ~3 == DA.MAX_VIEW_SOURCE


# ---- 3. the draws -----------------------------------------------------------------------------------------------------------------------------------
def test_draw_ranges_and_the_length_rule():
    rng = np.random.Generator(np.random.PCG64(3))
    n0 = rng.integers(1, 5000, size=20000)
    d = DA.draw_effects(rng, n0)
    assert d["speed"].min() >= 0.5 and d["speed"].max() < 2.0 and d["speed"].min() < 0.51 and d["speed"].max() > 1.99
    assert d["cents"].min() >= -2.0 and d["cents"].max() < 2.0 and d["cents"].min() < -1.99 and d["cents"].max() > 1.99
    assert set(d["att"].tolist()) == set(range(-4, 5)) and set(d["effect"].ravel().tolist()) == {0, 1, 2, 3}
    assert np.bincount(d["att"] + 4)[4] > 1.7 * np.bincount(d["att"] + 4)[0]      # truncation toward zero: 0 collects (-1, 1), twice the others
    pairs = np.bincount(4 * d["effect"][:, 0] + d["effect"][:, 1], minlength=16)
    assert pairs.min() > 0.8 * 20000 / 16 and pairs.max() < 1.2 * 20000 / 16       # with replacement: all 16 ordered pairs, the doubles too
    assert d["op"].dtype == np.int32 and d["param"].dtype == np.int64 and d["lens"].dtype == np.int64 and set(d["op"].ravel().tolist()) == {1, 2, 3}
    for i in range(0, 20000, 37):                                                 # the same (op, param) and lengths as the restatement's scalar rule
        n = int(n0[i])
        for slot in (0, 1):
            op, param = WS.effect_of(float(d["speed"][i]), float(d["cents"][i]), int(d["att"][i]), int(d["effect"][i, slot]))
            assert (op, param) == (int(d["op"][i, slot]), int(d["param"][i, slot])), (i, slot)
            n = WS.out_len(n, op, param)
            assert n == int(d["lens"][i, slot + 1]) and 1 <= n <= 2 * int(d["lens"][i, slot]) + 1
    rs = d["op"] == WS.RESAMPLE
    assert d["param"][rs].min() >= 1 << 31 and d["param"][rs].max() < 1 << 33
    assert (d["lens"][:, 2] <= 4 * d["lens"][:, 0]).all()                         # what the scratch pitch relies on
    assert ops.wave_effect_len([1, 2, 3, 1, 3], [2] * 5, [1 << 33, 1 << 33, 1 << 33, 1 << 31, WS.step_of(1.3)]).tolist() == [1, 1, 1, 2, 2]


@pytest.fixture
def stub(monkeypatch):
    """ops.wave_view replaced by the float64 oracle and ops.wave_effect by the float64 restatement, both on host tensors and rounded to fp32;
    every launch and every host-to-device copy is recorded."""
    calls, copies = [], []

    def rows_of(store, row_off, row_len):
        flat = store.numpy().reshape(-1)
        return [flat[o:o + n] for o, n in zip(row_off.tolist(), row_len.tolist())]

    def wave_view(store, row_off, row_len, src_row, crop_off, S, normalize, host=None):
        calls.append("view")
        return torch.from_numpy(WC.oracle(rows_of(store, row_off, row_len), src_row.numpy(), crop_off.numpy(), S, normalize).astype(np.float32))

    def wave_effect(store, row_off, row_len, src_row, op, param, dst_len, dst, delays, host):
        calls.append("effect")
        ops.check_wave_effect(*host, int(dst.shape[1]))
        assert all(np.array_equal(d.numpy(), h) for d, h in zip((src_row, op, param, dst_len), host))      # the device slices are the host slices
        assert np.array_equal(row_len.numpy()[src_row.numpy()], np.asarray(host[4])[host[0]])
        clips = rows_of(store, row_off, row_len)
        for b, r in enumerate(src_row.tolist()):
            y = WS.apply(int(op[b]), int(param[b]), clips[r], list(delays), 200)[0]
            assert y.size == int(dst_len[b])
            dst[b, :y.size] = torch.from_numpy(y.astype(np.float32))
        return dst
    monkeypatch.setattr(ops, "wave_view", wave_view)
    monkeypatch.setattr(ops, "wave_effect", wave_effect)
    real = DA._h2d
    monkeypatch.setattr(DA, "_h2d", lambda t, d: (copies.append(tuple(t.shape)), real(t, d))[1])
    return calls, copies


def _made_loader(seed=None, normalize=True):
    c = WC.LOADER
    ds = DA.DeviceWaveDataset(_clean_dict()["train_ulb"]["data"], None, "cpu")
    bu = c["batch_size"] * c["uratio"]
    per_epoch = c["num_train_iter"] // c["epoch"]
    return DA.WaveTrainLoader(ds, bu, EpochSampler(len(ds), per_epoch * bu, 1, 0), c["L"], normalize, keys=("idx_ulb", "x_ulb_w", "x_ulb_s"),
                              seed=(c["seed"] if seed is None else seed, 0, 1), device_strong=True, sample_rate=c["sample_rate"])


def test_loader_tables_replay_and_leave_the_weak_view_alone(stub):
    calls, copies = stub
    c, L = WC.LOADER, WC.LOADER["L"]
    ld, twin = _made_loader(), _made_loader()
    with_s, weak_only = WC.loader_pair(WC.loader_dataset_dict(), "cpu")[1], WC.loader_pair(WC.loader_dataset_dict(), "cpu", strong=False)[1]
    tables = {}
    for epoch in (0, 1):
        for x in (ld, twin, with_s, weak_only):
            x.set_epoch(epoch)
        t, where, N = ld._epoch_table()
        t2, _, _ = twin._epoch_table()
        assert np.array_equal(t, t2) and t.shape == (2 + 1 + 6, N) and where == {"idx_ulb": 0, "x_ulb_w": 1, "x_ulb_s": 3}       # equal (seed, epoch): equal tables
        tables[epoch], sd = t, ld.strong_draws
        (rows_s, crop_s), lens = ld.draws["x_ulb_s"], ld.strong_draws["lens"]
        assert np.array_equal(rows_s, t[0]) and np.array_equal(lens[:, 0], ld.dataset.row_len_host[rows_s])                       # the clean stream, no variant rows
        assert crop_s.dtype == np.int32 and (crop_s >= 0).all() and (crop_s[lens[:, 2] <= L] == 0).all()
        assert (crop_s[lens[:, 2] > L] <= lens[lens[:, 2] > L, 2] - L - 1).all() and (lens[:, 2] > L).any() and (lens[:, 2] <= L).any()
        i32 = t.view(np.int32).reshape(t.shape[0], 2, N)                                                                          # [row, half, position]
        assert np.array_equal(i32[4, 0], crop_s) and np.array_equal(i32[4, 1], sd["op"][:, 0]) and np.array_equal(i32[5, 0], sd["op"][:, 1])
        assert np.array_equal(i32[5, 1], lens[:, 1]) and np.array_equal(i32[6, 0], lens[:, 2]) and not i32[6, 1].any()
        assert np.array_equal(t[7], sd["param"][:, 0]) and np.array_equal(t[8], sd["param"][:, 1])
        for other in (with_s, weak_only):                                                                                         # x_ulb_w: the rows and offsets of a loader without the key
            other._epoch_table()
            assert all(np.array_equal(a, b) for a, b in zip(ld.draws["x_ulb_w"], other.draws["x_ulb_w"]))
    assert not np.array_equal(tables[0][3:], tables[1][3:])                                                                       # another epoch: other tables
    other_seed = _made_loader(seed=c["seed"] + 1)
    other_seed.set_epoch(1)
    assert not np.array_equal(other_seed._epoch_table()[0][4:], tables[1][4:])


def test_loader_batches_are_the_restated_chain_of_the_recorded_draws(stub):
    calls, copies = stub
    c, L = WC.LOADER, WC.LOADER["L"]
    ld, weak_only = _made_loader(), WC.loader_pair(WC.loader_dataset_dict(), "cpu", strong=False)[1]
    clips, dl, BU = WC.store_clips(ld.dataset), WS.delays(c["sample_rate"]), ld.batch_size
    for epoch in (0, 1):
        ld.set_epoch(epoch), weak_only.set_epoch(epoch)
        calls.clear(), copies.clear()
        got = [{k: v.numpy().copy() for k, v in b.items()} for b in ld]
        assert len(got) == 2 and len(copies) == 1 and calls == ["view", "effect", "effect", "view"] * 2          # one copy an epoch; a strong view is three launches
        sd, (rows, crop) = ld.strong_draws, ld.draws["x_ulb_s"]
        for t, (b, w) in enumerate(zip(got, weak_only)):
            assert list(b) == ["idx_ulb", "x_ulb_w", "x_ulb_s"] and b["x_ulb_s"].shape == (BU, L) and b["x_ulb_s"].dtype == np.float32
            assert np.array_equal(b["x_ulb_w"], w["x_ulb_w"].numpy()) and np.array_equal(b["idx_ulb"], w["idx_ulb"].numpy())
            aug = []
            for i in range(BU * t, BU * t + BU):
                y = clips[rows[i]]
                for slot in (0, 1):
                    y = WS.apply(int(sd["op"][i, slot]), int(sd["param"][i, slot]), y, dl, c["sample_rate"])[0].astype(np.float32)
                assert y.size == sd["lens"][i, 2]
                aug.append(y)
            want = WC.oracle(aug, np.arange(BU), crop[BU * t:BU * t + BU], L, True).astype(np.float32)
            assert np.array_equal(b["x_ulb_s"], want) and not np.array_equal(b["x_ulb_s"], b["x_ulb_w"])
        again = [{k: v.numpy().copy() for k, v in b.items()} for b in ld]                                         # iterating again replays the epoch
        assert all(np.array_equal(x[k], y[k]) for x, y in zip(got, again) for k in x)


# ---- 4. the restatement alone: the conditions its specification states -----------------------------------------------------------------------------
def test_resample_restatement():
    x = WS.clip(5, 300).astype(np.float64)
    out, l1, l1x, l1h, taps = WS.resample(x, WS.ONE)
    assert np.array_equal(out, x) and (taps == 1).all()                                                           # identity at step = 2^32
    for n in (1, 2, 3):
        for s in WS.RESAMPLE_S:
            step = WS.step_of(s)
            m = WS.resample(WS.clip(1, max(n, 2))[:n].astype(np.float64), step)[0].size
            assert m == max(1, (n << 32) // step) == WS.out_len(n, WS.RESAMPLE, step) and m >= 1
    assert [WS.out_len(n, WS.RESAMPLE, WS.step_of(2.0)) for n in (1, 2, 3)] == [1, 1, 1] and WS.out_len(3, WS.RESAMPLE, WS.step_of(0.5)) == 6
    assert WS.step_of(0.5) == 1 << 31 and WS.step_of(1.0) == WS.ONE and WS.resample(x, WS.step_of(2.0))[4].max() == 65       # at most 65 taps at s = 2
    n, sr, worst = 4000, 16000.0, 0.0
    t = np.arange(n)
    for f0 in (200.0, 1000.0):
        tone = np.sin(2 * np.pi * f0 * t / sr + 0.3)
        for s in (0.5, 0.75, 1.3, 2.0):
            step = WS.step_of(s)
            out = WS.resample(tone, step)[0]
            pos = np.arange(out.size) * (step / 2.0 ** 32)                                                        # where output j sits in the input
            edge = 40.0 * max(1.0, s)                                                                             # 40 / c samples at either end
            keep = (pos >= edge) & (pos <= n - 1 - edge)
            err = np.abs(out - np.sin(2 * np.pi * f0 * pos / sr + 0.3))[keep].max()
            worst = max(worst, err)
            assert keep.sum() > 1000 and err <= 2e-4, (f0, s, err)
    print("\nresample restatement: worst distance from the analytic tone %.3g (bound 2e-4)" % worst)


def test_gain_restatement():
    x = WS.gain_clip(3, 500, "middle").astype(np.float64)
    for att in WS.GAIN_ATT:
        out, pre = WS.gain_want(x, att)
        assert out.size == x.size and np.abs(out).max() <= 1.0
        if att <= 0:
            assert np.isclose(np.abs(out).max(), 10.0 ** (att / 20.0), rtol=1e-15) and np.array_equal(out, pre)     # the peak is 10^(att / 20)
        else:
            assert np.abs(pre).max() > 1.0 and np.abs(out).max() == 1.0 and np.array_equal(np.abs(out) == 1.0, np.abs(pre) >= 1.0)
    zero = np.zeros(17)
    assert np.array_equal(WS.gain_want(zero, 3)[0], zero)


def test_reverb_restatement():
    assert WS.delays(16000) == list(WS.DELAYS_16K) and WS.delays(8000) == list(WS.DELAYS_8K)
    assert ops.reverb_delays(16000).tolist() == list(WS.DELAYS_16K) and ops.reverb_delays(8000).tolist() == list(WS.DELAYS_8K)
    assert WS.DELAYS_8K[0] == 202 and WS.DELAYS_8K[7] == 293 and WS.DELAYS_8K[8:] == (101, 80, 62, 41)
    for dl in (WS.DELAYS_16K, WS.DELAYS_8K):
        imp = np.zeros(3000)
        imp[0] = 1.0
        h = WS.reverb(imp, dl)
        assert np.flatnonzero(h)[0] == min(dl[:8]) and np.isclose(h[min(dl[:8])], 3.0 * 0.015)                  # through four allpasses, each -1 at lag 0
    rng = np.random.Generator(np.random.PCG64(9))
    x = rng.standard_normal(5000)
    a, b = WS.reverb(x, WS.DELAYS_16K), WS.reverb(x, WS.DELAYS_16K, fir=True)
    d = np.abs(a - b).max()
    print("\nreverb: 24-term comb form against the recursion, max |difference| %.3g (bound 1e-12), max |out| %.3g" % (d, np.abs(a).max()))
    assert d <= 1e-12 and np.abs(a).max() > 0.1
    assert not WS.reverb(x[:400], WS.DELAYS_16K).any()                                                           # shorter than the shortest comb delay: silence
    g = WS.reverb_gains(tuple(WS.DELAYS_16K), WS.ir_length(16000))
    assert 30.0 < g["G"] < 60.0 and g["A"][4] == 1.0 and all(abs(s - 3.0) < 1e-9 for s in g["S"])               # an allpass: |-1| + 1 + 0.5 + 0.25 + ... = 3
