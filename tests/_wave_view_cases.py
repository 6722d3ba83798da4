"""The cases of tests/test_{cpu,gpu}_device_audio.py and of tools/device_audio_golden.py: srhip_wave_view (csrc/wave_view.hip) and the waveform
loaders (semireward_amd/data/device_audio.py), element by element against float64.  Nothing but recorded results is stored: every clip is
rebuilt from its seed, every expected value is recomputed by ``oracle`` below.

oracle.  For output row b with r = src_row[b], c = crop_off[b]: v = clip_r[c : c + S] zero-padded to S, in float64;
normalize = 0: v;  normalize = 1: (v - mean(v)) / sqrt(mean((v - mean(v))^2) + 1e-7) over all S positions (padding included) -- what
transformers' Wav2Vec2FeatureExtractor(do_normalize=True, return_attention_mask=False) computes in float32 on the padded vector.
tests/test_cpu_device_audio.py holds the oracle to the extractor's recorded float32 outputs (tests/golden/device_audio.npz).

Bound of an element, normalize = 1 (normalize = 0 is exact):  |got - want| <= 4 d_ref + 4 ulp_fp32(max |want|), where
d_ref = max |extractor fp32 - oracle f64| of THAT case, measured on the CPU by tools/device_audio_golden.py and stored in the fixture: the
factor 4 allows a summation order other than numpy's pairwise one (both float32), the floor covers the final divide, square root and
rounding.  Never set from what the kernel produced: a case outside the bound is a finding.

Kernel geometries.  For every S four clips -- c0 (2 S + 11 samples), c1 (S + 6), c2 (max(2, S // 2) + 3), c3 (9) -- and six kinds of row:
  k0 (c0, crop 0)              n = S, source 16-byte aligned       k1 (c0, crop 1 + 4 (S % 3))  n = S, source phase 1
  k2 (c1, crop 6)              n = S up to the row's last sample, phase 2
  k3 (c2, crop 3)              n < S (n = S at S = 1), phase 3     k4 (c3, crop 8)              n = 1, phase 0
  k5 (c2, crop 4)              n < S, phase 0: the aligned quads end inside the row
each alone (B = 1) and in two batches of five (a store row repeated with another crop; one (row, crop) pair twice)."""
import numpy as np

KERNEL_S = (1, 3, 4, 5, 255, 256, 257, 1029, 64000)
GEOMETRIES = {"k0": (0,), "k1": (1,), "k2": (2,), "k3": (3,), "k4": (4,), "k5": (5,), "b5a": (0, 1, 2, 3, 4), "b5b": (5, 3, 5, 1, 2)}


def clip(seed, n, dc=0.05, amp=0.1):
    """A float32 clip of n samples: noise of standard deviation ``amp`` around ``dc`` (a mean far from zero relative to the deviation makes a
    dropped or doubled sample of the sums visible)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (dc + amp * rng.standard_normal(n)).astype(np.float32)


def window(c, crop, S):
    """What the extractor is fed for one row: random_subsample's slice (the collator truncates to S itself)."""
    return c[crop:crop + S]


def oracle(clips, src_row, crop_off, S, normalize):
    out = np.zeros((len(src_row), S), dtype=np.float64)
    for b, (r, c) in enumerate(zip(src_row, crop_off)):
        w = window(np.asarray(clips[int(r)]), int(c), S).astype(np.float64)
        out[b, :w.size] = w
    if normalize:
        m = out.sum(1, keepdims=True) / S
        var = ((out - m) ** 2).sum(1, keepdims=True) / S
        out = (out - m) / np.sqrt(var + 1e-7)
    return out


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def bound(d_ref, want):
    return 4.0 * float(d_ref) + 4.0 * ulp32(np.abs(want).max())


def kernel_case(S, geom):
    seed = 1000 * KERNEL_S.index(S)
    clips = [clip(seed + 1, 2 * S + 11), clip(seed + 2, S + 6, dc=-0.2), clip(seed + 3, max(2, S // 2) + 3, dc=0.3, amp=0.02), clip(seed + 4, 9, dc=0.7)]
    kinds = [(0, 0), (0, 1 + 4 * (S % 3)), (1, 6), (2, 3), (3, 8), (2, 4)]
    rows = [kinds[k] for k in GEOMETRIES[geom]]
    return dict(name="S%d/%s" % (S, geom), S=S, clips=clips, src_row=np.array([r for r, _ in rows], dtype=np.int64),
                crop_off=np.array([c for _, c in rows], dtype=np.int32))


def kernel_cases():
    for S in KERNEL_S:
        for geom in GEOMETRIES:
            yield kernel_case(S, geom)


def exact_cases():
    """Cases whose float64 statistics are exact in any summation order: a constant 0.5 with S a power of two -- n = S (mean 0.5, variance 0:
    every element 0) and n = S / 2 (mean 0.25, variance 1 / 16) -- and an all-zero clip.  The kernel must return fp32(oracle) bit for bit."""
    S = 256
    half, zero = np.full(S + 8, 0.5, dtype=np.float32), np.zeros(S + 5, dtype=np.float32)
    yield dict(name="exact/const_full", S=S, clips=[half], src_row=np.array([0], dtype=np.int64), crop_off=np.array([3], dtype=np.int32))
    yield dict(name="exact/const_half", S=S, clips=[half], src_row=np.array([0], dtype=np.int64), crop_off=np.array([S // 2 + 8], dtype=np.int32))
    yield dict(name="exact/zero", S=S, clips=[zero], src_row=np.array([0, 0], dtype=np.int64), crop_off=np.array([0, 2], dtype=np.int32))


# ---- the recorded extractor batches (ragged clips, the offsets the reference's random_subsample drew) ------------------------------------------
FIXTURE_BATCHES = {"S64": dict(S=64, lens=(30, 50, 64, 80, 200), seed=7100, short=(0, 1)),
                   "S800": dict(S=800, lens=(700, 799, 800, 801, 1000, 1300), seed=7200, short=(0, 1))}
N_OFFSET_SEEDS = 400           # random.seed(k), k < N_OFFSET_SEEDS: one offset per clip and seed


def fixture_clips(name):
    f = FIXTURE_BATCHES[name]
    return [clip(f["seed"] + i, n, dc=0.03 * (i - 2)) for i, n in enumerate(f["lens"])]


# ---- the loaders' case: sample_rate 200, max_length_seconds 4.0 -> L = 800; the tiny Wav2Vec2 of the tests (conv_kernel (10, 3, 2)) ------------
LOADER = dict(sample_rate=200, max_length_seconds=4.0, L=800, batch_size=4, uratio=2, eval_batch_size=3, num_train_iter=4, epoch=2, seed=11,
              num_classes=4, lb_lens=(320, 500, 799, 800, 801, 900, 1000, 1200, 1400, 640), n_ulb=24, V=2,
              eval_lens=(320, 500, 799, 900, 400, 800, 350, 330))


def loader_dataset_dict():
    """The plain dataset_dict of the loader / training tests: ragged labelled, unlabelled (+ V variants of other lengths, as a speed effect
    gives) and evaluation clips."""
    c = LOADER
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    lb = [clip(8000 + i, n, dc=0.02 * (i % 5 - 2)) for i, n in enumerate(c["lb_lens"])]
    ulb_lens = rng.integers(320, 1500, size=c["n_ulb"])
    ulb_lens[:3] = (800, 801, 799)
    ulb = [clip(8100 + i, int(n), dc=0.01 * (i % 7 - 3)) for i, n in enumerate(ulb_lens)]
    data_s = [[clip(8200 + 100 * v + i, max(320, int(n * (0.8, 1.3)[v])), dc=0.05 * (v + 1), amp=0.2) for i, n in enumerate(ulb_lens)]
              for v in range(c["V"])]
    ev = [clip(8500 + i, n) for i, n in enumerate(c["eval_lens"])]
    return {"train_lb": {"data": lb, "targets": rng.integers(0, c["num_classes"], size=len(lb))},
            "train_ulb": {"data": ulb, "targets": None, "data_s": data_s},
            "eval": {"data": ev, "targets": rng.integers(0, c["num_classes"], size=len(ev))}}


def loader_pair(dd, device, strong=True, seed=None, normalize=True):
    """(train_lb, train_ulb) WaveTrainLoaders over ``dd`` as build_wave_loaders makes them for one rank, and their datasets."""
    from semireward_amd.data import device_audio as DA
    c = LOADER
    seed = c["seed"] if seed is None else seed
    per_epoch = c["num_train_iter"] // c["epoch"]
    lb, ulb = (DA.DeviceWaveDataset.from_reference(dd[k], device) for k in ("train_lb", "train_ulb"))
    ld_l = DA.WaveTrainLoader(lb, c["batch_size"], DA.EpochSampler(len(lb), per_epoch * c["batch_size"], 1, 0), c["L"], normalize,
                              keys=("idx_lb", "x_lb", "y_lb"), seed=(seed, 0, 0))
    bu = c["batch_size"] * c["uratio"]
    ld_u = DA.WaveTrainLoader(ulb, bu, DA.EpochSampler(len(ulb), per_epoch * bu, 1, 0), c["L"], normalize, strong=strong,
                              keys=("idx_ulb", "x_ulb_w", "x_ulb_s"), seed=(seed, 0, 1))
    return ld_l, ld_u


def store_clips(ds):
    """The clips of a DeviceWaveDataset back as a list of float32 arrays, by store row (host side: row_off_host / row_len_host)."""
    flat = ds.store.cpu().numpy()
    return [flat[o:o + n] for o, n in zip(ds.row_off_host, ds.row_len_host)]


# ---- running a case on the device (tests/test_gpu_device_audio.py, tools/device_audio_time.py) ------------------------------------------------------
NAN_BITS = 0x7FC00ABC                                                  # a quiet NaN with a payload: what columns S .. ldo hold before the launch


def launch(ds, src_row, crop_off, S, normalize, extra=8):
    """The C entry itself on an output whose rows are ``extra`` floats wider than S rounded up to 4, pre-filled with NaN: (the [B, S] block, the
    int32 bits of the columns past S)."""
    import torch
    from semireward_amd import ops
    B, ldo, dev = len(src_row), ((S + 3) & ~3) + extra, ds.device
    out = torch.full((B, ldo), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    r, c = torch.from_numpy(np.asarray(src_row, dtype=np.int64)).to(dev), torch.from_numpy(np.asarray(crop_off, dtype=np.int32)).to(dev)
    ops._call("srhip_wave_view", ds.store.data_ptr(), ds.row_off.data_ptr(), ds.row_len.data_ptr(), int(ds.row_len.shape[0]), r.data_ptr(), c.data_ptr(),
              B, S, int(normalize), out.data_ptr(), ldo, ops._s())
    o = out.cpu()
    return o[:, :S].numpy().copy(), o[:, S:].contiguous().view(torch.int32).numpy()


def verify(case, d_ref, device):
    """One kernel case, both modes, every property: normalize = 0 bit-exact; normalize = 1 every element within ``bound``; the columns past S
    untouched; two launches and the ops.wave_view wrapper give the same bits.  Returns (largest error, bound) of normalize = 1."""
    import torch
    from semireward_amd import ops
    from semireward_amd.data.device_audio import DeviceWaveDataset
    ds = DeviceWaveDataset(case["clips"], None, device)
    S, r, c = case["S"], case["src_row"], case["crop_off"]
    args = (ds.store, ds.row_off, ds.row_len, torch.from_numpy(r).to(device), torch.from_numpy(c).to(device), S)
    host = (r, c, ds.row_len_host)
    got, past = launch(ds, r, c, S, 0)
    want = oracle(case["clips"], r, c, S, False)
    assert (past == NAN_BITS).all(), case["name"]
    assert got.tobytes() == want.astype(np.float32).tobytes(), case["name"]
    assert ops.wave_view(*args, False, host=host).cpu().numpy().tobytes() == got.tobytes(), case["name"]
    got, past = launch(ds, r, c, S, 1)
    want = oracle(case["clips"], r, c, S, True)
    assert (past == NAN_BITS).all(), case["name"]
    err, tol = float(np.abs(got - want).max()), bound(d_ref, want)
    assert np.isfinite(got).all() and err <= tol, (case["name"], err, tol, d_ref)
    again, _ = launch(ds, r, c, S, 1)
    assert again.tobytes() == got.tobytes() and ops.wave_view(*args, True, host=host).cpu().numpy().tobytes() == got.tobytes(), case["name"]
    return err, tol
