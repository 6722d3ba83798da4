"""device_audio_strong on the MI355X: every srhip_wave_effect launch (csrc/wave_strong.hip) against the float64 restatement of
tests/_wave_strong_cases.py, element by element, with the bounds derived there from the arithmetic (gain: 1.5 ulp before the clamp; resample:
32 u sum |x_k| + (taps + 2) u sum |x_k h_k|; reverb: the per-sample roundings carried through the network's l1 gains, computed from the
restatement's impulse responses); the loader's strong view against wave_view of the restated chain of its recorded draws within the composed
bound; two SRFlexMatch steps of the tiny Wav2Vec2 fed by it.  Measured headroom per op: profiles/wave_strong_headroom.txt."""
import argparse
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _wave_strong_cases as WS                                        # noqa: E402
import _wave_view_cases as WC                                          # noqa: E402
from semireward_amd.algorithms import get_algorithm                    # noqa: E402
from semireward_amd.data import device_audio as DA                     # noqa: E402
from semireward_amd.nets import wave2vec                               # noqa: E402

DEV = "cuda:0"


_gain_bits, _check_resample, _check_gain, _check_reverb = WS.gain_bits, WS.check_resample, WS.check_gain, WS.check_reverb


@pytest.mark.parametrize("s", WS.RESAMPLE_S, ids=lambda s: "s%.4f" % s)
def test_resample_against_float64(s):
    step = WS.step_of(s)
    clips = [WS.clip(100 + n, max(n, 2))[:n] for n in WS.RESAMPLE_N]                 # (a clip of one sample keeps the first spike)
    outs, clean, _ = WS.launch(clips, [(WS.RESAMPLE, step)] * len(clips), WS.DELAYS_16K, DEV)
    assert clean and [o.size for o in outs] == [WS.out_len(n, WS.RESAMPLE, step) for n in WS.RESAMPLE_N]
    if step == WS.ONE:
        assert all(o.tobytes() == c.tobytes() for o, c in zip(outs, clips))        # step = 2^32 copies bit for bit
    used = max(_check_resample(c, step, o, (s, c.size)) for c, o in zip(clips, outs))
    print("\nresample s = %.6f: largest share of the bound used %.3f" % (s, used))


@pytest.mark.parametrize("s", (1.3, 2.0 ** (-2.0 / 1200.0)), ids=("speed1.3", "pitch-2c"))
def test_resample_positions_beyond_fp32_fraction_bits(s):
    """2^18 + 5 samples: an fp32 position j * s would keep six fraction bits or fewer behind j = 2^18; the kernel's positions are 64-bit integers."""
    step, x = WS.step_of(s), WS.clip(77, WS.LONG_N)
    (got,), clean, _ = WS.launch([x], [(WS.RESAMPLE, step)], WS.DELAYS_16K, DEV)
    assert clean and got.size == WS.out_len(WS.LONG_N, WS.RESAMPLE, step)
    used = _check_resample(x, step, got, s)
    print("\nresample n = %d, s = %.6f: largest share of the bound used %.3f" % (WS.LONG_N, s, used))


def test_gain_against_float64():
    cases = [(WS.gain_clip(10 * (att + 4) + i, 501 + att, where), att) for att in WS.GAIN_ATT for i, where in enumerate(("first", "last", "middle"))]
    cases += [(np.zeros(33, dtype=np.float32), 3), (np.array([-0.4], dtype=np.float32), -3), (WS.gain_clip(7, 4101, "last"), 2),
              (WS.gain_clip(8, 8195, "first"), -4)]                                   # a zero clip, one sample, more than one pass of the workgroup
    outs, clean, _ = WS.launch([c for c, _ in cases], [(WS.GAIN, _gain_bits(a)) for _, a in cases], WS.DELAYS_16K, DEV)
    assert clean and outs[27].tobytes() == cases[27][0].tobytes()                    # the zero clip comes back unchanged
    used = max(_check_gain(c, a, o, (i, a)) for i, ((c, a), o) in enumerate(zip(cases, outs)) if i != 27)
    print("\ngain: largest share of the 1.5 ulp bound used %.3f" % used)


@pytest.mark.parametrize("rate,lens,dl", [(16000, WS.REVERB_N_16K, WS.DELAYS_16K), (8000, WS.REVERB_N_8K, WS.DELAYS_8K)], ids=("16k", "8k"))
def test_reverb_against_the_sequential_recursion(rate, lens, dl):
    clips = [WS.clip(300 + n, max(n, 2))[:n] for n in lens]
    outs, clean, _ = WS.launch(clips, [(WS.REVERB, 0)] * len(clips), dl, DEV)
    assert clean and [o.size for o in outs] == list(lens)
    used = max(_check_reverb(c, list(dl), rate, o, c.size) for c, o in zip(clips, outs))
    for c, o in zip(clips, outs):
        assert o.any() == (c.size > min(dl[:8]))                                     # nothing before the shortest comb delay: silence
    g = WS.reverb_gains(tuple(dl), WS.ir_length(rate))
    print("\nreverb %d Hz: sum |h| = %.2f, bound %.3g per unit of max |x|, largest share used %.4f"
          % (rate, g["G"], WS.reverb_bound(list(dl), 1.0, WS.ir_length(rate)), used))


def test_one_launch_mixes_the_ops_and_touches_nothing_else():
    clips, slots = [], []
    for i, (op, arg, n) in enumerate(WS.MIXED):
        clips.append(WS.gain_clip(500 + i, n, "middle") if op == WS.GAIN and n > 2 else WS.clip(500 + i, max(n, 2))[:n])
        slots.append((op, _gain_bits(arg) if op == WS.GAIN else WS.step_of(arg) if op == WS.RESAMPLE else 0))
    dl = list(WS.DELAYS_16K)
    outs, clean, bits = WS.launch(clips, slots, dl, DEV)
    assert clean                                                                       # behind dst_len[b], the pitch padding included: the NaN pattern
    assert len({o.size for o in outs}) >= 7 and bits.shape[1] % 4 == 0 and bits.shape[1] > max(o.size for o in outs)
    for (op, arg, n), (_, param), c, o in zip(WS.MIXED, slots, clips, outs):
        assert o.size == WS.out_len(n, op, param)
        if op == WS.COPY or param == WS.ONE:
            assert o.tobytes() == c.tobytes()                                          # op 0 and a resample at step 2^32: bit-for-bit copies
        elif op == WS.GAIN:
            _check_gain(c, arg, o, (op, n))
        elif op == WS.RESAMPLE:
            _check_resample(c, param, o, (op, n))
        else:
            _check_reverb(c, dl, 16000, o, (op, n))
    again = WS.launch(clips, slots, dl, DEV)[2]
    assert again.tobytes() == bits.tobytes()                                           # equal inputs, equal bits


# ---- the loader ------------------------------------------------------------------------------------------------------------------------------------------
def _clean_dict():
    dd = WC.loader_dataset_dict()
    del dd["train_ulb"]["data_s"]
    return dd


def _made_loader(normalize):
    c = WC.LOADER
    ds = DA.DeviceWaveDataset(_clean_dict()["train_ulb"]["data"], None, DEV)
    bu, per_epoch = c["batch_size"] * c["uratio"], c["num_train_iter"] // c["epoch"]
    return DA.WaveTrainLoader(ds, bu, DA.EpochSampler(len(ds), per_epoch * bu, 1, 0), c["L"], normalize, keys=("idx_ulb", "x_ulb_w", "x_ulb_s"),
                              seed=(c["seed"], 0, 1), device_strong=True, sample_rate=c["sample_rate"])


@pytest.mark.parametrize("normalize", (True, False), ids=("normalized", "raw"))
def test_loader_strong_view_is_the_restated_chain_of_its_draws(normalize):
    c, L, rate = WC.LOADER, WC.LOADER["L"], WC.LOADER["sample_rate"]
    ld = _made_loader(normalize)
    plain_lb, plain_ulb = WC.loader_pair(WC.loader_dataset_dict(), DEV, normalize=normalize)     # loaders without the key, the same seed
    clips, dl, BU, worst = WC.store_clips(ld.dataset), WS.delays(rate), ld.batch_size, 0.0
    for epoch in range(c["epoch"]):
        ld.set_epoch(epoch), plain_ulb.set_epoch(epoch)
        got = [{k: v.cpu().numpy() for k, v in b.items()} for b in ld]
        sd, (rows, crop) = ld.strong_draws, ld.draws["x_ulb_s"]
        assert len(got) == 2 and len({tuple(x) for x in sd["op"].tolist()}) >= 4
        for t, (b, p) in enumerate(zip(got, plain_ulb)):
            assert b["x_ulb_w"].tobytes() == p["x_ulb_w"].cpu().numpy().tobytes() and np.array_equal(b["idx_ulb"], p["idx_ulb"].cpu().numpy())
            assert b["x_ulb_s"].shape == (BU, L) and np.isfinite(b["x_ulb_s"]).all()
            for j in range(BU):
                i = BU * t + j
                y, e = WS.chain(clips[rows[i]], [(int(sd["op"][i, s]), int(sd["param"][i, s])) for s in (0, 1)], dl, rate)
                assert y.size == sd["lens"][i, 2]
                want = WC.oracle([y], [0], crop[i:i + 1], L, normalize)[0]
                v = np.zeros(L)
                w = y[crop[i]:crop[i] + L]
                v[:w.size] = w
                tol = WS.view_bound(want, v.var(), float(e.max())) if normalize else float(e.max())
                err = float(np.abs(b["x_ulb_s"][j] - want).max())
                worst = max(worst, err / tol)
                assert err <= tol, (epoch, i, sd["op"][i].tolist(), err, tol)
        again = [{k: v.cpu().numpy() for k, v in b.items()} for b in ld]               # iterating the epoch again replays it bit for bit
        assert all(x[k].tobytes() == y[k].tobytes() for x, y in zip(got, again) for k in x)
    print("\nloader strong views (normalize %s): largest share of the composed bound used %.4f" % (normalize, worst))
    if normalize:                                                                      # x_lb: the labelled loader never sees the key
        a = argparse.Namespace(device_audio=True, device_audio_strong=True, sample_rate=rate, max_length_seconds=c["max_length_seconds"],
                               audio_do_normalize=True, batch_size=c["batch_size"], uratio=c["uratio"], eval_batch_size=c["eval_batch_size"],
                               seed=c["seed"], train_sampler="RandomSampler")
        built = DA.build_wave_loaders(a, DA.build_wave_datasets(a, _clean_dict(), DEV), ["x_lb", "y_lb", "idx_ulb", "x_ulb_w", "x_ulb_s"],
                                      c["num_train_iter"], c["epoch"], 1, 0)
        for x, y in zip(built["train_lb"], plain_lb):
            assert list(x) == list(y) and all(x[k].cpu().numpy().tobytes() == y[k].cpu().numpy().tobytes() for k in x)
        for x, y in zip(built["train_ulb"], _made_loader(True)):
            assert all(x[k].cpu().numpy().tobytes() == y[k].cpu().numpy().tobytes() for k in x)


def test_srflexmatch_trains_on_device_made_strong_views():
    c = WC.LOADER
    args = argparse.Namespace(
        algorithm="srflexmatch", thresh_warmup=True, num_classes=c["num_classes"], num_train_iter=2, epoch=1, ema_m=0.0, ulb_loss_ratio=1.0, use_cat=False,
        amp=False, optim="AdamW", lr=5e-4, weight_decay=5e-4, layer_decay=0.75, num_warmup_iter=0, T=0.5, hard_label=True, p_cutoff=0.95, N_k=2,
        start_timing=2, feature_dim=128, sr_lr=5e-4, sr_ema=False, sr_ema_m=0.99, num_eval_iter=0, num_log_iter=2, gpu=0, rank=0, world_size=1,
        distributed=False, dataset="urbansound8k", sample_rate=c["sample_rate"], max_length_seconds=c["max_length_seconds"], batch_size=c["batch_size"],
        uratio=c["uratio"], eval_batch_size=c["eval_batch_size"], train_sampler="RandomSampler", seed=c["seed"], device_audio=True,
        device_audio_strong=True, audio_do_normalize=True, dataset_dict=_clean_dict())
    alg = get_algorithm(args, wave2vec.wave2vecv2_tiny_test)
    ulb = alg.loader_dict["train_ulb"]
    assert ulb.makes_strong and ulb.keys == ("idx_ulb", "x_ulb_w", "x_ulb_s") and alg.dataset_dict["train_ulb"].n_variants == 0
    losses, step = [], alg.train_step
    BU, L = c["batch_size"] * c["uratio"], c["L"]

    @functools.wraps(step)
    def recording(**kw):
        s, w = kw["x_ulb_s"], kw["x_ulb_w"]
        assert s.is_cuda and s.shape == w.shape == (BU, L) and s.is_contiguous() and bool(torch.isfinite(s).all())
        assert bool((s != w).any(dim=1).all())                                         # every strong row differs from its weak row
        out, log = step(**kw)
        losses.append(log["train/total_loss"])
        return out, log
    alg.train_step = recording
    alg.train()
    torch.cuda.synchronize()
    assert alg.it == 2 and len(losses) == 2 and all(np.isfinite(float(v)) for v in losses)
