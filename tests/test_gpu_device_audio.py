"""device_audio on the MI355X: srhip_wave_view against the float64 oracle of tests/_wave_view_cases.py, element by element, at every size and
geometry the kernel branches on; the waveform loaders against the oracle applied to their own logged draws; ``alg.train()`` / ``alg.evaluate()``
fed by the loaders for SRPseudoLabel and SRFreeMatch on the tiny Wav2Vec2.

Bound (tests/_wave_view_cases.py): normalize = 0 is bit-exact; normalize = 1 stays within 4 d_ref + 4 ulp_fp32(max |out|) per element, d_ref the
float32 extractor's own distance from the oracle, measured on the CPU and stored in tests/golden/device_audio.npz.  Measured headroom per case:
profiles/device_audio.txt."""
import argparse
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _wave_view_cases as WC                                          # noqa: E402
from semireward_amd import ops                                         # noqa: E402
from semireward_amd.algorithms import get_algorithm                    # noqa: E402
from semireward_amd.data import device_audio as DA                     # noqa: E402
from semireward_amd.nets import wave2vec                               # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
launch, NAN_BITS = WC.launch, WC.NAN_BITS


@pytest.mark.parametrize("S", WC.KERNEL_S)
def test_wave_view_against_the_float64_oracle(golden, S):
    g, report = golden("device_audio"), []
    for geom in WC.GEOMETRIES:
        case = WC.kernel_case(S, geom)
        d_ref = float(g["kernel/%s/d_ref" % case["name"]])
        err, tol = WC.verify(case, d_ref, DEV)
        report.append("%-14s d_ref %.3e  kernel %.3e  bound %.3e  used %.3f" % (case["name"], d_ref, err, tol, err / tol))
    print("\n" + "\n".join(report))
    assert len(report) == len(WC.GEOMETRIES)


def test_wave_view_exact_cases():
    """Statistics that are exact in any order (0.5 over a power of two, zeros): the kernel returns fp32(oracle) bit for bit."""
    for case in WC.exact_cases():
        ds = DA.DeviceWaveDataset(case["clips"], None, DEV)
        for normalize in (0, 1):
            got, past = launch(ds, case["src_row"], case["crop_off"], case["S"], normalize)
            want = WC.oracle(case["clips"], case["src_row"], case["crop_off"], case["S"], bool(normalize)).astype(np.float32)
            assert np.array_equal(got, want) and (past == NAN_BITS).all(), (case["name"], normalize)
    S = 256
    full, _ = launch(DA.DeviceWaveDataset([np.full(S + 8, 0.5, dtype=np.float32)], None, DEV), [0, 0], [3, S // 2 + 8], S, 1)
    assert not full[0].any()                                                   # mean 0.5, variance 0: (0.5 - 0.5) / sqrt(1e-7)
    assert np.array_equal(full[1, :S // 2], np.full(S // 2, np.float32(0.25 / np.sqrt(0.0625 + 1e-7))))        # mean 0.25, variance 1 / 16
    assert np.array_equal(full[1, S // 2:], np.full(S // 2, np.float32(-0.25 / np.sqrt(0.0625 + 1e-7))))       # the padding: -m / sigma


def test_wave_view_entry_refusals_on_device_pointers():
    ds = DA.DeviceWaveDataset([WC.clip(1, 40)], None, DEV)
    r, c = torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    out = torch.zeros(2, 16, device=DEV)

    def call(**kw):
        a = dict(store=ds.store.data_ptr(), off=ds.row_off.data_ptr(), ln=ds.row_len.data_ptr(), n=1, r=r.data_ptr(), c=c.data_ptr(), B=2, S=10, norm=1,
                 out=out.data_ptr(), ldo=16, stream=ops._s())
        a.update(kw)
        ops._call("srhip_wave_view", *a.values())
    call()
    torch.cuda.synchronize()
    for kw in (dict(B=0), dict(B=65536), dict(S=0), dict(S=17), dict(ldo=14), dict(out=out.data_ptr() + 4), dict(store=None), dict(c=None)):
        with pytest.raises(RuntimeError, match="invalid argument"):
            call(**kw)
    with pytest.raises(IndexError, match="crop_off outside"):                 # the wrapper refuses what the kernel would clamp
        ops.wave_view(ds.store, ds.row_off, ds.row_len, r, c + 40, 10, True, host=(np.zeros(2, dtype=np.int64), np.full(2, 40), ds.row_len_host))


# ---- the loaders ---------------------------------------------------------------------------------------------------------------------------------
def test_train_loader_batches_equal_the_oracle_on_their_own_draws(golden):
    g, c, dd = golden("device_audio"), WC.LOADER, WC.loader_dataset_dict()
    d_ref, L = float(g["loader/d_ref"]), c["L"]
    pair, twin = WC.loader_pair(dd, DEV), WC.loader_pair(dd, DEV)
    worst = 0.0
    for epoch in range(c["epoch"]):
        for ld, other in zip(pair, twin):
            ld.set_epoch(epoch), other.set_epoch(epoch)
            clips = WC.store_clips(ld.dataset)
            a, b = [{k: v.cpu().numpy() for k, v in x.items()} for x in ld], [{k: v.cpu().numpy() for k, v in x.items()} for x in other]
            assert len(a) == len(b) == len(ld) == 2
            for t, (x, y) in enumerate(zip(a, b)):
                assert list(x) == list(ld.keys) and all(x[k].tobytes() == y[k].tobytes() for k in x)       # two loaders, one seed: the same bits
                for k, (src, crop) in ld.draws.items():
                    n = ld.batch_size
                    want = WC.oracle(clips, src[n * t:n * t + n], crop[n * t:n * t + n], L, True)
                    assert x[k].shape == want.shape and x[k].dtype == np.float32
                    err, tol = float(np.abs(x[k] - want).max()), WC.bound(d_ref, want)
                    worst = max(worst, err / tol)
                    assert err <= tol, (epoch, t, k, err, tol)
    print("\nloader views: d_ref %.3e, largest share of the bound used %.3f" % (d_ref, worst))
    raw = WC.loader_pair(dd, DEV, normalize=False)[1]                            # do_normalize: False: the stored samples themselves
    x = next(iter(raw))
    clips = WC.store_clips(raw.dataset)
    for k, (src, crop) in raw.draws.items():
        assert x[k].cpu().numpy().tobytes() == WC.oracle(clips, src[:8], crop[:8], L, False).astype(np.float32).tobytes()


def _args(dd, **kw):
    c = WC.LOADER
    d = dict(num_classes=c["num_classes"], num_train_iter=c["num_train_iter"], epoch=c["epoch"], ema_m=0.0, ulb_loss_ratio=1.0, use_cat=False, amp=False,
             optim="AdamW", lr=5e-4, weight_decay=5e-4, layer_decay=0.75, num_warmup_iter=0, T=0.5, hard_label=True, p_cutoff=0.95, N_k=2, start_timing=2,
             feature_dim=128, sr_lr=5e-4, sr_ema=False, sr_ema_m=0.99, num_eval_iter=0, num_log_iter=2, gpu=0, rank=0, world_size=1, distributed=False,
             dataset="urbansound8k", sample_rate=c["sample_rate"], max_length_seconds=c["max_length_seconds"], batch_size=c["batch_size"],
             uratio=c["uratio"], eval_batch_size=c["eval_batch_size"], train_sampler="RandomSampler", seed=c["seed"], device_audio=True,
             audio_do_normalize=True, dataset_dict=dd)
    d.update(kw)
    return argparse.Namespace(**d)


ALGS = {"srpseudolabel": dict(algorithm="srpseudolabel", unsup_warm_up=0.4),
        "srfreematch": dict(algorithm="srfreematch", ema_p=0.9, use_quantile=True, clip_thresh=False, ent_loss_ratio=0.05)}


@pytest.mark.parametrize("name", sorted(ALGS))
def test_train_and_evaluate_through_the_wave_loaders(golden, name):
    g, c, dd = golden("device_audio"), WC.LOADER, WC.loader_dataset_dict()
    strong = name == "srfreematch"
    if not strong:
        del dd["train_ulb"]["data_s"]                                            # SRPseudoLabel needs no strong view, hence no variants
    args = _args(dd, **ALGS[name])
    alg = get_algorithm(args, wave2vec.wave2vecv2_tiny_test)
    assert args.ulb_dest_len == c["n_ulb"] and args.lb_dest_len == len(c["lb_lens"]) and "DistSamplerSeedHook" in alg.hooks_dict
    assert alg.loader_dict["train_ulb"].keys == (("idx_ulb", "x_ulb_w", "x_ulb_s") if strong else ("idx_ulb", "x_ulb_w"))
    assert alg.dataset_dict["train_ulb"].n_variants == (c["V"] if strong else 0)
    seen, losses, step = [], [], alg.train_step
    B, BU, L = c["batch_size"], c["batch_size"] * c["uratio"], c["L"]

    @functools.wraps(step)
    def recording(**kw):
        assert all(v.is_cuda for v in kw.values()) and kw["x_lb"].shape == (B, L) and kw["x_ulb_w"].shape == (BU, L) and kw["x_lb"].is_contiguous()
        assert ("x_ulb_s" in kw) == strong and (not strong or kw["x_ulb_s"].shape == (BU, L))
        seen.append(kw["y_lb"].cpu().numpy().copy())
        out, log = step(**kw)
        losses.append(log["train/total_loss"])
        return out, log
    alg.train_step = recording
    alg.train()                                                                   # no batches= argument: the loaders feed the loop, across the epoch boundary
    torch.cuda.synchronize()
    assert alg.it == c["num_train_iter"] == 4 and alg.epoch == 1 and alg.optimizer.step_count == 4 and len(seen) == 4
    assert all(np.isfinite(float(v)) for v in losses)
    want = []
    for e in (0, 1):
        s = DA.EpochSampler(len(c["lb_lens"]), 2 * B, 1, 0)
        s.set_epoch(e)
        want.append(np.asarray(dd["train_lb"]["targets"])[s.indices()])
    assert np.array_equal(np.concatenate(seen), np.concatenate(want))
    # evaluation: the reference's per-batch lengths, the same metrics from host copies of the batches and with device_eval on top
    ev = alg.evaluate("eval")
    host = [{k: v.cpu() for k, v in b.items()} for b in alg.loader_dict["eval"]]
    assert [tuple(b["x_lb"].shape) for b in host] == [(3, n) if i < 2 else (2, n) for i, n in enumerate(g["loader/eval_lengths"].tolist())]
    assert np.array_equal(torch.cat([b["y_lb"] for b in host]).numpy(), np.asarray(dd["eval"]["targets"]))
    assert ev == alg.evaluate("eval", loader=host) and np.isfinite(ev["eval/loss"]) and {"eval/top-1-acc", "eval/F1"} <= set(ev)
    clips, d_ref, s = WC.store_clips(alg.dataset_dict["eval"]), float(g["loader/eval_d_ref"]), 0
    for b in host:
        n, S = b["x_lb"].shape
        w = WC.oracle(clips, np.arange(s, s + n), np.zeros(n, dtype=np.int64), S, True)
        assert float(np.abs(b["x_lb"].numpy() - w).max()) <= WC.bound(d_ref, w)
        s += n
    alg.device_eval = True
    on_device = alg.evaluate("eval")
    assert set(on_device) == set(ev) and all(on_device[k] == ev[k] for k in ev if k != "eval/loss")
    # both losses are fp32 row arithmetic, each within 2e-6 (relative) of the float64 value: the bound of tests/test_gpu_run_hooks.py
    assert abs(on_device["eval/loss"] - ev["eval/loss"]) <= 2 * 2e-6 * abs(ev["eval/loss"])


# ---- the example ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [["--steps", "8"], ["--steps", "8", "--algorithm", "srfreematch"], ["--steps", "24", "--run-hooks"]],
                         ids=["srpseudolabel", "srfreematch", "run_hooks"])
def test_train_device_audio_example_runs(monkeypatch, argv):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_device_audio as ex
    monkeypatch.setattr(sys, "argv", ["train_device_audio.py"] + argv)
    ev = ex.main()
    assert {"eval/loss", "eval/top-1-acc"} <= set(ev) and all(np.isfinite(float(v)) for v in ev.values())
