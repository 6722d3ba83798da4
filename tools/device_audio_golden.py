"""Write tests/golden/device_audio.npz: what the waveform store, its loaders (semireward_amd/data/device_audio.py) and srhip_wave_view
(csrc/wave_view.hip) are pinned to.

TEST INFRASTRUCTURE (build container only, like tools/gen_device_data_golden.py): needs transformers and the reference tree, runs on the CPU; the
tests and everything that runs on the GPU machine read only the fixture.  Arrays only (the clips are rebuilt from their seeds by
tests/_wave_view_cases.py):

  * fx/<batch>/offsets [N_OFFSET_SEEDS, clips]: the offset of the window the reference's own random_subsample (semilearn/datasets/utils.py) returned
    for every clip of the ragged batch under random.seed(k);
  * fx/<batch>/pad_true, pad_max, pad_true_short: Wav2Vec2FeatureExtractor's float32 output for the windows of seed 0 with padding=True (the
    whole batch, and the sub-batch of clips shorter than S) and padding='max_length' -- the calls of the reference's collator
    (semilearn/datasets/collactors/audio_collactor.py:61-83), do_normalize=True, return_attention_mask=False as in both checkpoints'
    preprocessor_config.json;
  * kernel/<case>/d_ref: max |extractor float32 - oracle float64| of every kernel case, the measured float32 error the GPU test's bound is built on;
  * loader/d_ref, loader/eval_d_ref, loader/eval_lengths: the same for the views the loaders of the test configuration draw (two epochs), and the
    lengths the extractor pads the evaluation batches to.

    PYTHONDONTWRITEBYTECODE=1 python tools/device_audio_golden.py
"""
import importlib.util
import os
import random
import sys

import numpy as np
import transformers
from transformers import Wav2Vec2FeatureExtractor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _wave_view_cases as WC  # noqa: E402
from oracle import _ref_import as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "device_audio.npz")


def reference_random_subsample():
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("_ref_dataset_utils", os.path.join(R.REF, "semilearn", "datasets", "utils.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.random_subsample


def extractor(rate):
    return Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=rate, padding_value=0.0, do_normalize=True, return_attention_mask=False)


def extract(windows, S, padding, rate=16000):
    """The collator's call (audio_collactor.py:61-69 / :75-83) on a list of windows."""
    return extractor(rate)(list(windows), padding=padding, max_length=S, sampling_rate=rate, truncation=True, return_tensors="np")["input_values"]


def offset_of(w, c):
    return (w.__array_interface__["data"][0] - c.__array_interface__["data"][0]) // c.itemsize


def main():
    out = {"meta/transformers": np.array(transformers.__version__)}
    subsample = reference_random_subsample()
    for name, f in WC.FIXTURE_BATCHES.items():
        S, clips = f["S"], WC.fixture_clips(name)
        offs = np.zeros((WC.N_OFFSET_SEEDS, len(clips)), dtype=np.int64)
        for k in range(WC.N_OFFSET_SEEDS):
            random.seed(k)
            wins = [subsample(c, max_length=1.0, sample_rate=S) for c in clips]          # int(round(sample_rate * max_length)) = S
            assert all(w.size == min(c.size, S) for w, c in zip(wins, clips))
            offs[k] = [offset_of(w, c) for w, c in zip(wins, clips)]
            if k == 0:
                out[f"fx/{name}/pad_true"] = extract(wins, S, True)
                out[f"fx/{name}/pad_max"] = extract(wins, S, "max_length")
                out[f"fx/{name}/pad_true_short"] = extract([wins[i] for i in f["short"]], S, True)
        out[f"fx/{name}/offsets"] = offs
    worst = 0.0
    for case in WC.kernel_cases():
        wins = [WC.window(case["clips"][r], c, case["S"]) for r, c in zip(case["src_row"], case["crop_off"])]
        got = extract(wins, case["S"], "max_length")
        want = WC.oracle(case["clips"], case["src_row"], case["crop_off"], case["S"], True)
        assert got.dtype == np.float32 and got.shape == want.shape
        d = float(np.abs(got - want).max())
        out["kernel/%s/d_ref" % case["name"]] = np.array(d)
        worst = max(worst, d / WC.ulp32(np.abs(want).max()))
    print("kernel cases: largest d_ref = %.2f ulp_fp32(max |out|)" % worst)
    # the loaders' own draws (host side only: no launch)
    from semireward_amd.data import device_audio as DA
    c, dd = WC.LOADER, WC.loader_dataset_dict()
    d_ref = 0.0
    for ld in WC.loader_pair(dd, "cpu"):
        clips = WC.store_clips(ld.dataset)
        for epoch in range(c["epoch"]):
            ld.set_epoch(epoch)
            ld._epoch_table()
            for key, (src, crop) in ld.draws.items():
                for s in range(0, len(ld) * ld.batch_size, ld.batch_size):
                    r, o = src[s:s + ld.batch_size], crop[s:s + ld.batch_size]
                    got = extract([WC.window(clips[i], j, c["L"]) for i, j in zip(r, o)], c["L"], "max_length", c["sample_rate"])
                    d_ref = max(d_ref, float(np.abs(got - WC.oracle(clips, r, o, c["L"], True)).max()))
    out["loader/d_ref"] = np.array(d_ref)
    ev = DA.DeviceWaveDataset.from_reference(dd["eval"], "cpu")
    clips, lengths, d_ref = WC.store_clips(ev), [], 0.0
    for s in range(0, len(ev), c["eval_batch_size"]):
        r = np.arange(s, min(s + c["eval_batch_size"], len(ev)))
        got = extract([clips[i] for i in r], c["L"], True, c["sample_rate"])          # is_train=False: the clip whole, truncated by the collator
        lengths.append(got.shape[1])
        d_ref = max(d_ref, float(np.abs(got - WC.oracle(clips, r, np.zeros(len(r), dtype=np.int64), got.shape[1], True)).max()))
    out["loader/eval_lengths"], out["loader/eval_d_ref"] = np.array(lengths, dtype=np.int64), np.array(d_ref)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
