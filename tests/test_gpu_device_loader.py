"""device_data on the MI355X: srhip_resize_bilinear_u8 against Pillow's recorded bytes (tests/golden/device_data.npz), the device train loader
against the numpy augmentation oracle applied to the fixture-checked resized images with the loader's own logged draws, reproducibility
across loaders / epochs, and ``alg.train()`` / ``alg.evaluate()`` fed by the loaders for SRFlexMatch + ViT-S/2 and SRPseudoLabel + WRN-28-2.
Every comparison is exact."""
import argparse
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import augment_ref as A                                    # noqa: E402
from oracle.gen_golden import synth_image                              # noqa: E402
from semireward_amd import _lib, ops                                   # noqa: E402
from semireward_amd.algorithms import get_algorithm                    # noqa: E402
from semireward_amd.data import device_loader as DL                    # noqa: E402
from semireward_amd.data.augment import GpuAugment                     # noqa: E402
from semireward_amd.data.resize import apply_tables                    # noqa: E402
from semireward_amd.nets import vit, wrn                               # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = DL.DATASET_STATS["cifar100"]


def _fixture_cases(g):
    for n in range(int(g["meta/n_resize"])):
        seed, H0, S, kind = [int(v) for v in g[f"resize/{n}/meta"]]
        yield synth_image(seed, H0, H0, kind), S, g[f"resize/{n}/out"]


# ---- 1. the kernel --------------------------------------------------------------------------------------------------------------------------
def test_resize_kernel_equals_pillow_bytes(golden):
    g = golden("device_data")
    by_pair = {}
    for im, S, want in _fixture_cases(g):
        by_pair.setdefault((im.shape[0], S), []).append((im, want))
    assert set(by_pair) == {(64, 32), (28, 32), (96, 32), (64, 96)}
    for (H0, S), cs in by_pair.items():
        src = torch.from_numpy(np.stack([c[0] for c in cs])).to(DEV)
        got = ops.resize_bilinear_u8(src, S)
        again = ops.resize_bilinear_u8(src, S)
        assert got.shape == (len(cs), S, S, 3) and got.dtype == torch.uint8
        for t, (_, want) in enumerate(cs):                      # each stored case on its own, and as part of a batch
            assert np.array_equal(got[t].cpu().numpy(), want), (H0, S, t)
            assert np.array_equal(ops.resize_bilinear_u8(src[t:t + 1], S)[0].cpu().numpy(), want), (H0, S, t)
        assert torch.equal(got, again)                          # two launches, equal bytes
        assert torch.equal(ops.resize_bilinear_u8(src, S, chunk=2), got)          # launches of 2 + 1 images share one scratch plane
    src = torch.from_numpy(np.stack([synth_image(5 + t, 32, 32, t % 3) for t in range(5)])).to(DEV)
    same = ops.resize_bilinear_u8(src, 32)                     # H0 == S: the input bytes, in a new tensor
    assert torch.equal(same, src) and same.data_ptr() != src.data_ptr()
    with pytest.raises(RuntimeError, match="invalid argument"):               # the C entry refuses non-square sources itself (SR_EINVAL)
        ops._call("srhip_resize_bilinear_u8", src.data_ptr(), 5, 32, 16, same.data_ptr(), 32, None, None, 0, None, ops._s())
    with pytest.raises(ValueError, match="square"):
        ops.resize_bilinear_u8(src[:, :, :16].contiguous(), 32)


def test_resize_kernel_other_sizes_match_the_host_passes():
    """Sizes outside the fixture (the host passes are pinned to Pillow by tests/test_cpu_device_loader.py): 32 -> 224, 96 -> 224, odd sizes."""
    for H0, S in [(32, 224), (96, 224), (50, 17), (17, 50), (64, 1)]:
        im = np.stack([synth_image(40 + H0 + t, H0, H0, t % 3) for t in range(3)])
        got = ops.resize_bilinear_u8(torch.from_numpy(im).to(DEV), S).cpu().numpy()
        assert np.array_equal(got, apply_tables(im, S)), (H0, S)


# ---- 2. the train loader against the oracle -------------------------------------------------------------------------------------------------------
class _LoggedAugment(GpuAugment):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.log = []

    def draw(self, B, strong, src_hw=None):
        d = super().draw(B, strong, src_hw)
        self.log.append(d)
        return d


def _dataset64(g, n, labelled, seed):
    """n 64 x 64 images: the fixture's three 64 -> 32 sources first (their resized bytes are Pillow's own), then other seeded images."""
    fx = [(im, want) for im, S, want in _fixture_cases(g) if im.shape[0] == 64 and S == 32]
    imgs = [im for im, _ in fx] + [synth_image(seed + t, 64, 64, t % 3) for t in range(n - len(fx))]
    rng = np.random.Generator(np.random.PCG64(seed))
    y = rng.integers(0, 10, size=n) if labelled else None
    ds = DL.DeviceImageDataset(np.stack(imgs), y, 32, DEV)
    resized = ds.data.cpu().numpy()
    assert ds.stored_size == 64 and resized.shape == (n, 32, 32, 3)
    for t, (_, want) in enumerate(fx):
        assert np.array_equal(resized[t], want)
    assert np.array_equal(resized, apply_tables(np.stack(imgs), 32))
    return ds, resized, y


def _want_view(img, d, t, pad, S):
    if "ops" in d:
        return A.strong(img, pad, S, int(d["i"][t]), int(d["j"][t]), bool(d["flip"][t]), d["ops"][t], d["vals"][t], float(d["cut_v"][t]),
                        float(d["ux"][t]), float(d["uy"][t]), MEAN, STD)
    return A.weak(img, pad, S, int(d["i"][t]), int(d["j"][t]), bool(d["flip"][t]), MEAN, STD)


def test_train_loader_views_equal_the_oracle_on_the_resized_images(golden):
    g = golden("device_data")
    S, pad = 32, 4
    lb, lb_img, y = _dataset64(g, 12, True, 300)
    ulb, ulb_img, _ = _dataset64(g, 30, False, 400)
    aug_l, aug_u = _LoggedAugment(S, pad, MEAN, STD, device=DEV), _LoggedAugment(S, pad, MEAN, STD, device=DEV)
    ld_l = DL.DeviceTrainLoader(lb, 4, DL.EpochSampler(12, 20, 1, 0), aug_l, keys=("idx_lb", "x_lb", "y_lb"), seed=(0, 0, 0))
    ld_u = DL.DeviceTrainLoader(ulb, 8, DL.EpochSampler(30, 40, 1, 0), aug_u, keys=("idx_ulb", "x_ulb_w", "x_ulb_s"), seed=(0, 0, 1))
    for epoch in (0, 1):
        ld_l.set_epoch(epoch), ld_u.set_epoch(epoch)
        sl, su = DL.EpochSampler(12, 20, 1, 0), DL.EpochSampler(30, 40, 1, 0)
        sl.set_epoch(epoch), su.set_epoch(epoch)
        sl, su = sl.indices(), su.indices()
        aug_l.log.clear(), aug_u.log.clear()
        steps = list(zip(ld_l, ld_u))
        assert len(steps) == 5 and len(aug_l.log) == 5 and len(aug_u.log) == 10
        for t, (bl, bu) in enumerate(steps):
            il, iu = sl[4 * t:4 * t + 4], su[8 * t:8 * t + 8]
            assert all(v.is_cuda for v in list(bl.values()) + list(bu.values()))
            assert np.array_equal(bl["idx_lb"].cpu().numpy(), il) and np.array_equal(bl["y_lb"].cpu().numpy(), y[il])
            assert np.array_equal(bu["idx_ulb"].cpu().numpy(), iu)
            x_lb, x_w, x_s = bl["x_lb"].cpu().numpy(), bu["x_ulb_w"].cpu().numpy(), bu["x_ulb_s"].cpu().numpy()
            assert x_lb.shape == (4, 3, S, S) and x_lb.dtype == np.float32 and x_s.shape == (8, 3, S, S)
            dl, dw, ds_ = aug_l.log[t], aug_u.log[2 * t], aug_u.log[2 * t + 1]
            assert "ops" not in dl and "ops" not in dw and "ops" in ds_
            for r in range(4):
                assert np.array_equal(x_lb[r], _want_view(lb_img[il[r]], dl, r, pad, S)), (epoch, t, r)
            for r in range(8):
                assert np.array_equal(x_w[r], _want_view(ulb_img[iu[r]], dw, r, pad, S)), (epoch, t, r)
                assert np.array_equal(x_s[r], _want_view(ulb_img[iu[r]], ds_, r, pad, S)), (epoch, t, r)


# ---- 3. reproducibility ---------------------------------------------------------------------------------------------------------------------------
def test_same_seed_same_batches_and_epochs_are_addressable(golden):
    g = golden("device_data")
    ulb, _, _ = _dataset64(g, 30, False, 500)
    keys = ("idx_ulb", "x_ulb_w", "x_ulb_s")

    def loader(seed):
        return DL.DeviceTrainLoader(ulb, 8, DL.EpochSampler(30, 24, 1, 0), GpuAugment(32, 4, MEAN, STD, device=DEV), keys=keys, seed=seed)

    def run(ld, epochs):
        out = []
        for e in epochs:
            ld.set_epoch(e)
            out.append([{k: v.cpu().numpy().copy() for k, v in b.items()} for b in ld])
        return out

    def same(a, b):
        return len(a) == len(b) and all(set(x) == set(y) and all(np.array_equal(x[k], y[k]) for k in x) for x, y in zip(a, b))
    a, b = run(loader((7, 0, 1)), (0, 1)), run(loader((7, 0, 1)), (0, 1))
    assert len(a[0]) == 3 and same(a[0], b[0]) and same(a[1], b[1])
    assert not same(a[0], a[1])
    second = run(loader((7, 0, 1)), (1,))[0]                    # set_epoch(1) directly: the second epoch of the uninterrupted loader
    assert same(second, a[1])
    c = run(loader((8, 0, 1)), (0,))[0]                         # another seed: the sampler's stream (seeded by the epoch) stays, the draws change
    assert all(np.array_equal(x["idx_ulb"], y["idx_ulb"]) for x, y in zip(a[0], c)) and not same(a[0], c)


# ---- 4. alg.train() / alg.evaluate() through the loaders -----------------------------------------------------------------------------------------
def _flex_args(dd, **kw):
    d = dict(algorithm="srflexmatch", num_classes=10, num_train_iter=6, epoch=2, ema_m=0.0, ulb_loss_ratio=1.0, use_cat=True, amp=False, lr=5e-4,
             weight_decay=5e-4, layer_decay=0.5, num_warmup_iter=0, optim="AdamW", T=0.5, p_cutoff=0.95, hard_label=True, thresh_warmup=True, N_k=2,
             start_timing=2, feature_dim=384, sr_lr=5e-4, sr_ema=False, sr_ema_m=0.99, num_eval_iter=0, num_log_iter=3, gpu=0, rank=0, world_size=1,
             distributed=False, dataset="cifar100", img_size=32, crop_ratio=0.875, batch_size=4, uratio=2, eval_batch_size=4,
             train_sampler="RandomSampler", seed=5, device_data=True, dataset_dict=dd)
    d.update(kw)
    return argparse.Namespace(**d)


def _dict_datasets(H0, n_lb=12, n_ulb=40, n_ev=10, C=10):
    rng = np.random.Generator(np.random.PCG64(H0))
    mk = lambda n, s: np.stack([synth_image(s + t, H0, H0, t % 3) for t in range(n)])      # noqa: E731
    return {"train_lb": {"data": mk(n_lb, 1000), "targets": rng.integers(0, C, size=n_lb)}, "train_ulb": {"data": mk(n_ulb, 2000), "targets": None},
            "eval": {"data": mk(n_ev, 3000), "targets": rng.integers(0, C, size=n_ev)}}


def test_srflexmatch_vit_trains_and_evaluates_through_the_device_loaders():
    dd = _dict_datasets(64)
    args = _flex_args(dd)
    alg = get_algorithm(args, vit.vit_small_patch2_32)
    assert args.ulb_dest_len == 40 and args.lb_dest_len == 12 and alg.hooks_dict["MaskingHook"].selected_label.numel() == 40
    assert "DistSamplerSeedHook" in alg.hooks_dict and alg.dataset_dict["train_ulb"].data.shape == (40, 32, 32, 3)
    seen, losses, step = [], [], alg.train_step

    @functools.wraps(step)
    def recording(**kw):
        assert all(v.is_cuda for v in kw.values()) and kw["x_ulb_s"].shape == (8, 3, 32, 32) and kw["x_lb"].shape == (4, 3, 32, 32)
        seen.append(kw["idx_ulb"].cpu().numpy().copy())
        out, log = step(**kw)
        losses.append(log["train/total_loss"])
        return out, log
    alg.train_step = recording
    alg.train()                                                 # no batches= argument: the loaders feed the loop, across the epoch boundary
    torch.cuda.synchronize()
    assert alg.it == 6 and alg.epoch == 1 and alg.optimizer.step_count == 6 and len(seen) == 6
    assert all(np.isfinite(float(v)) for v in losses)
    want = []
    for e in (0, 1):
        s = DL.EpochSampler(40, 3 * 8, 1, 0)
        s.set_epoch(e)
        want.append(s.indices())
    assert np.array_equal(np.concatenate(seen), np.concatenate(want))
    touched = np.nonzero(alg.hooks_dict["MaskingHook"].selected_label.cpu().numpy() != -1)[0]
    assert set(touched.tolist()) <= set(np.concatenate(want).tolist())          # the FlexMatch table was indexed by the sampler's idx_ulb only
    # evaluation over the device eval loader == evaluation over host tensors of the same transformed images
    ev = alg.evaluate("eval")
    host = [{k: v.cpu() for k, v in b.items()} for b in alg.loader_dict["eval"]]
    assert [int(b["y_lb"].shape[0]) for b in host] == [4, 4, 2]
    assert np.array_equal(torch.cat([b["y_lb"] for b in host]).numpy(), np.asarray(dd["eval"]["targets"]))
    ev_host = alg.evaluate("eval", loader=host)
    assert ev == ev_host and np.isfinite(ev["eval/loss"]) and {"eval/top-1-acc", "eval/F1"} <= set(ev)
    val = apply_tables(dd["eval"]["data"], 32)                 # transform_val: Resize, ToTensor, Normalize
    x = torch.cat([b["x_lb"] for b in host]).numpy()
    assert all(np.array_equal(x[t], A.to_tensor_normalize(val[t], MEAN, STD)) for t in range(len(val)))


# ---- 5. an algorithm without a strong view ----------------------------------------------------------------------------------------------------------
def test_srpseudolabel_wrn_steps_from_the_loaders_without_a_strong_launch(monkeypatch):
    from semireward_amd import config as srconfig
    dd = _dict_datasets(32, n_lb=16, n_ulb=48, n_ev=8, C=100)
    args = srconfig.get_config(os.path.join(ROOT, "configs", "classic_cv_srpseudolabel_cifar100_400_wrn_28_2.yaml"),
                               overrides=dict(gpu=0, rank=0, world_size=1, distributed=False, batch_size=8, eval_batch_size=8, num_train_iter=8, epoch=2,
                                              device_data=True, dataset_dict=dd))
    alg = get_algorithm(args, wrn.wrn_28_2)
    assert alg.loader_dict["train_ulb"].keys == ("idx_ulb", "x_ulb_w") and len(alg.loader_dict["train_lb"]) == 4
    h = _lib.lib()
    real, calls = h.srhip_augment, []
    monkeypatch.setattr(h, "srhip_augment", lambda *a: (calls.append(a[4]), real(*a))[1])
    data_lb, data_ulb = next(iter(alg.loader_dict["train_lb"])), next(iter(alg.loader_dict["train_ulb"]))
    assert calls == [8, 8] and "x_ulb_s" not in data_ulb         # x_lb and x_ulb_w: two launches of 8 images, no third
    alg.model.train()
    alg.out_dict, alg.log_dict = alg.train_step(**alg.process_batch(**data_lb, **data_ulb))
    alg.call_hook("after_train_step")
    torch.cuda.synchronize()
    assert np.isfinite(float(alg.log_dict["train/total_loss"])) and alg.optimizer.step_count == 1 and calls == [8, 8]


# ---- 6. the example ----------------------------------------------------------------------------------------------------------------------------------
def test_train_device_loader_example_learns(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_device_loader as ex
    monkeypatch.setattr(sys, "argv", ["train_device_loader.py", "--steps", "100"])
    ev = ex.main()
    assert all(np.isfinite(float(v)) for v in ev.values())
    # measured once on an MI355X: top-1 1.0000 (eval/loss 0.1737) after 100 steps; chance is 1 / 10 classes.  The bar is half-way between the two.
    assert ev["eval/top-1-acc"] > 0.5 * (0.1 + 1.0)
