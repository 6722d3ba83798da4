"""device_tokens_strong on the MI355X: every srhip_token_strong launch (csrc/token_strong.hip) against the integer restatement of
tests/_token_strong_cases.py -- the whole sentinel-guarded [rows, ld_ids] buffer and key_len, bit for bit, every launch made twice --; the token
loaders' strong batches against the restatement applied to their recorded draws, the weak views against a loader without the key, one
host-to-device copy per loader and epoch; SRFlexMatch and SRSoftMatch trained through ``alg.train()`` with the key and no data_s.  Integer
results: every comparison is exact, there is no tolerance."""
import argparse
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _token_strong_cases as TS                                       # noqa: E402
from semireward_amd import ops                                         # noqa: E402
from semireward_amd.algorithms import get_algorithm                    # noqa: E402
from semireward_amd.data import device_tokens as DT                    # noqa: E402
from semireward_amd.data.device_loader import EpochSampler             # noqa: E402
from semireward_amd.nets import bert                                   # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in TS.kernel_cases()}
ULB_KEYS = ("idx_ulb", "x_ulb_w", "x_ulb_s")


@pytest.mark.parametrize("name", sorted(CASES))
def test_token_strong_against_the_restatement(name):
    c = CASES[name]
    store = TS.store_of(c, DEV)
    assert store[0].data_ptr() % 16 == 0 and (store[1].cpu().numpy() % 4 != 0).any() == c["tight"]
    want = TS.expected(c)
    first, second = TS.launch(c, DEV, store), TS.launch(c, DEV, store)
    bad = TS.mismatches(c, *first, want=want)
    assert bad == [], (name, "rows (1 = output row 0; 0 and the last are guard rows) that differ from the restatement", bad[:10],
                       [(int(c["src_row"][b - 1]), TS.unpack(int(c["slots"][0, b - 1])), TS.unpack(int(c["slots"][1, b - 1]))) for b in bad[:3] if 0 < b <= c["src_row"].size])
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])        # equal inputs give equal bits
    assert first[1].dtype == np.int32 and first[1][1:-1].max() <= c["L"]


def test_wrapper_returns_token_view_shaped_results_and_refuses_before_launching():
    c = CASES["pairs"]
    flat, off, lens = TS.store_of(c, DEV)
    lens_host = lens.cpu().numpy()
    src, slots = torch.from_numpy(c["src_row"]).to(DEV), torch.from_numpy(c["slots"]).to(DEV)
    want, want_kl = TS.strong_batch_ref(c["rows"], c["src_row"], c["slots"], c["L"], c["Lsrc"], c["pad_id"], c["mask_id"])
    ids, kl = ops.token_strong(flat, off, lens, src, slots[0], slots[1], c["L"], c["Lsrc"], c["pad_id"], c["mask_id"],
                               host=(c["src_row"], c["slots"], lens_host))
    assert ids.is_contiguous() and ids.dtype == torch.int64 and kl.dtype == torch.int32 and tuple(ids.shape) == (src.numel(), c["L"])
    assert np.array_equal(ids.cpu().numpy(), want) and np.array_equal(kl.cpu().numpy(), want_kl)
    # two copies: a strong view of COPY slots is the token view
    zero = torch.zeros_like(slots[0])
    a, a_kl = ops.token_strong(flat, off, lens, src, zero, zero, c["L"], c["Lsrc"], c["pad_id"], c["mask_id"])
    b, b_kl = ops.token_view(flat, off, lens, src, c["L"], c["pad_id"])
    assert torch.equal(a, b) and torch.equal(a_kl, b_kl)
    out, okl = torch.zeros(2, 16, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)

    def call(**kw):
        a = dict(store=flat.data_ptr(), off=off.data_ptr(), ln=lens.data_ptr(), n=len(c["rows"]), r=src.data_ptr(), s0=slots[0].data_ptr(),
                 s1=slots[1].data_ptr(), B=2, Lsrc=8, L=10, pad=0, mask=103, ids=out.data_ptr(), ld=16, kl=okl.data_ptr(), stream=ops._s())
        a.update(kw)
        ops._call("srhip_token_strong", *a.values())
    call()
    torch.cuda.synchronize()
    for kw in (dict(store=None), dict(off=None), dict(ln=None), dict(r=None), dict(s0=None), dict(s1=None), dict(ids=None), dict(kl=None), dict(n=0),
               dict(B=0), dict(B=65536), dict(Lsrc=0), dict(Lsrc=4097), dict(L=0), dict(L=17), dict(ld=9), dict(store=flat.data_ptr() + 4),
               dict(store=flat.data_ptr() + 8), dict(ids=out.data_ptr() + 4), dict(pad=-1), dict(mask=-1)):
        with pytest.raises(RuntimeError, match="invalid argument"):
            call(**kw)
    launched, real = [], ops._call
    try:
        ops._call = lambda *a: launched.append(a)
        bad = c["slots"].copy()
        bad[1, 0] = TS.pack(7, 0, 0)
        for exc, match, h in ((IndexError, "src_row outside the store's 4 rows", (np.where(np.arange(src.numel()) == 3, 4, c["src_row"]), c["slots"], lens_host)),
                              (ValueError, "slot 1 holds op 7", (c["src_row"], bad, lens_host))):
            with pytest.raises(exc, match=match):                                                # the wrapper refuses what the kernel would mend
                ops.token_strong(flat, off, lens, src, slots[0], slots[1], c["L"], c["Lsrc"], host=h)
        with pytest.raises(ValueError, match="L = 100 is below the 257 tokens"):
            ops.token_strong(flat, off, lens, src, slots[0], slots[1], 100, c["Lsrc"], host=(c["src_row"], c["slots"], lens_host))
    finally:
        ops._call = real
    assert not launched                                                                           # ... before launching


# ---- the loaders ---------------------------------------------------------------------------------------------------------------------------------
def _loader(dd, device_strong, **kw):
    c = TS.LOADER
    ds = DT.DeviceTokenDataset.from_reference(dd["train_ulb"], DEV, None, c["max_length"])
    bu, per_epoch = c["batch_size"] * c["uratio"], c["num_train_iter"] // c["epoch"]
    return DT.TokenTrainLoader(ds, bu, EpochSampler(len(ds), per_epoch * bu, 1, 0), keys=ULB_KEYS, seed=(c["seed"], 0, 1), device_strong=device_strong, **kw)


def _equals_restatement(batch, loader, t, rows, mask_id):
    ids, kl = TS.loader_batch_ref(loader, t, rows, mask_id=mask_id)
    assert isinstance(batch, bert.TokenBatch) and batch.ids.is_cuda and batch.ids.is_contiguous() and batch.seq_len is None
    assert batch.ids.dtype == torch.int64 and batch.key_len.dtype == torch.int32 and (batch.S, batch.L) == ids.shape
    assert np.array_equal(batch.ids.cpu().numpy(), ids) and np.array_equal(batch.key_len.cpu().numpy(), kl)
    return ids


def test_loader_batches_equal_the_restatement_of_the_recorded_draws(monkeypatch):
    copies, real = [], DT._h2d
    monkeypatch.setattr(DT, "_h2d", lambda t, d: (copies.append(tuple(t.shape)), real(t, d))[1])
    ld, plain = _loader(TS.loader_dataset_dict(), True), _loader(TS.loader_dataset_dict(data_s=True), False)
    rows = TS.loader_dataset_dict()["train_ulb"]["data"]
    assert len(rows) == 24 and (min(map(len, rows)), max(map(len, rows))) == (2, 64) and ld.batch_size == 8 and ld.mask_id == 103
    lengths, changed = set(), 0
    for epoch in (0, 1):
        ld.set_epoch(epoch), plain.set_epoch(epoch)
        copies.clear()
        got, weak = list(ld), list(plain)
        assert len(got) == 3 and copies == [(5, 24), (3, 24)]                    # one host-to-device copy per loader and epoch
        for t, (b, w) in enumerate(zip(got, weak)):
            assert list(b) == list(ULB_KEYS) and torch.equal(b["idx_ulb"], w["idx_ulb"])
            assert torch.equal(b["x_ulb_w"].ids, w["x_ulb_w"].ids) and torch.equal(b["x_ulb_w"].key_len, w["x_ulb_w"].key_len)      # the weak views of a loader without the key
            ids = _equals_restatement(b["x_ulb_s"], ld, t, rows, 103)
            lengths.add(ids.shape[1])
            changed += int((b["x_ulb_s"].key_len != b["x_ulb_w"].key_len).sum())
        again = list(ld)                                                          # iterating again replays the epoch
        assert all(torch.equal(x["x_ulb_s"].ids, y["x_ulb_s"].ids) and torch.equal(x["x_ulb_s"].key_len, y["x_ulb_s"].key_len) for x, y in zip(got, again))
    assert len(lengths) > 1 and changed > 8                                       # deletions: the strong view meets more lengths


# ---- train() through the loaders -----------------------------------------------------------------------------------------------------------------
def _args(dd, **kw):
    c = TS.LOADER
    d = dict(num_classes=c["num_classes"], num_train_iter=3, epoch=1, ema_m=0.0, ulb_loss_ratio=1.0, use_cat=False, amp=False,
             optim="AdamW", lr=5e-4, weight_decay=5e-4, layer_decay=0.75, num_warmup_iter=0, T=0.5, hard_label=True, p_cutoff=0.95, N_k=2, start_timing=2,
             feature_dim=128, sr_lr=5e-4, sr_ema=False, sr_ema_m=0.99, num_eval_iter=0, num_log_iter=2, gpu=0, rank=0, world_size=1, distributed=False,
             dataset="aclImdb", max_length=c["max_length"], batch_size=c["batch_size"], uratio=c["uratio"], eval_batch_size=c["eval_batch_size"],
             train_sampler="RandomSampler", seed=c["seed"], device_tokens=True, dataset_dict=dd)
    d.update(kw)
    return argparse.Namespace(**d)


ALGS = {"srflexmatch": dict(algorithm="srflexmatch", thresh_warmup=True),
        "srsoftmatch": dict(algorithm="srsoftmatch", dist_align=True, dist_uniform=True, per_class=False, ema_p=0.9, n_sigma=2)}


@pytest.mark.parametrize("name", sorted(ALGS))
def test_train_with_the_key_and_no_data_s(name):
    rows = TS.loader_dataset_dict()["train_ulb"]["data"]
    with pytest.raises(ValueError, match="this algorithm's train_step takes x_ulb_s but the unlabelled set has no data_s"):     # without the key: today's refusal
        get_algorithm(_args(TS.loader_dataset_dict(), **ALGS[name]), bert.bert_tiny_test)
    lines = []
    args = _args(TS.loader_dataset_dict(), device_tokens_strong=True, device_tokens_mask_id=4, **ALGS[name])
    alg = get_algorithm(args, bert.bert_tiny_test, logger=argparse.Namespace(info=lines.append, warning=lines.append))
    ulb = alg.loader_dict["train_ulb"]
    assert ulb.makes_strong and ulb.keys == ULB_KEYS and alg.dataset_dict["train_ulb"].n_variants == 0 and (ulb.mask_id, ulb.rate) == (4, 0.3)
    received, losses, step = [], [], alg.train_step

    @functools.wraps(step)
    def recording(**kw):
        t = len(received)
        received.append(_equals_restatement(kw["x_ulb_s"], ulb, t, rows, 4))      # checked while the epoch's draws are the loader's
        out, log = step(**kw)
        losses.append(log["train/total_loss"])
        return out, log
    alg.train_step = recording
    alg.train()
    torch.cuda.synchronize()
    assert alg.it == 3 and len(received) == 3 and all(np.isfinite(float(v)) for v in losses)
    assert any((ids == 4).any() for ids in received)                              # the configured mask id reached a batch
    ops.check_label_errors()


# ---- the example ------------------------------------------------------------------------------------------------------------------------------------
def test_train_device_tokens_example_runs_with_device_strong(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_device_tokens as ex
    monkeypatch.setattr(sys, "argv", ["train_device_tokens.py", "--steps", "8", "--device-strong"])
    ev = ex.main()
    assert {"eval/loss", "eval/top-1-acc"} <= set(ev) and all(np.isfinite(float(v)) for v in ev.values())
