"""device_tokens on the MI355X: srhip_token_view against the numpy oracle of tests/_token_view_cases.py at every length, pitch and geometry
the kernel branches on, on sentinel-guarded buffers; the token loaders against the reference collator's recorded batches
(tests/golden/device_tokens.npz); ``alg.evaluate()`` / ``alg.train()`` fed by the loaders on the tiny BERT.  Integer results: every
comparison is exact, there is no tolerance."""
import argparse
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _token_view_cases as TC                                         # noqa: E402
from semireward_amd import ops                                         # noqa: E402
from semireward_amd.algorithms import get_algorithm                    # noqa: E402
from semireward_amd.data import device_tokens as DT                    # noqa: E402
from semireward_amd.nets import bert                                   # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kernel_store():
    rows = TC.kernel_rows()
    ds = DT.DeviceTokenDataset(rows, None, DEV)
    assert ds.store.numel() == ds.row_off_host[-1] + ds.row_len_host[-1]        # the last row ends on the store's last int
    assert ds.store.data_ptr() % 16 == 0
    return rows, ds


@pytest.mark.parametrize("L", TC.KERNEL_L)
def test_token_view_against_the_oracle_b24(kernel_store, L):
    rows, ds = kernel_store
    cases = [c for c in TC.kernel_cases() if c["name"].startswith("b24_L%d_" % L)]
    assert len(cases) == 3
    for c in cases:
        ids, kl, guards_intact = TC.launch(ds, c["src_row"], c["L"], c["ld_ids"], c["pad_id"])
        want, want_kl = TC.token_view_oracle(rows, c["src_row"], c["L"], c["pad_id"])
        assert np.array_equal(ids, want) and np.array_equal(kl, want_kl) and kl.dtype == np.int32, c["name"]
        assert guards_intact, c["name"]                                         # guard rows, guard columns L .. ld_ids, key_len's neighbours
        assert kl.max() == min(L, 600) and (L < 600) == bool((kl == L).sum() > 1)


def test_token_view_single_rows_and_rows_outside_the_store(kernel_store):
    rows, ds = kernel_store
    cases = [c for c in TC.kernel_cases() if c["name"].startswith("b1_")]
    assert len(cases) == 8
    for c in cases:
        ids, kl, guards_intact = TC.launch(ds, c["src_row"], c["L"], c["ld_ids"], c["pad_id"])
        want, want_kl = TC.token_view_oracle(rows, c["src_row"], c["L"], c["pad_id"])
        assert np.array_equal(ids, want) and np.array_equal(kl, want_kl) and guards_intact, c["name"]
    # a src_row outside [0, n_rows): an all-pad row of length 0, through the raw entry only (the wrapper's host check refuses it)
    n = len(rows)
    src = np.array([0, -1, n, 5, 1 << 40, -(1 << 40)], dtype=np.int64)
    for L, ld in ((9, 9), (8, 10)):
        ids, kl, guards_intact = TC.launch(ds, src, L, ld, 77)
        want, want_kl = TC.token_view_oracle(rows, src, L, 77)
        assert np.array_equal(ids, want) and kl.tolist() == want_kl.tolist() == [5, 0, 0, 7, 0, 0] and guards_intact
        assert (ids[[1, 2, 4, 5]] == 77).all()
    # n_rows smaller than the store: the rows past it count as outside
    ids, kl, guards_intact = TC.launch(ds, np.array([2, 3], dtype=np.int64), 4, 4, 0, n_rows=3)
    assert kl.tolist() == [2, 0] and not ids[1].any() and np.array_equal(ids[0, :2], rows[2]) and guards_intact


def test_token_view_reads_rows_that_start_off_a_16_byte_boundary(kernel_store):
    """The store's contract puts every row on a multiple of 4 ints; a row placed elsewhere takes the kernel's single-load path and must give
    the same result: the rows packed tightly (row_off % 4 = 1, 2, 3, 0 all occur), every L, even and odd pitch."""
    rows, ds = kernel_store
    off = np.concatenate([[0], np.cumsum(TC.ROW_LENS)[:-1]]).astype(np.int64)
    assert set((off % 4).tolist()) == {0, 1, 2, 3}
    tight = argparse.Namespace(store=torch.from_numpy(np.concatenate(rows)).to(DEV), row_off=torch.from_numpy(off).to(DEV), row_len=ds.row_len,
                               row_len_host=ds.row_len_host)
    assert tight.store.numel() == sum(TC.ROW_LENS) and tight.store.data_ptr() % 16 == 0
    src = TC.kernel_cases()[0]["src_row"]
    for L in TC.KERNEL_L:
        for ld, pad in ((L, 0), (L + 1, 103)):
            ids, kl, guards_intact = TC.launch(tight, src, L, ld, pad)
            want, want_kl = TC.token_view_oracle(rows, src, L, pad)
            assert np.array_equal(ids, want) and np.array_equal(kl, want_kl) and guards_intact, (L, ld)


def test_token_view_wrapper_and_entry_refusals(kernel_store):
    rows, ds = kernel_store
    src = torch.tensor([7, 0, 11, 7], dtype=torch.int64, device=DEV)
    for L in (9, 12):
        ids, kl = ops.token_view(ds.store, ds.row_off, ds.row_len, src, L, pad_id=5, host=(src.cpu().numpy(), ds.row_len_host))
        want, want_kl = TC.token_view_oracle(rows, src.cpu().numpy(), L, 5)
        assert ids.is_contiguous() and ids.dtype == torch.int64 and kl.dtype == torch.int32
        assert np.array_equal(ids.cpu().numpy(), want) and np.array_equal(kl.cpu().numpy(), want_kl)
    out, kl = torch.zeros(2, 16, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)

    def call(**kw):
        a = dict(store=ds.store.data_ptr(), off=ds.row_off.data_ptr(), ln=ds.row_len.data_ptr(), n=len(rows), r=src.data_ptr(), B=2, L=10, pad=0,
                 ids=out.data_ptr(), ld=16, kl=kl.data_ptr(), stream=ops._s())
        a.update(kw)
        ops._call("srhip_token_view", *a.values())
    call()
    torch.cuda.synchronize()
    for kw in (dict(store=None), dict(off=None), dict(ln=None), dict(r=None), dict(ids=None), dict(kl=None), dict(n=0), dict(B=0), dict(B=65536),
               dict(L=0), dict(L=17), dict(ld=9), dict(store=ds.store.data_ptr() + 4), dict(store=ds.store.data_ptr() + 8), dict(ids=out.data_ptr() + 4)):
        with pytest.raises(RuntimeError, match="invalid argument"):
            call(**kw)
    launched = []
    real = ops._call
    try:
        ops._call = lambda *a: launched.append(a)
        with pytest.raises(IndexError, match="src_row outside the store's 12 rows"):       # the wrapper refuses what the kernel would pad
            ops.token_view(ds.store, ds.row_off, ds.row_len, src, 10, host=(np.array([7, 0, 12, 7]), ds.row_len_host))
    finally:
        ops._call = real
    assert not launched                                                                     # ... before launching


# ---- the loaders ---------------------------------------------------------------------------------------------------------------------------------
def _equals_collator(batch, g, prefix, s=""):
    """as_dict() equals the recorded collator output; ids / key_len equal TokenBatch.from_dict(collator dict) exactly."""
    ids, mask = g[prefix + s + "input_ids"], g[prefix + s + "attention_mask"]
    d = batch.as_dict()
    assert d["input_ids"].is_cuda and d["input_ids"].dtype == d["attention_mask"].dtype == torch.int64
    assert np.array_equal(d["input_ids"].cpu().numpy(), ids) and np.array_equal(d["attention_mask"].cpu().numpy(), mask)
    ref = bert.TokenBatch.from_dict({"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(mask)}, DEV)
    assert torch.equal(batch.ids, ref.ids) and torch.equal(batch.key_len, ref.key_len) and batch.key_len.dtype == ref.key_len.dtype
    assert (batch.S, batch.L) == (ref.S, ref.L) and batch.ids.is_contiguous() and batch.seq_len is None


def test_loader_batches_equal_the_collators_recorded_output(golden):
    g, c = golden("device_tokens"), TC.LOADER
    dd = TC.loader_dataset_dict(g)
    ld_l, ld_u = TC.loader_pair(dd, DEV)
    for epoch in range(c["epoch"]):
        ld_l.set_epoch(epoch), ld_u.set_epoch(epoch)
        steps = list(zip(ld_l, ld_u))
        assert len(steps) == 2
        for t, (bl, bu) in enumerate(steps):
            pl, pu = "col/e%d/lb/%d/" % (epoch, t), "col/e%d/ulb/%d/" % (epoch, t)
            assert all(v.is_cuda for k, v in {**bl, **bu}.items() if not k.startswith("x"))
            assert np.array_equal(bl["idx_lb"].cpu().numpy(), g[pl + "idx"]) and np.array_equal(bl["y_lb"].cpu().numpy(), g[pl + "y_lb"])
            assert np.array_equal(bu["idx_ulb"].cpu().numpy(), g[pu + "idx"])
            _equals_collator(bl["x_lb"], g, pl)
            _equals_collator(bu["x_ulb_w"], g, pu)
            BU = ld_u.batch_size
            assert np.array_equal(ld_u.draws["x_ulb_s"][0][BU * t:BU * t + BU] // len(ld_u.dataset) - 1, g[pu + "variant"])
            _equals_collator(bu["x_ulb_s"], g, pu, "s_")                          # the collator on the variants the loader drew
    ev = DT.TokenEvalLoader(DT.DeviceTokenDataset.from_reference(dd["eval"], DEV), c["eval_batch_size"])
    got = list(ev)
    assert len(got) == 3
    for t, b in enumerate(got):
        _equals_collator(b["x_lb"], g, "col/eval/%d/" % t)
        assert np.array_equal(b["y_lb"].cpu().numpy(), g["col/eval/%d/y_lb" % t])


# ---- evaluate() and train() through the loaders ----------------------------------------------------------------------------------------------------
def _args(dd, **kw):
    c = TC.LOADER
    d = dict(num_classes=c["num_classes"], num_train_iter=c["num_train_iter"], epoch=c["epoch"], ema_m=0.0, ulb_loss_ratio=1.0, use_cat=False, amp=False,
             optim="AdamW", lr=5e-4, weight_decay=5e-4, layer_decay=0.75, num_warmup_iter=0, T=0.5, hard_label=True, p_cutoff=0.95, N_k=2, start_timing=2,
             feature_dim=128, sr_lr=5e-4, sr_ema=False, sr_ema_m=0.99, num_eval_iter=0, num_log_iter=2, gpu=0, rank=0, world_size=1, distributed=False,
             dataset="aclImdb", max_length=c["max_length"], batch_size=c["batch_size"], uratio=c["uratio"], eval_batch_size=c["eval_batch_size"],
             train_sampler="RandomSampler", seed=c["seed"], device_tokens=True, dataset_dict=dd)
    d.update(kw)
    return argparse.Namespace(**d)


ALGS = {"srpseudolabel": dict(algorithm="srpseudolabel", unsup_warm_up=0.4),
        "srsoftmatch": dict(algorithm="srsoftmatch", dist_align=True, dist_uniform=True, per_class=False, ema_p=0.9, n_sigma=2)}


def test_evaluate_through_the_token_eval_loader_equals_host_dict_batches(golden):
    g = golden("device_tokens")
    alg = get_algorithm(_args(TC.loader_dataset_dict(g), **ALGS["srpseudolabel"]), bert.bert_tiny_test)
    alg.model.view("classifier.2.weight").mul_(8.0)                               # spread the logits (a random-init head is flat)
    alg.model.refresh_operands()
    loader = alg.loader_dict["eval"]
    assert isinstance(loader, DT.TokenEvalLoader)
    host = [{"x_lb": {k: v.cpu() for k, v in b["x_lb"].as_dict().items()}, "y_lb": b["y_lb"].cpu()} for b in loader]
    assert [tuple(b["x_lb"]["input_ids"].shape) for b in host] == [g["col/eval/%d/input_ids" % t].shape for t in range(3)]
    assert np.array_equal(torch.cat([b["y_lb"] for b in host]).numpy(), TC.targets("eval"))
    for device_eval in (False, True):
        alg.device_eval = device_eval
        h1, h2 = (alg.evaluate("eval", loader=host, return_logits=True) for _ in range(2))
        repeatable = h1["eval/loss"] == h2["eval/loss"] and np.array_equal(h1["eval/logits"], h2["eval/logits"])
        ev = alg.evaluate("eval", return_logits=True)
        print("\ndevice_eval %s: host-dict path repeats bit for bit: %s; eval/loss loader %r host dicts %r"
              % (device_eval, repeatable, ev["eval/loss"], h1["eval/loss"]))
        assert set(ev) == set(h1) and np.isfinite(ev["eval/loss"]) and {"eval/top-1-acc", "eval/F1"} <= set(ev)
        assert np.array_equal(ev["eval/logits"].argmax(-1), h1["eval/logits"].argmax(-1))                        # equal predictions
        assert all(ev[k] == h1[k] for k in ev if k not in ("eval/loss", "eval/logits"))                           # equal metrics
        assert repeatable, "two runs of the host-dict path differ: a finding about existing code, see the printed line"
        assert ev["eval/loss"] == h1["eval/loss"] and np.array_equal(ev["eval/logits"], h1["eval/logits"])        # bit for bit
    ops.check_label_errors()


@pytest.mark.parametrize("name", sorted(ALGS))
def test_train_through_the_token_loaders_with_run_hooks(golden, tmp_path, name):
    g, c = golden("device_tokens"), TC.LOADER
    dd = TC.loader_dataset_dict(g)
    strong = name == "srsoftmatch"
    if not strong:
        del dd["train_ulb"]["data_s"]                                            # SRPseudoLabel takes no strong view, hence needs no variants
    lines = []
    args = _args(dd, run_hooks=True, device_eval=True, num_eval_iter=2, num_log_iter=2, save_dir=str(tmp_path), save_name="run", **ALGS[name])
    alg = get_algorithm(args, bert.bert_tiny_test, logger=argparse.Namespace(info=lines.append, warning=lines.append))
    assert args.ulb_dest_len == TC.SPLITS["train_ulb"][0] and "DistSamplerSeedHook" in alg.hooks_dict and "EvaluationHook" in alg.hooks_dict
    assert alg.loader_dict["train_ulb"].keys == (("idx_ulb", "x_ulb_w", "x_ulb_s") if strong else ("idx_ulb", "x_ulb_w"))
    yielded, received, losses, step = {"train_lb": [], "train_ulb": []}, [], [], alg.train_step

    class Recording:                                                             # the loader, every batch it yields kept
        def __init__(self, ld, log):
            self.ld, self.log = ld, log

        def set_epoch(self, epoch):
            self.ld.set_epoch(epoch)

        def __iter__(self):
            for b in self.ld:
                self.log.append(b)
                yield b
    for k in yielded:
        alg.loader_dict[k] = Recording(alg.loader_dict[k], yielded[k])

    @functools.wraps(step)
    def recording(**kw):
        received.append(kw)
        out, log = step(**kw)
        losses.append(log["train/total_loss"])
        return out, log
    alg.train_step = recording
    alg.train()                                                                   # no batches= argument: the loaders feed the loop, across the epoch boundary
    torch.cuda.synchronize()
    assert alg.it == c["num_train_iter"] == 4 and alg.epoch == 1 and len(received) == 4
    for t, kw in enumerate(received):                                             # what the step received is what the loaders yielded: the same objects
        bl, bu = yielded["train_lb"][t], yielded["train_ulb"][t]
        views = ("x_lb", "x_ulb_w") + (("x_ulb_s",) if strong else ())
        assert set(kw) == set(views) | {"y_lb"}                                   # train_step's parameters, nothing else
        assert all(isinstance(kw[k], bert.TokenBatch) and kw[k] is {**bl, **bu}[k] and kw[k].ids.is_cuda for k in views)
        assert kw["y_lb"] is bl["y_lb"]
        e, s = divmod(t, 2)
        for k, p, sfx in (("x_lb", "lb", ""), ("x_ulb_w", "ulb", "")) + ((("x_ulb_s", "ulb", "s_"),) if strong else ()):
            assert np.array_equal(kw[k].ids.cpu().numpy(), g["col/e%d/%s/%d/%sinput_ids" % (e, p, s, sfx)])
    assert all(np.isfinite(float(v)) for v in losses)
    assert (tmp_path / "run" / "latest_model.pth").exists()
    ops.check_label_errors()


# ---- the example ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [["--steps", "8"], ["--steps", "8", "--algorithm", "srpseudolabel"], ["--steps", "12", "--run-hooks"]],
                         ids=["srsoftmatch", "srpseudolabel", "run_hooks"])
def test_train_device_tokens_example_runs(monkeypatch, argv):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_device_tokens as ex
    monkeypatch.setattr(sys, "argv", ["train_device_tokens.py"] + argv)
    ev = ex.main()
    assert {"eval/loss", "eval/top-1-acc"} <= set(ev) and all(np.isfinite(float(v)) for v in ev.values())
