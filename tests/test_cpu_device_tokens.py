"""device_tokens (semireward_amd/data/device_tokens.py, csrc/token_view.hip) without a GPU: the C ABI entry, its wrapper and its argument
refusals; the store's packing against the recorded token ids (tests/golden/device_tokens.npz, written by tools/device_tokens_golden.py); the
loaders' bookkeeping with the launch stubbed by the numpy oracle, element for element against what the reference's collator returned for the
same index stream; tokenising the fixture strings through the tiny vocabulary directory; the option's wiring into AlgorithmBase (refusals;
nothing changes without it); the kernel's registers."""
import argparse
import builtins
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import _token_view_cases as TC
from semireward_amd import _lib, ops
from semireward_amd.core.algorithmbase import AlgorithmBase
from semireward_amd.core.hooks import DistSamplerSeedHook, EMAHook, ParamUpdateHook, TimerHook
from semireward_amd.data import device_tokens as DT
from semireward_amd.data.device_loader import EpochSampler
from semireward_amd.nets import bert, vit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_signature_and_wrapper_agree(monkeypatch):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srhip.h")).read(), flags=re.S)
    decl = re.search(r"int\s+srhip_token_view\s*\(([^)]*)\)", src).group(1)
    res, argtypes = _lib.SIGNATURES["srhip_token_view"]
    assert res is _lib.I and len(argtypes) == len(decl.split(",")) == 12
    assert [_lib.P if "*" in a else _lib.I for a in decl.split(",")] == argtypes          # pointer / int, position by position
    sent = []
    monkeypatch.setattr(ops, "_call", lambda name, *a: sent.append((name, a)))
    monkeypatch.setattr(ops, "_p", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(ops, "_s", lambda: None)
    store, off, ln = torch.zeros(16, dtype=torch.int32), torch.tensor([0, 8]), torch.tensor([5, 8], dtype=torch.int32)
    ids, kl = ops.token_view(store, off, ln, torch.tensor([1, 0, 1]), 7, pad_id=9, host=(np.array([1, 0, 1]), np.array([5, 8])))
    (name, a), = sent
    assert name == "srhip_token_view" and len(a) == len(argtypes)
    assert a[3] == 2 and a[5:8] == (3, 7, 9) and a[9] == 7                                   # n_rows, B, L, pad_id, ld_ids
    assert ids.shape == (3, 7) and ids.dtype == torch.int64 and ids.is_contiguous() and kl.shape == (3,) and kl.dtype == torch.int32
    ops.token_view(store, off, ln, torch.tensor([0]), 4)
    assert sent[1][1][7] == 0                                                                # pad_id defaults to [PAD] = 0
    for bad in (np.array([2]), np.array([-1]), np.array([0, 1, 2])):
        with pytest.raises(IndexError, match="src_row outside the store's 2 rows"):         # refused on the host, before the launch
            ops.token_view(store, off, ln, torch.tensor([0]), 4, host=(bad, np.array([5, 8])))
    assert len(sent) == 2
    with pytest.raises(ValueError, match="1-D integer"):
        ops.check_token_rows(np.array([0.5]), np.array([5, 8]))
    with pytest.raises(ValueError, match="int64"):
        ops.token_view(store, off, ln, torch.tensor([0], dtype=torch.int32), 4)
    with pytest.raises(ValueError, match="int32 with int64 row_off"):
        ops.token_view(store.long(), off, ln, torch.tensor([0]), 4)
    with pytest.raises(ValueError, match="one entry per row"):
        ops.token_view(store, off, ln[:1], torch.tensor([0]), 4)


def test_entry_refuses_each_bad_argument():
    f = _lib.lib().srhip_token_view
    buf = (ctypes.c_int * 64)()
    a = (ctypes.addressof(buf) + 15) & ~15                                       # a 16-byte aligned host address: never dereferenced, every call is refused first
    ok = dict(store=a, row_off=a, row_len=a, n_rows=2, src_row=a, B=2, L=6, pad_id=0, ids=a, ld_ids=7, key_len=a, stream=None)

    def rc(**kw):
        return f(*{**ok, **kw}.values())
    for k in ("store", "row_off", "row_len", "src_row", "ids", "key_len"):
        assert rc(**{k: None}) == -1, k                                          # SR_EINVAL
    for kw in (dict(n_rows=0), dict(n_rows=-1), dict(B=0), dict(B=-3), dict(B=65536), dict(L=0), dict(L=-1), dict(L=8), dict(ld_ids=5),
               dict(store=a + 4), dict(store=a + 8), dict(ids=a + 4)):
        assert rc(**kw) == -1, kw


# ---- 2. the fixture ---------------------------------------------------------------------------------------------------------------------------
def test_fixture_is_arrays_only_small_and_holds_the_edge_sentences(golden):
    g = golden("device_tokens")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "device_tokens.npz")) < 100 * 1024
    assert all(g[k].dtype.kind in "iuU" for k in g.keys())
    for ml in TC.MAX_LENGTHS:
        for split, (n, _) in TC.SPLITS.items():
            rows, var = TC.fixture_rows(g, split, ml)
            assert len(rows) == n and (var is None) == (split == "eval")
            every = rows + (var[0] + var[1] if var else [])
            assert all(2 <= len(r) <= ml and r[0] == TC.CLS and r[-1] == TC.SEP and 0 < r.min() and r.max() < len(TC.VOCAB) for r in every)
        rows, _ = TC.fixture_rows(g, "train_ulb", ml)
        assert len(rows[0]) == ml                                                 # tokenises longer than max_length: truncated, [SEP] kept last
        assert rows[1].tolist() == [TC.CLS, TC.SEP]                               # the empty string
        pieces = [TC.VOCAB.index(w) for w in ("watch", "##ing", "cat", "##s")]
        assert rows[2].tolist() == [TC.CLS] + pieces + [TC.SEP]                   # "watching cats"
        assert rows[3].tolist()[1:3] == [TC.VOCAB.index("the"), TC.UNK]          # "the zebra ...": outside the vocabulary


def test_tokenising_the_fixture_strings_gives_the_recorded_ids(golden, tmp_path):
    pytest.importorskip("transformers")
    g = golden("device_tokens")
    tok = DT.load_tokenizer(TC.write_vocab_dir(str(tmp_path / "vocab")))
    assert tok.vocab_size == len(TC.VOCAB) and tok.pad_token_id == TC.PAD == DT.DeviceTokenDataset.pad_id
    for ml in TC.MAX_LENGTHS:
        tri = TC.sentences("train_ulb")
        ds = DT.DeviceTokenDataset([t[0] for t in tri], None, "cpu", data_s=[[t[1] for t in tri], [t[2] for t in tri]], max_length=ml,
                                   tokenize=DT.make_tokenize(tok, ml))
        rows, var = TC.fixture_rows(g, "train_ulb", ml)
        assert all(np.array_equal(a, b) for a, b in zip(TC.store_rows(ds), rows + var[0] + var[1])) and len(ds.row_len_host) == 3 * len(rows)

    class Ref:                                                                    # duck-typed reference BasicDataset: triples of strings
        data, targets, is_ulb = TC.sentences("eval"), TC.targets("eval"), False
    ev = DT.DeviceTokenDataset.from_reference(Ref, "cpu", DT.make_tokenize(tok, 16), 16)
    assert ev.n_variants == 0 and len(ev.row_len_host) == len(Ref.data)           # the literal 'None' augmentations are not stored
    assert all(np.array_equal(a, b) for a, b in zip(TC.store_rows(ev), TC.fixture_rows(g, "eval", 16)[0]))
    Ref.data, Ref.is_ulb = np.array(TC.sentences("train_ulb")), True              # the [n, 3] string array split_ssl_data leaves in a training set
    ul = DT.DeviceTokenDataset.from_reference(Ref, "cpu", DT.make_tokenize(tok, 16), 16)
    assert ul.n_variants == 2 and ul.targets is None and np.array_equal(ul.row_len_host, g["tok/16/train_ulb/len"])


def _recorded_tokenize(g, max_length=16):
    """str -> the recorded ids of that fixture sentence: a tokenizer for tests that must not need transformers."""
    table = {}
    for split in TC.SPLITS:
        tri = TC.sentences(split)
        texts = [t[0] for t in tri] + ([t[1] for t in tri] + [t[2] for t in tri] if split != "eval" else [])
        rows, var = TC.fixture_rows(g, split, max_length)
        for s, r in zip(texts, rows + (var[0] + var[1] if var else [])):
            assert table.setdefault(s, r.tolist()) == r.tolist()
    return lambda text: (type(text) is str or pytest.fail("the tokenizer must get a plain str, got %r" % type(text))) and table[text]


def test_training_sets_as_split_ssl_data_leaves_them(golden, monkeypatch):
    """The reference's get_json_dset sends the training triples through split_ssl_data: ``np.array(data)[idx]`` (semilearn/datasets/utils.py:38-52),
    so BasicDataset.data of train_lb / train_ulb is an [n, 3] string array; only eval / test stay lists of tuples."""
    g = golden("device_tokens")
    tok = _recorded_tokenize(g)
    refs, want = {}, {}
    for split, ulb in (("train_lb", False), ("train_ulb", True)):
        tri, y = TC.sentences(split), TC.targets(split if not ulb else "train_lb")
        idx = np.random.Generator(np.random.PCG64(3)).permutation(len(tri))[:len(tri) - 2]
        arr = np.array(tri)[idx]
        assert arr.shape == (len(idx), 3) and arr.dtype.kind == "U" and DT._holds_strings(argparse.Namespace(data=arr))
        assert DT._triples(arr) == ([tri[i][0] for i in idx], [[tri[i][1] for i in idx], [tri[i][2] for i in idx]])
        refs[split] = argparse.Namespace(data=arr, targets=np.resize(y, len(tri))[idx], is_ulb=ulb)
        rows, var = TC.fixture_rows(g, split, 16)
        want[split] = [rows[i] for i in idx] + [var[0][i] for i in idx] + [var[1][i] for i in idx]
        ds = DT.DeviceTokenDataset.from_reference(refs[split], "cpu", tok, 16)
        assert ds.n_variants == 2 and len(ds) == len(idx) and (ds.targets is None) == ulb
        assert all(np.array_equal(a, b) for a, b in zip(TC.store_rows(ds), want[split])) and len(ds.row_len_host) == 3 * len(idx)
    # ... and through the wiring: only the training sets hold strings, the tokenizer is still resolved (once) and the stores hold the recorded ids
    resolved = []
    monkeypatch.setattr(DT, "resolve_tokenizer", lambda args: (resolved.append(args.net), lambda text, **kw: (
        kw == dict(max_length=16, truncation=True, padding=False) or pytest.fail(str(kw))) and {"input_ids": tok(text)})[1])
    refs["eval"] = {"data": TC.fixture_rows(g, "eval", 16)[0], "targets": TC.targets("eval")}
    dd = DT.build_token_datasets(_args(net="bert_base_uncased"), refs, "cpu")
    assert resolved == ["bert_base_uncased"]
    for split in ("train_lb", "train_ulb"):
        assert all(np.array_equal(a, b) for a, b in zip(TC.store_rows(dd[split]), want[split]))
    assert dd["train_lb"].targets_host.tolist() == refs["train_lb"].targets.tolist()
    # rows that are 1-D arrays of 3 strings (a list of such rows), and what is NOT a triple
    assert DT._triples(list(np.array(TC.sentences("eval")))) == ([t[0] for t in TC.sentences("eval")], [["None"] * 7] * 2)
    assert DT._triples([np.arange(3), np.arange(3)]) is None and DT._triples(["a b c", "d e f"]) is None and DT._triples([]) is None
    assert not DT._holds_strings({"data": [np.arange(3)], "data_s": [[np.arange(3)]]}) and DT._holds_strings({"data": [np.arange(3)], "data_s": [["a"]]})


# ---- 3. packing ---------------------------------------------------------------------------------------------------------------------------------
def test_store_packing_and_refusals(golden):
    g = golden("device_tokens")
    rows, var = TC.fixture_rows(g, "train_ulb", 16)
    ds = DT.DeviceTokenDataset(rows, None, "cpu", data_s=var, max_length=16)
    n = len(rows)
    assert len(ds) == n and ds.n_variants == 2 and ds.store.dtype == torch.int32 and ds.row_off.dtype == torch.int64 and ds.row_len.dtype == torch.int32
    assert np.array_equal(ds.row_len_host, g["tok/16/train_ulb/len"]) and (ds.row_off_host % 4 == 0).all() and ds.targets is None
    assert ds.row_off_host.tolist() == np.concatenate([[0], np.cumsum((ds.row_len_host + 3) // 4 * 4)[:-1]]).tolist()
    assert np.array_equal(ds.row_off.numpy(), ds.row_off_host) and np.array_equal(ds.row_len.numpy(), ds.row_len_host)
    flat = ds.store.numpy()
    assert flat.size == int(((ds.row_len_host + 3) // 4 * 4).sum())
    for r, c in enumerate(rows + var[0] + var[1]):                                # variants sit in their own rows, after the sentences
        o = ds.row_off_host[r]
        assert np.array_equal(flat[o:o + c.size], c) and not flat[o + c.size:o + (c.size + 3) // 4 * 4].any()
    assert ds.strong_row([0, 1, 1], [2, 0, 3]).tolist() == [n + 2, 2 * n + 0, 2 * n + 3]
    assert ds.max_id_host == int(g["tok/16/train_ulb/flat"].max()) and ds.max_length == 16
    lb = DT.DeviceTokenDataset.from_reference({"data": rows[:4], "targets": torch.tensor([3, 1, 0, 2])}, "cpu")
    assert lb.targets.tolist() == lb.targets_host.tolist() == [3, 1, 0, 2] and lb.targets.dtype == torch.int64 and lb.n_variants == 0
    assert DT.DeviceTokenDataset.from_reference(ds, "cpu") is ds
    assert DT.DeviceTokenDataset([[5, 6, 7], torch.tensor([2, 3])], None, "cpu").row_len_host.tolist() == [3, 2]      # lists and tensors of ints
    with pytest.raises(ValueError, match="row 1 of data holds 5 tokens, more than max_length = 4; the store does not truncate silently"):
        DT.DeviceTokenDataset([np.arange(1, 5), np.arange(1, 6)], None, "cpu", max_length=4)
    with pytest.raises(ValueError, match="row 1 of data is empty"):
        DT.DeviceTokenDataset([rows[0], np.zeros(0, dtype=np.int64)], None, "cpu")
    with pytest.raises(ValueError, match="negative token id"):
        DT.DeviceTokenDataset([np.array([2, -1, 3])], None, "cpu")
    with pytest.raises(ValueError, match="integer arrays, got dtype float32 for row 0 of data"):
        DT.DeviceTokenDataset([np.ones(3, dtype=np.float32)], None, "cpu")
    with pytest.raises(ValueError, match="1-D token rows"):
        DT.DeviceTokenDataset([np.ones((2, 3), dtype=np.int64)], None, "cpu")
    with pytest.raises(ValueError, match="is a string and no tokenizer was given"):
        DT.DeviceTokenDataset(["a film"], None, "cpu")
    with pytest.raises(ValueError, match="one label per sentence"):
        DT.DeviceTokenDataset(rows, [0, 1], "cpu")
    with pytest.raises(ValueError, match=r"data_s\[1\] must hold one variant of every sentence"):
        DT.DeviceTokenDataset(rows, None, "cpu", data_s=[var[0], var[1][:3]])
    with pytest.raises(ValueError, match="holds no sentence"):
        DT.DeviceTokenDataset([], None, "cpu")


def test_pretokenised_rows_never_import_transformers(golden, monkeypatch):
    real = builtins.__import__

    def guarded(name, *a, **k):
        assert not name.startswith("transformers"), "transformers imported for already-tokenised rows"
        return real(name, *a, **k)
    for m in [m for m in sys.modules if m.startswith("transformers")]:
        monkeypatch.delitem(sys.modules, m)
    monkeypatch.setattr(builtins, "__import__", guarded)
    dd = DT.build_token_datasets(_args(), TC.loader_dataset_dict(golden("device_tokens")), "cpu")
    assert all(isinstance(v, DT.DeviceTokenDataset) for v in dd.values())


def test_tokenizer_is_resolved_offline_and_every_failure_names_its_paths(tmp_path, monkeypatch):
    monkeypatch.setenv("HF_HUB_CACHE", str(tmp_path / "no-hub-cache"))
    dd = {"train_lb": {"data": ["a film"], "targets": [0]}}
    with pytest.raises(RuntimeError, match="no snapshot directory with a tokenizer was found for net 'bert_base_uncased'.*no-hub-cache"):
        DT.build_token_datasets(_args(net="bert_base_uncased"), dd, "cpu")
    snap = tmp_path / "snap"
    snap.mkdir()
    (snap / "config.json").write_text("{}")
    (snap / "model.safetensors").write_bytes(b"")
    with pytest.raises(RuntimeError, match="holds no tokenizer files .*tried: .*snap"):
        DT.build_token_datasets(_args(net="bert_base_uncased", pretrain_path=str(snap)), dd, "cpu")
    TC.write_vocab_dir(str(snap))
    real = builtins.__import__

    def missing(name, *a, **k):
        if name.startswith("transformers"):
            raise ImportError("No module named 'transformers'")
        return real(name, *a, **k)
    with monkeypatch.context() as m:
        for mod in [x for x in sys.modules if x.startswith("transformers")]:
            m.delitem(sys.modules, mod)
        m.setattr(builtins, "__import__", missing)
        with pytest.raises(RuntimeError, match="transformers is not importable.*tried: .*snap"):
            DT.build_token_datasets(_args(net="bert_base_uncased", pretrain_path=str(snap)), dd, "cpu")


# ---- 4. loaders, the launch stubbed by the oracle -----------------------------------------------------------------------------------------------
@pytest.fixture
def stub(monkeypatch):
    """ops.token_view replaced by the numpy oracle on host tensors; every call and every host-to-device copy is recorded."""
    calls, copies = [], []

    def token_view(store, row_off, row_len, src_row, L, pad_id=0, host=None):
        flat = store.numpy()
        rows = [flat[o:o + n] for o, n in zip(row_off.tolist(), row_len.tolist())]
        assert src_row.dtype == torch.int64 and src_row.is_contiguous() and store.dtype == torch.int32
        calls.append((src_row.numpy().copy(), int(L), int(pad_id)))
        ids, kl = TC.token_view_oracle(rows, src_row.numpy(), L, pad_id)
        return torch.from_numpy(ids), torch.from_numpy(kl)
    monkeypatch.setattr(ops, "token_view", token_view)
    real = DT._h2d
    monkeypatch.setattr(DT, "_h2d", lambda t, d: (copies.append(tuple(t.shape)), real(t, d))[1])
    return calls, copies


def _same_as_collator(batch, g, prefix, s=""):
    """A TokenBatch against the collator's recorded {'input_ids', 'attention_mask'}: element for element, through as_dict and as ids / key_len."""
    assert isinstance(batch, bert.TokenBatch) and batch.seq_len is None
    ids, mask = g[prefix + s + "input_ids"], g[prefix + s + "attention_mask"]
    d = batch.as_dict()
    assert list(d) == ["input_ids", "attention_mask"] and d["input_ids"].dtype == d["attention_mask"].dtype == torch.int64
    assert d["input_ids"].shape == ids.shape and np.array_equal(d["input_ids"].numpy(), ids) and np.array_equal(d["attention_mask"].numpy(), mask)
    assert batch.ids.is_contiguous() and batch.key_len.dtype == torch.int32 and np.array_equal(batch.key_len.numpy(), mask.sum(1))
    assert (batch.S, batch.L) == ids.shape


def test_train_loaders_equal_the_collators_recorded_batches(stub, golden):
    calls, copies = stub
    g, c = golden("device_tokens"), TC.LOADER
    dd = TC.loader_dataset_dict(g)
    ld_l, ld_u = TC.loader_pair(dd, "cpu")
    B, BU = c["batch_size"], c["batch_size"] * c["uratio"]
    assert len(ld_l) == len(ld_u) == 2 and ld_l.keys == ("idx_lb", "x_lb", "y_lb") and ld_u.keys == ("idx_ulb", "x_ulb_w", "x_ulb_s")
    rows_u, n_u, seen, widths = TC.store_rows(ld_u.dataset), len(ld_u.dataset), set(), set()
    for epoch in range(c["epoch"]):
        ld_l.set_epoch(epoch), ld_u.set_epoch(epoch)
        calls.clear(), copies.clear()
        steps = list(zip(ld_l, ld_u))
        assert len(steps) == 2 and len(copies) == 2 and len(calls) == 6          # one copy per loader and epoch; x_lb, x_ulb_w, x_ulb_s per step
        assert all(x[2] == 0 for x in calls)                                      # [PAD]
        for t, (bl, bu) in enumerate(steps):
            pl, pu = "col/e%d/lb/%d/" % (epoch, t), "col/e%d/ulb/%d/" % (epoch, t)
            assert list(bl) == ["idx_lb", "x_lb", "y_lb"] and list(bu) == ["idx_ulb", "x_ulb_w", "x_ulb_s"]
            assert np.array_equal(bl["idx_lb"].numpy(), g[pl + "idx"]) and bl["idx_lb"].dtype == torch.int64
            assert np.array_equal(bl["y_lb"].numpy(), g[pl + "y_lb"]) and bl["y_lb"].dtype == torch.int64
            assert np.array_equal(bu["idx_ulb"].numpy(), g[pu + "idx"])
            _same_as_collator(bl["x_lb"], g, pl)
            _same_as_collator(bu["x_ulb_w"], g, pu)
            # the strong view: the drawn variant's row of the same sentence, padded to ITS OWN longest row -- the collator on those variants
            src = ld_u.draws["x_ulb_s"][0][BU * t:BU * t + BU]
            assert np.array_equal(src % n_u, g[pu + "idx"]) and np.array_equal(src // n_u - 1, g[pu + "variant"])
            _same_as_collator(bu["x_ulb_s"], g, pu, "s_")
            want, mask = TC.padded_batch(rows_u, src)
            assert np.array_equal(bu["x_ulb_s"].ids.numpy(), want) and np.array_equal(bu["x_ulb_s"].as_dict()["attention_mask"].numpy(), mask)
            assert bl["x_lb"].S == B and bu["x_ulb_w"].S == bu["x_ulb_s"].S == BU
            widths.add((bl["x_lb"].L, bu["x_ulb_w"].L, bu["x_ulb_s"].L))
            seen |= set(g[pu + "variant"].tolist())
        for k, ld, i in (("x_lb", ld_l, 0), ("x_ulb_w", ld_u, 1), ("x_ulb_s", ld_u, 1)):      # draws: the store rows and every batch's padded length
            src, lens = ld.draws[k]
            assert src.dtype == np.int64 and src.shape == (2 * ld.batch_size,) and lens.tolist() == [s[i][k].L for s in steps]
    assert seen == {0, 1}                                                         # both variants are drawn
    assert any(len(set(w)) == 3 for w in widths)                                  # the three views of a step keep their own lengths


def test_train_loader_replays_and_two_ranks_split_the_stream(stub, golden):
    calls, copies = stub
    c, dd = TC.LOADER, TC.loader_dataset_dict(golden("device_tokens"))

    def flat(ld):
        return [{k: (v.numpy().copy() if torch.is_tensor(v) else (v.ids.numpy().copy(), v.key_len.numpy().copy())) for k, v in b.items()} for b in ld]

    def eq(x, y):
        return all(np.array_equal(p, q) for p, q in zip(x, y)) if isinstance(x, tuple) else np.array_equal(x, y)

    def same(a, b):
        return len(a) == len(b) and all(list(x) == list(y) and all(eq(x[k], y[k]) for k in x) for x, y in zip(a, b))
    a, b = TC.loader_pair(dd, "cpu")[1], TC.loader_pair(dd, "cpu")[1]
    e0, e0b = flat(a), flat(b)
    assert same(e0, e0b) and same(e0, flat(a))                                    # the same seed: the same batches; iterating again replays them
    a.set_epoch(1)
    e1 = flat(a)
    assert not same(e0, e1) and not np.array_equal(e0[0]["idx_ulb"], e1[0]["idx_ulb"])
    b.set_epoch(1)
    assert same(e1, flat(b))
    a.set_epoch(0)
    assert same(e0, flat(a))                                                      # set_epoch addresses an epoch directly
    o = TC.loader_pair(dd, "cpu", seed=c["seed"] + 1)[1]
    other = flat(o)                                                               # another seed: the sampler's stream stays, the variant draws change
    assert all(np.array_equal(x["idx_ulb"], y["idx_ulb"]) and eq(x["x_ulb_w"], y["x_ulb_w"]) for x, y in zip(e0, other))
    assert not np.array_equal(o.draws["x_ulb_s"][0], a.draws["x_ulb_s"][0])
    # no strong view: not drawn, not launched, the weak view unchanged
    calls.clear()
    weak = flat(TC.loader_pair(dd, "cpu", strong=False)[1])
    assert all(list(x) == ["idx_ulb", "x_ulb_w"] for x in weak) and len(calls) == 2 and all(eq(x["x_ulb_w"], y["x_ulb_w"]) for x, y in zip(weak, e0))
    # two ranks: each takes every second index of the one-rank stream, drop_last on its own share
    ds = DT.DeviceTokenDataset.from_reference(dd["train_ulb"], "cpu")
    whole = EpochSampler(len(ds), 40, 1, 0)
    whole.set_epoch(3)
    for rank in (0, 1):
        ld = DT.TokenTrainLoader(ds, 6, EpochSampler(len(ds), 40, 2, rank), keys=("idx_ulb", "x_ulb_w", "x_ulb_s"), seed=(0, rank, 1))
        ld.set_epoch(3)
        got = flat(ld)
        assert len(ld) == len(got) == 20 // 6 and all(x["x_ulb_w"][0].shape[0] == 6 for x in got)
        assert np.array_equal(np.concatenate([x["idx_ulb"] for x in got]), whole.indices()[rank::2][:18])
    r0, r1 = (DT.TokenTrainLoader(ds, 6, EpochSampler(len(ds), 40, 2, r), keys=("idx_ulb", "x_ulb_s"), seed=(0, r, 1)) for r in (0, 1))
    r0._epoch_table(), r1._epoch_table()
    assert not np.array_equal(r0.draws["x_ulb_s"][0] // len(ds), r1.draws["x_ulb_s"][0] // len(ds))      # the rank is part of the seed
    with pytest.raises(ValueError, match="labelled"):
        DT.TokenTrainLoader(ds, 4, EpochSampler(len(ds), 12, 1, 0), keys=("idx_lb", "x_lb", "y_lb"))
    with pytest.raises(ValueError, match="strong view was asked of a dataset without data_s"):
        DT.TokenTrainLoader(DT.DeviceTokenDataset(dd["train_ulb"]["data"], None, "cpu"), 4, EpochSampler(len(ds), 12, 1, 0),
                            keys=("idx_ulb", "x_ulb_w", "x_ulb_s"))


def test_eval_loader_pads_each_batch_like_the_collator(stub, golden):
    calls, copies = stub
    g, c = golden("device_tokens"), TC.LOADER
    dd = TC.loader_dataset_dict(g)
    ds = DT.DeviceTokenDataset.from_reference(dd["eval"], "cpu")
    ld = DT.TokenEvalLoader(ds, c["eval_batch_size"])
    assert len(ld) == 3 and ld.batch_lengths() == [g["col/eval/%d/input_ids" % t].shape[1] for t in range(3)]
    for _ in range(2):                                                            # re-iterable
        calls.clear()
        got = list(ld)
        assert [b["x_lb"].S for b in got] == [3, 3, 1] and all(list(b) == ["x_lb", "y_lb"] for b in got)
        for t, b in enumerate(got):
            _same_as_collator(b["x_lb"], g, "col/eval/%d/" % t)
            assert np.array_equal(b["y_lb"].numpy(), g["col/eval/%d/y_lb" % t])
        assert np.array_equal(np.concatenate([x[0] for x in calls]), np.arange(7))
    assert not copies
    with pytest.raises(ValueError, match="labelled"):
        DT.TokenEvalLoader(DT.DeviceTokenDataset.from_reference(dd["train_ulb"], "cpu"), 4)


def test_token_batch_to_and_as_dict():
    tb = bert.TokenBatch(torch.tensor([[2, 5, 3, 0], [2, 3, 0, 0]]), torch.tensor([3, 2], dtype=torch.int32))
    assert tb.to("cpu") is tb and tb.to(torch.device("cpu"), non_blocking=True) is tb
    d = tb.as_dict()
    assert d["attention_mask"].tolist() == [[1, 1, 1, 0], [1, 1, 0, 0]] and d["input_ids"] is tb.ids
    moved = tb.to("meta")
    assert moved is not tb and moved.ids.device.type == "meta" and moved.key_len.device.type == "meta" and moved.seq_len is None and (moved.S, moved.L) == (2, 4)


# ---- 5. wiring -------------------------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    c = TC.LOADER
    d = dict(algorithm="hostonly", num_classes=c["num_classes"], num_train_iter=c["num_train_iter"], epoch=c["epoch"], ema_m=0.0, ulb_loss_ratio=1.0,
             use_cat=False, amp=False, lr=5e-4, num_eval_iter=0, num_log_iter=0, gpu=None, rank=0, world_size=1, distributed=False, dataset="aclImdb",
             num_labels=10, batch_size=c["batch_size"], uratio=c["uratio"], eval_batch_size=c["eval_batch_size"], train_sampler="RandomSampler",
             max_length=c["max_length"], seed=c["seed"], data_functions=(None, None))
    d.update(kw)
    return argparse.Namespace(**d)


TINY = dict(vocab=120, hidden=128, layers=2, heads=2, inter=512, max_pos=64)


class _HostOnly(AlgorithmBase):
    """The base class's wiring with a backbone that is never launched (CPU device) and no optimizer."""
    # bert_tiny_test's configuration, built on the CPU without its (launched) weight initialisation
    net = staticmethod(lambda nc: bert.ClassificationBert(bert.BertConfig(num_classes=nc, **TINY), device="cpu"))

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


def test_option_absent_changes_nothing(golden):
    dd = TC.loader_dataset_dict(golden("device_tokens"))
    for kw in (dict(), dict(device_tokens=False)):
        alg = _HostOnly(_args(dataset=None, **kw), None)
        assert alg.dataset_dict is None and alg.loader_dict is None and alg.device_tokens is False
        assert [type(h) for h in alg.hooks_dict.values()] == [ParamUpdateHook, EMAHook, TimerHook]
    ld = {"train_lb": [], "train_ulb": []}
    assert _HostOnly(_args(dataset=None, loader_dict=ld), None).loader_dict is ld
    with pytest.raises(RuntimeError, match="get_data_loader"):                   # a dataset_dict without the option: today's error
        _HostOnly(_args(dataset_dict=dd), None)
    with pytest.raises(NotImplementedError, match="token batches"):              # device_data with a BERT net stays refused
        _HostOnly(_args(device_data=True, net="bert_base_uncased", dataset_dict=dd), None)
    # dict batches pass through process_batch as before; a TokenBatch on the device is handed on as it is
    alg = _HostOnly(_args(dataset=None), None)
    x = {"input_ids": torch.ones(2, 3, dtype=torch.int64), "attention_mask": torch.ones(2, 3, dtype=torch.int64)}
    tb = bert.TokenBatch(torch.ones(2, 3, dtype=torch.int64), torch.full((2,), 3, dtype=torch.int32))
    out = alg.process_batch(x_lb=x, y_lb=torch.zeros(2, dtype=torch.int64), idx_ulb=None, x_ulb_w=tb, x_ulb_s=tb, idx_lb=torch.zeros(2))
    assert list(out) == ["x_lb", "y_lb", "x_ulb_w", "x_ulb_s"] and isinstance(out["x_lb"], dict) and out["x_ulb_w"] is tb and out["x_ulb_s"] is tb


def test_option_builds_the_token_loaders_and_the_seed_hook(stub, golden):
    c, g = TC.LOADER, golden("device_tokens")
    a = _args(device_tokens=True, dataset_dict=TC.loader_dataset_dict(g), net="bert_base_uncased")
    alg = _HostOnly(a, None)
    assert a.ulb_dest_len == TC.SPLITS["train_ulb"][0] and a.lb_dest_len == TC.SPLITS["train_lb"][0] and alg.device_tokens
    assert set(alg.loader_dict) == {"train_lb", "train_ulb", "eval"}
    lb, ulb, ev = (alg.loader_dict[k] for k in ("train_lb", "train_ulb", "eval"))
    assert isinstance(lb, DT.TokenTrainLoader) and isinstance(ev, DT.TokenEvalLoader) and isinstance(alg.dataset_dict["train_ulb"], DT.DeviceTokenDataset)
    assert (lb.batch_size, ulb.batch_size, ev.batch_size) == (4, 8, 3) and len(lb) == len(ulb) == 2
    assert (lb.sampler.total, ulb.sampler.total) == (2 * 4, 2 * 8)
    assert lb.keys == ("idx_lb", "x_lb", "y_lb") and ulb.keys == ("idx_ulb", "x_ulb_w", "x_ulb_s")
    assert lb.seed == (c["seed"], 0, 0) and ulb.seed == (c["seed"], 0, 1) and alg.dataset_dict["train_lb"].max_length == 16
    assert [type(h) for h in alg.hooks_dict.values()].count(DistSamplerSeedHook) == 1 and len(alg.hooks_dict) == 4
    alg.epoch = 1
    alg.call_hook("before_train_epoch")
    assert lb.epoch == ulb.epoch == lb.sampler.epoch == ulb.sampler.epoch == 1
    got = list(ulb)                                                               # epoch 1 of the wired loader: the collator's recorded batches
    assert len(got) == 2
    for t, b in enumerate(got):
        _same_as_collator(b["x_ulb_w"], g, "col/e1/ulb/%d/" % t)
        _same_as_collator(b["x_ulb_s"], g, "col/e1/ulb/%d/" % t, "s_")
    # a train_step without x_ulb_s (srpseudolabel): no strong view, and no data_s needed
    dd = TC.loader_dataset_dict(g)
    del dd["train_ulb"]["data_s"]
    weak = _HostOnlyWeak(_args(device_tokens=True, dataset_dict=dd), None)
    assert weak.loader_dict["train_ulb"].keys == ("idx_ulb", "x_ulb_w") and weak.dataset_dict["train_ulb"].n_variants == 0
    # the evaluation path takes the loader's TokenBatch as it is
    seen = []

    class Net:
        def forward_features(self, x, *a, **k):
            seen.append(x)
            return torch.zeros(x.S, 4), None, None
    pairs = list(alg._eval_batches(Net(), ev))
    assert len(pairs) == 3 and all(isinstance(x, bert.TokenBatch) for x in seen) and [x.S for x in seen] == [3, 3, 1]


def test_option_refusals_name_their_reason(stub, golden):
    g = golden("device_tokens")
    dd = lambda: TC.loader_dataset_dict(g)      # noqa: E731
    ok = dict(device_tokens=True)
    with pytest.raises(ValueError, match="device_tokens and device_data are two input pipelines"):
        _HostOnly(_args(dataset_dict=dd(), device_data=True, img_size=8, **ok), None)
    with pytest.raises(ValueError, match="device_tokens and device_audio are two input pipelines"):
        _HostOnly(_args(dataset_dict=dd(), device_audio=True, sample_rate=16000, max_length_seconds=1.0, **ok), None)
    for net in ("vit_small_patch2_32", "wave2vecv2_base", "hubert_base", "wrn_28_2"):
        with pytest.raises(NotImplementedError, match="does not take token batches"):
            _HostOnly(_args(dataset_dict="never looked at", net=net, **ok), None)          # from the yaml keys, before a dataset is looked at

    class Images(_HostOnly):                                                     # ... and from the built model, for a builder handed in without a net name
        net = staticmethod(lambda nc: vit.VisionTransformer(vit.VitConfig(img_size=8, patch_size=2, embed_dim=128, depth=2, num_heads=2, num_classes=nc),
                                                            device="cpu"))
    with pytest.raises(NotImplementedError, match="VisionTransformer.*does not take token batches"):
        Images(_args(dataset_dict=dd(), **ok), None)
    with pytest.raises(NotImplementedError, match="train_sampler 'WeightedRandomSampler'"):
        _HostOnly(_args(dataset_dict="never looked at", train_sampler="WeightedRandomSampler", **ok), None)
    with pytest.raises(ValueError, match="needs args.max_length"):
        _HostOnly(_args(dataset_dict="never looked at", max_length=None, **ok), None)
    with pytest.raises(RuntimeError, match="needs the sentences"):
        _HostOnly(_args(dataset=None, **ok), None)
    weak = dd()
    del weak["train_ulb"]["data_s"]
    with pytest.raises(ValueError, match="takes x_ulb_s but the unlabelled set has no data_s"):
        _HostOnly(_args(dataset_dict=weak, **ok), None)
    none = dd()
    none["train_ulb"] = None
    with pytest.raises(ValueError, match=r"dataset_dict\['train_ulb'\] is missing or None"):
        _HostOnly(_args(dataset_dict=none, **ok), None)
    built = DT.build_token_datasets(_args(), dd(), "cpu")
    for gone in ({**built, "train_lb": None}, {k: v for k, v in built.items() if k != "train_lb"}):
        with pytest.raises(ValueError, match=r"dataset_dict\['train_lb'\] is missing or None"):
            DT.build_token_loaders(_args(), gone, ["x_lb", "y_lb", "x_ulb_w"], 4, 2, 1, 0)
    long = dd()
    long["train_lb"]["data"][2] = np.arange(1, 18)
    with pytest.raises(ValueError, match="holds 17 tokens, more than max_length = 16"):
        _HostOnly(_args(dataset_dict=long, **ok), None)
    # after set_model, before any launch: the position table and the vocabulary of the CPU-built bert_tiny_test (64 positions, 120 ids)
    with pytest.raises(ValueError, match=r"max_length = 65 of dataset 'train_lb' exceeds the model's 64 positions"):
        _HostOnly(_args(dataset_dict=dd(), max_length=65, **ok), None)
    assert _HostOnly(_args(dataset_dict=TC.loader_dataset_dict(g, 64), max_length=64, **ok), None).loader_dict is not None
    bad = dd()
    bad["eval"]["data"][1] = np.array([2, 120, 3])
    with pytest.raises(ValueError, match=r"dataset 'eval' holds token id 120, outside the model's vocabulary of 120"):
        _HostOnly(_args(dataset_dict=bad, **ok), None)
    edge = dd()
    edge["eval"]["data"][1] = np.array([2, 119, 3])
    assert _HostOnly(_args(dataset_dict=edge, **ok), None).dataset_dict["eval"].max_id_host == 119


# ---- 6. register budget -------------------------------------------------------------------------------------------------------------------------------
def test_token_view_kernel_keeps_its_register_budget(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "semireward_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-c",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "o.o"), os.path.join(csrc, "token_view.hip")],
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
    assert len(out) == 1 and "token_view_kernel" in next(iter(out)), sorted(out)
    v = next(iter(out.values()))
    assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, v
    assert v["VGPRs"] <= 64 and v["LDS Size [bytes/block]"] == 0, v               # 8 waves per SIMD; no LDS
