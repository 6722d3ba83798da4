"""device_tokens_strong (semireward_amd/data/device_tokens.py, csrc/token_strong.hip) without a GPU: the restatement of
tests/_token_strong_cases.py held to the invariants its specification states (it is what the kernel is tested against:
tests/test_gpu_token_strong.py) and its checker shown to trip on every planted fault; the C ABI entry and every refusal of it and of its
wrapper; the option's wiring and refusals; the loader's draws (order, replay, the length rule, the weak view untouched, one copy per epoch)
with the launch stubbed by the restatement."""
import argparse
import collections
import ctypes
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import _token_strong_cases as TS
from semireward_amd import _lib, ops
from semireward_amd.core.algorithmbase import AlgorithmBase
from semireward_amd.data import device_tokens as DT
from semireward_amd.data.device_loader import EpochSampler
from semireward_amd.nets import bert

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_KEYS = ["x_lb", "y_lb", "idx_ulb", "x_ulb_w", "x_ulb_s"]               # the train_step signature of srflexmatch / srsoftmatch / srfreematch
ULB_KEYS = ("idx_ulb", "x_ulb_w", "x_ulb_s")


# ---- 1. the restatement alone: the invariants its specification states ---------------------------------------------------------------------------
def _is_subsequence(short, full):
    it = iter(full)
    return all(x in it for x in short)


def test_restatement_invariants_on_200_seeded_rows():
    rng = np.random.Generator(np.random.PCG64(1))
    seen = collections.Counter()
    for trial in range(200):
        n = int(rng.integers(1, 80))
        row = np.concatenate([[TS.CLS], rng.integers(5, 103, size=max(n - 2, 0)), [TS.SEP]])[:n] if n > 1 else np.array([TS.CLS])
        ni = max(0, n - 2)
        op, seed = int(rng.integers(0, 5)), int(rng.integers(0, 2 ** 32))
        c = int(rng.integers(0, ni + 1))
        t = TS.apply_slot(list(row), op, c, seed, TS.MASK_ID)
        interior, t_in = list(row[1:n - 1]), t[1:len(t) - 1]
        assert t[0] == row[0] and t[-1] == row[-1]                                                  # first and last token kept
        assert len(t) == TS.out_len(n, [(op, c, seed)]) == int(ops.token_strong_len(n, op, c))
        if op in (TS.DELETE, TS.CUTOFF):
            assert len(t) == n - c and _is_subsequence(t, list(row))                                # the survivors keep their order
            if op == TS.CUTOFF and c:
                start = 1 + TS.fmix32(seed) % (ni - c + 1)
                assert 1 <= start and start + c <= n - 1 and t == list(row[:start]) + list(row[start + c:])
        elif op == TS.MASK:
            assert len(t) == n and sum(a != b for a, b in zip(t, row)) == c and all(b == TS.MASK_ID for a, b in zip(row, t) if a != b)
        elif op == TS.SWAP:
            assert len(t) == n and sorted(t_in) == sorted(interior)                                 # a permutation of the interior
        else:
            assert t == list(row)
        keys = TS.slot_keys(seed, range(1, n - 1))                                                  # (asserts that they are pairwise distinct)
        assert len(keys) == ni
        seen[op] += 1
        # both slots: the lengths of the chain equal the host rule, slot 1 on what slot 0 left
        s0, s1 = (op, c, seed), (int(rng.integers(0, 5)), int(rng.integers(0, 90)), int(rng.integers(0, 2 ** 32)))
        out, m = TS.strong_row_ref(row, s0, s1, 4096, TS.MASK_ID)
        c1 = min(s1[1], max(0, len(t) - 2))
        assert m == len(out) == TS.out_len(n, [s0, s1]) == int(ops.token_strong_len(ops.token_strong_len(n, s0[0], c), s1[0], c1))
        assert out == TS.apply_slot(t, *s1, TS.MASK_ID) and out[0] == row[0] and out[-1] == row[-1]
    assert min(seen.values()) > 20 and set(seen) == set(range(5))
    assert TS.fmix32(0) == 0 and TS.fmix32(1) == 0x514E28B7 and TS.fmix32(0xFFFFFFFF) == 0x81F16F39    # MurmurHash3's finaliser, published values


def test_slot_word_and_length_rule_agree_with_ops():
    rng = np.random.Generator(np.random.PCG64(2))
    op, c, seed = rng.integers(0, 256, size=500), rng.integers(0, 1 << 24, size=500), rng.integers(0, 2 ** 32, size=500)
    seed[:2], c[:2], op[:2] = [0xFFFFFFFF, 0x80000000], [0xFFFFFF, 0], [255, 0]                         # the sign bit of the word
    words = ops.pack_token_slot(op, c, seed)
    assert words.dtype == np.int64 and words.tolist() == [TS.pack(int(a), int(b), int(s)) for a, b, s in zip(op, c, seed)]
    assert [TS.unpack(int(w)) for w in words] == list(zip(op.tolist(), c.tolist(), seed.tolist()))
    assert all(np.array_equal(a, b) for a, b in zip(ops.unpack_token_slot(words), (op, c, seed)))
    for bad in ((256, 0, 0), (0, 1 << 24, 0), (0, 0, 1 << 32), (-1, 0, 0)):
        with pytest.raises(ValueError, match="8 bits"):
            ops.pack_token_slot(*bad)
    assert (ops.TOKEN_COPY, ops.TOKEN_DELETE, ops.TOKEN_MASK, ops.TOKEN_CUTOFF, ops.TOKEN_SWAP) == (TS.COPY, TS.DELETE, TS.MASK, TS.CUTOFF, TS.SWAP)
    assert ops.token_strong_len([10, 10, 10, 10, 10, 10], [0, 1, 2, 3, 4, 9], [3] * 6).tolist() == [10, 7, 10, 7, 10, 10]
    assert ops.token_strong_len(np.int64(1) << 40, 1, 5).dtype == np.int64


def test_case_list_covers_what_the_specification_names():
    cases = {c["name"]: c for c in TS.kernel_cases()}
    assert set(TS.ROW_NS) >= {1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512} and TS.LONG_N == 4096
    for which in (0, 1):
        c = cases["counts_slot%d" % which]
        got = collections.defaultdict(set)
        for b, r in enumerate(c["src_row"].tolist()):
            op, cnt, _ = TS.unpack(int(c["slots"][which, b]))
            got[(len(c["rows"][r]), op)].add(cnt)
        assert all(got[(n, op)] == {x for x in (0, 1, n - 3, n - 2) if 0 <= x <= max(0, n - 2)} for n in TS.ROW_NS for op in (1, 2, 3, 4))
        assert c["L"] > 512 and c["Lsrc"] == 512
    assert cases["counts_slot0"]["L"] % 4 and cases["counts_slot0"]["ld_ids"] % 2 == 1 and cases["counts_slot1"]["ld_ids"] % 2 == 0
    assert {len(cases["counts_4096"]["rows"][r]) for r in cases["counts_4096"]["src_row"]} == {4096, 4095} and cases["counts_4096"]["Lsrc"] == 4096
    for name in ("pairs", "pairs_tight"):
        c = cases[name]
        pairs = collections.Counter((len(c["rows"][r]), TS.unpack(int(a))[0], TS.unpack(int(b))[0]) for r, a, b in zip(c["src_row"], *c["slots"]))
        assert set(pairs) == {(n, a, b) for n in TS.PAIR_NS for a in range(5) for b in range(5)} and c["L"] % 4 and c["L"] > max(TS.PAIR_NS)
    assert cases["pairs_tight"]["tight"] and cases["pairs"]["ld_ids"] % 2 == 0 and cases["pairs_tight"]["ld_ids"] % 2 == 1
    d = cases["defensive"]
    assert {-1, len(d["rows"]), 1 << 40} <= set(d["src_row"].tolist()) and {9, 255} <= {TS.unpack(int(w))[0] for w in d["slots"].ravel()}
    t = cases["truncated_at_L"]
    lens = [TS.out_len(len(t["rows"][r]), [TS.unpack(int(a)), TS.unpack(int(b))]) for r, a, b in zip(t["src_row"], *t["slots"])]
    assert max(lens) > t["L"] > min(lens) and TS.expected(t)[1][1:-1].tolist() == [min(x, t["L"]) for x in lens]
    assert cases["truncated_at_Lsrc"]["Lsrc"] < max(len(r) for r in cases["truncated_at_Lsrc"]["rows"])
    for c in cases.values():                                                      # what the wrapper's host check accepts / refuses is what the list says
        lens = np.array([len(r) for r in c["rows"]], dtype=np.int32)
        if c["wrapper_ok"]:
            assert np.array_equal(ops.check_token_strong(c["src_row"], c["slots"], c["L"], lens, c["Lsrc"]), TS.expected(c)[1][1:-1])
        else:
            with pytest.raises((ValueError, IndexError)):
                ops.check_token_strong(c["src_row"], c["slots"], c["L"], lens, c["Lsrc"])


def test_checker_trips_on_every_planted_fault():
    cases = TS.kernel_cases(long_rows=False)
    good = {c["name"]: TS.expected(c) for c in cases}
    assert all(TS.mismatches(c, *good[c["name"]]) == [] for c in cases)
    for fault in TS.FAULTS:
        tripped = {c["name"]: len(TS.mismatches(c, *TS.expected(c, fault=fault), want=good[c["name"]])) for c in cases}
        print("planted fault %-26s rows that differ: %s" % (fault, tripped))
        assert any(tripped.values()), fault
        assert tripped["pairs"] and tripped["pairs_tight"], fault               # the one launch with all 25 op pairs alone catches every one
    # a write outside ids[b, 0 .. L) or past B is a mismatch too
    c = cases[1]                                                                  # (pitch above L: guard columns)
    buf, kl = (a.copy() for a in good[c["name"]])
    buf[3, c["L"]] = 0
    assert TS.mismatches(c, buf, kl) == [3]
    buf[3, c["L"]], buf[-1, 0], kl[0] = TS.SENTINEL, 5, 0
    assert TS.mismatches(c, buf, kl) == [0, buf.shape[0] - 1]


# ---- 2. the entry and the wrapper ------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_and_the_binding_matches_the_header():
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "srhip_token_strong")
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srhip.h")).read(), flags=re.S)
    decl = re.search(r"int\s+srhip_token_strong\s*\(([^)]*)\)", src).group(1).split(",")
    res, argtypes = _lib.SIGNATURES["srhip_token_strong"]
    assert res is _lib.I and len(decl) == 16 and [_lib.P if "*" in a else _lib.I for a in decl] == argtypes
    assert re.search(r"SR_TOKEN_COPY = 0, SR_TOKEN_DELETE = 1, SR_TOKEN_MASK = 2, SR_TOKEN_CUTOFF = 3, SR_TOKEN_SWAP = 4", src)
    assert re.search(r"SR_TOKEN_STRONG_MAX_LSRC = 4096", src) and ops.TOKEN_STRONG_MAX_LSRC == 4096


def test_entry_refuses_each_bad_argument():
    f = _lib.lib().srhip_token_strong
    buf = (ctypes.c_int * 64)()
    a = (ctypes.addressof(buf) + 15) & ~15                                       # a 16-byte aligned host address: never dereferenced, every call is refused first
    ok = dict(store=a, row_off=a, row_len=a, n_rows=2, src_row=a, slot0=a, slot1=a, B=2, Lsrc=16, L=8, pad_id=0, mask_id=103, ids=a, ld_ids=8,
              key_len=a, stream=None)

    def rc(**kw):
        return f(*{**ok, **kw}.values())
    for k in ("store", "row_off", "row_len", "src_row", "slot0", "slot1", "ids", "key_len"):
        assert rc(**{k: None}) == -1, k                                          # SR_EINVAL
    for kw in (dict(B=0), dict(B=-1), dict(B=65536), dict(n_rows=0), dict(Lsrc=0), dict(Lsrc=-4), dict(Lsrc=4097), dict(L=0), dict(L=-1), dict(ld_ids=7),
               dict(L=9), dict(store=a + 4), dict(store=a + 8), dict(ids=a + 4), dict(pad_id=-1), dict(mask_id=-1)):
        assert rc(**kw) == -1, kw


def _wrapper_args():
    store, off, ln = torch.zeros(24, dtype=torch.int32), torch.tensor([0, 8]), torch.tensor([5, 8], dtype=torch.int32)
    rows = np.array([1, 0, 1])
    slots = np.stack([ops.pack_token_slot([1, 2, 3], [2, 1, 6], [7, 8, 9]), ops.pack_token_slot([4, 0, 1], [3, 0, 0], [1, 2, 3])])
    return [store, off, ln, torch.from_numpy(rows), torch.from_numpy(slots[0]), torch.from_numpy(slots[1])], [rows, slots, np.array([5, 8], dtype=np.int32)]


def test_wrapper_checks_on_the_host_what_the_kernel_would_mend(monkeypatch):
    sent = []
    monkeypatch.setattr(ops, "_call", lambda name, *a: sent.append((name, a)))
    monkeypatch.setattr(ops, "_p", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(ops, "_s", lambda: None)
    a, h = _wrapper_args()
    ids, kl = ops.token_strong(*a, 8, 8, pad_id=0, mask_id=4, host=h)
    (name, s), = sent
    assert name == "srhip_token_strong" and len(s) == 16 and tuple(ids.shape) == (3, 8) and ids.dtype == torch.int64 and kl.dtype == torch.int32
    assert s[3] == 2 and s[7:12] == (3, 8, 8, 0, 4) and s[13] == 8                # n_rows; B, Lsrc, L, pad_id, mask_id; ld_ids
    assert ops.check_token_strong(*h[:2], 8, h[2], 8).tolist() == [6, 5, 2]      # 8 - 2 (swap keeps), 5 (mask, copy), 8 - 6 (delete 0)
    assert ops.check_token_strong(*h[:2], np.array([6, 5, 2]), h[2], 8).tolist() == [6, 5, 2]        # one L per row

    def bad(exc, match, i=None, v=None, hi=None, hv=None, L=8, Lsrc=8, **kw):
        a, h = _wrapper_args()
        if i is not None:
            a[i] = v
        if hi is not None:
            h[hi] = hv
        with pytest.raises(exc, match=match):
            ops.token_strong(*a, L, Lsrc, host=h, **kw)
    bad(IndexError, "src_row outside the store's 2 rows", hi=0, hv=np.array([1, 2, 1]))
    bad(IndexError, "src_row outside", hi=0, hv=np.array([1, -1, 1]))
    slots = _wrapper_args()[1][1]
    for s in (0, 1):
        w = slots.copy()
        w[s, 1] = ops.pack_token_slot(5, 0, 0)
        bad(ValueError, "slot %d holds op 5, outside 0..4" % s, hi=1, hv=w)
    w = slots.copy()
    w[0, 1] = ops.pack_token_slot(2, 4, 0)                                       # a row of 5 has 3 interior tokens
    bad(ValueError, "slot 0 of row 1 asks for 4 of the 3 interior tokens", hi=1, hv=w)
    w = slots.copy()
    w[1, 2] = ops.pack_token_slot(2, 1, 0)                                       # slot 0 deleted all 6: slot 1 meets none
    bad(ValueError, "slot 1 of row 2 asks for 1 of the 0 interior tokens", hi=1, hv=w)
    bad(ValueError, "L = 5 is below the 6 tokens row 0 comes out with", L=5)
    bad(ValueError, r"slot 0 of row 0 asks for 2 of the 1 interior", Lsrc=3)     # the row is taken up to Lsrc: a smaller interior
    bad(ValueError, "Lsrc = 4097 outside", Lsrc=4097)
    bad(ValueError, r"\[2, 3\]", hi=1, hv=slots[:, :2])
    bad(ValueError, "int64", i=3, v=torch.tensor([1, 0, 1], dtype=torch.int32))
    bad(ValueError, "int64", i=4, v=torch.zeros(2, dtype=torch.int64))
    bad(ValueError, "the store is int32", i=0, v=torch.zeros(24, dtype=torch.int64))
    bad(ValueError, "token ids", mask_id=-1)
    assert len(sent) == 1                                                         # nothing else reached the library


def test_token_strong_kernel_keeps_its_register_budget(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "semireward_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-c",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "o.o"), os.path.join(csrc, "token_strong.hip")],
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
    assert len(out) == 1 and "token_strong_kernel" in next(iter(out)), sorted(out)
    v = next(iter(out.values()))
    assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, v
    assert v["VGPRs"] <= 64 and v["LDS Size [bytes/block]"] == 2048, v            # 8 waves per SIMD; the scan's two buffers (the row is dynamic LDS)


# ---- 3. wiring -------------------------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    c = TS.LOADER
    d = dict(algorithm="hostonly", num_classes=c["num_classes"], num_train_iter=c["num_train_iter"], epoch=c["epoch"], ema_m=0.0, ulb_loss_ratio=1.0,
             use_cat=False, amp=False, lr=5e-4, num_eval_iter=0, num_log_iter=0, gpu=None, rank=0, world_size=1, distributed=False, dataset="aclImdb",
             num_labels=16, batch_size=c["batch_size"], uratio=c["uratio"], eval_batch_size=c["eval_batch_size"], train_sampler="RandomSampler",
             max_length=c["max_length"], seed=c["seed"], data_functions=(None, None), device_tokens=True)
    d.update(kw)
    return argparse.Namespace(**d)


TINY = dict(vocab=120, hidden=128, layers=2, heads=2, inter=512, max_pos=64)       # bert_tiny_test's configuration


class _HostOnly(AlgorithmBase):
    """The base class's wiring with a backbone that is never launched (CPU device) and no optimizer."""

    def set_model(self):
        self.print_fn = lambda *a: None
        return bert.ClassificationBert(bert.BertConfig(num_classes=self.num_classes, **TINY), device="cpu")

    def set_ema_model(self):
        return self.model

    def set_optimizer(self):
        return None, None

    def train_step(self, x_lb, y_lb, idx_ulb, x_ulb_w, x_ulb_s):
        raise AssertionError("not stepped")


class _HostOnlyWeak(_HostOnly):
    def train_step(self, x_lb, y_lb, x_ulb_w):
        raise AssertionError("not stepped")


def test_key_builds_strong_loaders_without_data_s():
    alg = _HostOnly(_args(device_tokens_strong=True, dataset_dict=TS.loader_dataset_dict()), None)
    ulb, lb = alg.loader_dict["train_ulb"], alg.loader_dict["train_lb"]
    assert ulb.keys == ULB_KEYS and ulb.makes_strong and alg.dataset_dict["train_ulb"].n_variants == 0
    assert (ulb.rate, ulb.mask_id, ulb.Lsrc) == (0.3, 103, 64) and alg.dataset_dict["train_ulb"].strong_mask_id == 103
    assert lb.keys == ("idx_lb", "x_lb", "y_lb") and not hasattr(lb, "Lsrc")      # nothing set up where no strong view is made
    a = _args(device_tokens_strong=True, device_tokens_strong_rate=1, device_tokens_mask_id=4, dataset_dict=TS.loader_dataset_dict())
    ulb = _HostOnly(a, None).loader_dict["train_ulb"]
    assert (ulb.rate, ulb.mask_id) == (1.0, 4)
    # an algorithm whose train_step does not take x_ulb_s makes no strong view, with or without the key
    for kw in (dict(device_tokens_strong=True), dict()):
        weak = _HostOnlyWeak(_args(dataset_dict=TS.loader_dataset_dict(), **kw), None).loader_dict["train_ulb"]
        assert weak.keys == ("idx_ulb", "x_ulb_w") and not hasattr(weak, "Lsrc")
    # the tokenizer's [MASK] when one was resolved, the yaml key before it
    tok = types.SimpleNamespace(mask_token_id=17)
    assert DT.strong_mask_id(argparse.Namespace(), tok) == 17 and DT.strong_mask_id(argparse.Namespace(device_tokens_mask_id=9), tok) == 9
    assert DT.strong_mask_id(argparse.Namespace(), None) == DT.strong_mask_id(argparse.Namespace(), types.SimpleNamespace()) == 103


def test_option_refusals_name_the_key():
    dd = TS.loader_dataset_dict
    for kw in (dict(device_tokens=False), dict(device_tokens=False, device_data=True, img_size=8)):
        with pytest.raises(ValueError, match="device_tokens_strong: True .* needs device_tokens: True"):
            _HostOnly(_args(device_tokens_strong=True, dataset_dict=dd(), **kw), None)
    with pytest.raises(ValueError, match="device_tokens_strong.*needs device_tokens"):
        DT.device_strong(argparse.Namespace(device_tokens_strong=True))
    with pytest.raises(ValueError, match="device_tokens_strong: the unlabelled set carries data_s .* one source of strong views"):
        _HostOnly(_args(device_tokens_strong=True, dataset_dict=dd(data_s=True)), None)
    for rate in (0, 0.0, -0.1, 1.01, "0.3", True, float("nan")):
        with pytest.raises(ValueError, match=r"device_tokens_strong: device_tokens_strong_rate = .* must lie in \(0, 1\]"):
            _HostOnly(_args(device_tokens_strong=True, device_tokens_strong_rate=rate, dataset_dict=dd()), None)
    # decided from the model, before any launch: the mask id against the vocabulary (120 ids) and the store's pad
    with pytest.raises(ValueError, match="device_tokens_strong: device_tokens_mask_id = 120 lies outside the model's vocabulary of 120"):
        _HostOnly(_args(device_tokens_strong=True, device_tokens_mask_id=120, dataset_dict=dd()), None)
    with pytest.raises(ValueError, match="device_tokens_strong: device_tokens_mask_id = 0 is the store's pad_id"):
        _HostOnly(_args(device_tokens_strong=True, device_tokens_mask_id=0, dataset_dict=dd()), None)
    assert _HostOnly(_args(device_tokens_strong=True, device_tokens_mask_id=119, dataset_dict=dd()), None).loader_dict["train_ulb"].mask_id == 119
    with pytest.raises(ValueError, match="this algorithm's train_step takes x_ulb_s but the unlabelled set has no data_s"):      # without the key: today's refusal
        _HostOnly(_args(dataset_dict=dd()), None)
    with pytest.raises(ValueError, match="this algorithm's train_step takes x_ulb_s but the unlabelled set has no data_s"):
        _HostOnly(_args(device_tokens_strong=False, device_tokens_strong_rate=7, dataset_dict=dd()), None)                      # (the rate is not looked at)
    # the loader itself
    ds_s = DT.DeviceTokenDataset.from_reference(dd(data_s=True)["train_ulb"], "cpu")
    with pytest.raises(ValueError, match="one source of strong views"):
        DT.TokenTrainLoader(ds_s, 8, EpochSampler(24, 24, 1, 0), keys=ULB_KEYS, device_strong=True)
    ds = DT.DeviceTokenDataset.from_reference(dd()["train_ulb"], "cpu")
    with pytest.raises(ValueError, match=r"must lie in \(0, 1\]"):
        DT.TokenTrainLoader(ds, 8, EpochSampler(24, 24, 1, 0), keys=ULB_KEYS, device_strong=True, rate=1.5)
    with pytest.raises(ValueError, match="a strong view was asked of a dataset without data_s"):
        DT.TokenTrainLoader(ds, 8, EpochSampler(24, 24, 1, 0), keys=ULB_KEYS)
    long = types.SimpleNamespace(n=2, n_variants=0, targets=None, device=torch.device("cpu"), row_len_host=np.array([9, 4097], dtype=np.int32))
    with pytest.raises(ValueError, match="device_tokens_strong: sentence 1 holds 4097 tokens, more than the 4096"):
        DT.TokenTrainLoader(long, 2, EpochSampler(2, 2, 1, 0), keys=ULB_KEYS, device_strong=True)


# ---- 4. the draws and the epoch table --------------------------------------------------------------------------------------------------------------
def _loader(device_strong=True, seed=None, data_s=False, **kw):
    c = TS.LOADER
    ds = DT.DeviceTokenDataset.from_reference(TS.loader_dataset_dict(data_s)["train_ulb"], "cpu", None, c["max_length"])
    bu, per_epoch = c["batch_size"] * c["uratio"], c["num_train_iter"] // c["epoch"]
    return DT.TokenTrainLoader(ds, bu, EpochSampler(len(ds), per_epoch * bu, 1, 0), keys=ULB_KEYS, seed=(c["seed"] if seed is None else seed, 0, 1),
                               device_strong=device_strong, **kw)


def test_draw_order_ranges_and_counts():
    n0 = np.random.Generator(np.random.PCG64(3)).integers(1, 70, size=20000)
    d = DT.draw_token_slots(np.random.Generator(np.random.PCG64(4)), n0, 0.3)
    rng = np.random.Generator(np.random.PCG64(4))                                 # the documented order: op, u, seed, whole-epoch vectors
    op, u, seed = rng.integers(1, 5, size=(2, 20000)), rng.random((2, 20000)), rng.integers(0, 2 ** 32, size=(2, 20000))
    assert np.array_equal(d["op"], op) and np.array_equal(d["seed"], seed) and set(op.ravel().tolist()) == {1, 2, 3, 4}
    pairs = np.bincount(4 * (op[0] - 1) + op[1] - 1, minlength=16)
    assert pairs.min() > 0.8 * 20000 / 16 and pairs.max() < 1.2 * 20000 / 16       # with replacement: all 16 ordered pairs
    assert seed.min() >= 0 and seed.max() < 2 ** 32 and seed.max() > 2 ** 31 and d["len"].shape == (3, 20000) and np.array_equal(d["len"][0], n0)
    for i in range(0, 20000, 41):
        n = int(n0[i])
        for s in (0, 1):
            ni = max(0, n - 2)
            c = int(np.floor(u[s, i] * 0.3 * ni))
            c = 0 if op[s, i] == TS.SWAP and ni < 2 else c
            assert c == d["c"][s, i] and 0 <= c <= ni
            n = TS.out_len(n, [(int(op[s, i]), c, 0)])
            assert n == d["len"][s + 1, i]
    assert d["c"].max() == int(0.3 * 68 - 1e-9) and (d["len"][2] >= np.minimum(n0, 2)).all()
    full = DT.draw_token_slots(np.random.Generator(np.random.PCG64(4)), n0, 1.0)
    assert (full["c"][0] <= np.maximum(n0 - 2, 0)).all() and (full["len"][2] >= np.minimum(n0, 2)).all()      # rate 1: never more than the interior


def test_epoch_table_with_and_without_the_key():
    ld, twin, plain, other_seed = _loader(), _loader(), _loader(False, data_s=True), _loader(seed=TS.LOADER["seed"] + 1)
    rows = [r for r in TS.loader_dataset_dict()["train_ulb"]["data"]]
    tables = {}
    for epoch in (0, 1):
        for x in (ld, twin, plain, other_seed):
            x.set_epoch(epoch)
        t, where, N = ld._epoch_table()
        t2 = twin._epoch_table()[0]
        tp, where_p, _ = plain._epoch_table()
        assert where == {"idx_ulb": 0, "x_ulb_w": 1, "x_ulb_s": 2} == where_p and t.shape == (5, N) and tp.shape == (3, N)
        assert np.array_equal(t, t2)                                              # the same (seed, epoch): the same slots
        assert np.array_equal(t[:2], tp[:2]) and np.array_equal(t[0], t[1])       # idx_ulb and x_ulb_w rows: what they are without the key
        assert all(np.array_equal(a, b) for a, b in zip(ld.draws["x_ulb_w"], plain.draws["x_ulb_w"]))
        assert np.array_equal(t[2], t[0]) and not np.array_equal(tp[2], tp[0])    # the clean stream, no variant rows
        sd, (src, padded) = ld.strong_draws, ld.draws["x_ulb_s"]
        assert sorted(sd) == ["c", "len", "op", "seed"] and all(sd[k].dtype == np.int64 for k in sd)
        assert np.array_equal(t[3], ops.pack_token_slot(sd["op"][0], sd["c"][0], sd["seed"][0]))
        assert np.array_equal(t[4], ops.pack_token_slot(sd["op"][1], sd["c"][1], sd["seed"][1]))
        B = ld.batch_size
        for b in range(len(ld)):                                                  # padded lengths: the maximum of the restated lengths
            want = [len(TS.strong_row_ref(rows[r], *[(int(sd["op"][s, i]), int(sd["c"][s, i]), int(sd["seed"][s, i])) for s in (0, 1)], 64, 103)[0])
                    for i, r in zip(range(B * b, B * b + B), src[B * b:B * b + B])]
            assert padded[b] == max(want) and np.array_equal(sd["len"][2][B * b:B * b + B], want)
        tables[epoch] = t
        assert not np.array_equal(other_seed._epoch_table()[0][3:], t[3:])
    assert not np.array_equal(tables[0][3:], tables[1][3:])                       # another epoch: other slots


@pytest.fixture
def stub(monkeypatch):
    """ops.token_view and ops.token_strong replaced by their numpy restatements on host tensors; launches and host-to-device copies recorded."""
    calls, copies = [], []

    def rows_of(store, row_off, row_len):
        flat = store.numpy()
        return [flat[o:o + n] for o, n in zip(row_off.tolist(), row_len.tolist())]

    def token_view(store, row_off, row_len, src_row, L, pad_id=0, host=None):
        calls.append("view")
        ids = np.full((src_row.numel(), L), pad_id, dtype=np.int64)
        rows = rows_of(store, row_off, row_len)
        for b, r in enumerate(src_row.tolist()):
            ids[b, :min(len(rows[r]), L)] = rows[r][:L]
        return torch.from_numpy(ids), torch.tensor([min(len(rows[r]), L) for r in src_row.tolist()], dtype=torch.int32)

    def token_strong(store, row_off, row_len, src_row, slot0, slot1, L, Lsrc, pad_id=0, mask_id=103, host=None):
        calls.append("strong")
        assert all(t.dtype == torch.int64 and t.is_contiguous() for t in (src_row, slot0, slot1))
        slots = np.stack([slot0.numpy(), slot1.numpy()])
        ops.check_token_strong(src_row.numpy(), slots, L, row_len.numpy(), Lsrc)
        ids, kl = TS.strong_batch_ref(rows_of(store, row_off, row_len), src_row.numpy(), slots, L, Lsrc, pad_id, mask_id)
        return torch.from_numpy(ids), torch.from_numpy(kl)
    monkeypatch.setattr(ops, "token_view", token_view)
    monkeypatch.setattr(ops, "token_strong", token_strong)
    real = DT._h2d
    monkeypatch.setattr(DT, "_h2d", lambda t, d: (copies.append(tuple(t.shape)), real(t, d))[1])
    return calls, copies


def test_loader_batches_are_the_restated_chain_of_the_recorded_draws(stub):
    calls, copies = stub
    ld, plain = _loader(mask_id=4), _loader(False, data_s=True)
    rows = TS.loader_dataset_dict()["train_ulb"]["data"]
    for epoch in (0, 1):
        ld.set_epoch(epoch), plain.set_epoch(epoch)
        calls.clear(), copies.clear()
        got = list(ld)
        assert len(got) == 3 and copies == [(5, 24)] and calls == ["view", "strong"] * 3          # one copy an epoch; one launch per view
        for t, (b, w) in enumerate(zip(got, plain)):
            assert list(b) == list(ULB_KEYS) and all(isinstance(b[k], bert.TokenBatch) for k in ULB_KEYS[1:])
            assert torch.equal(b["idx_ulb"], w["idx_ulb"]) and torch.equal(b["x_ulb_w"].ids, w["x_ulb_w"].ids) and torch.equal(b["x_ulb_w"].key_len, w["x_ulb_w"].key_len)
            ids, kl = TS.loader_batch_ref(ld, t, rows, mask_id=4)
            s = b["x_ulb_s"]
            assert np.array_equal(s.ids.numpy(), ids) and np.array_equal(s.key_len.numpy(), kl) and (s.S, s.L) == ids.shape and s.L == kl.max()
            assert s.ids.is_contiguous() and s.key_len.dtype == torch.int32 and s.seq_len is None
        again = list(ld)                                                          # iterating again replays the epoch
        assert all(torch.equal(x["x_ulb_s"].ids, y["x_ulb_s"].ids) for x, y in zip(got, again))
    assert any(not torch.equal(b["x_ulb_s"].ids[:, :min(b["x_ulb_s"].L, b["x_ulb_w"].L)], b["x_ulb_w"].ids[:, :min(b["x_ulb_s"].L, b["x_ulb_w"].L)]) for b in got)
