"""srhip_token_cat, ``token_len_bucket`` and the token engine's arenas without a GPU: the restatement of tests/_token_cat_cases.py (what
tests/test_gpu_token_cat.py holds the kernel to) against an independent numpy formulation, its checker shown to reject every planted fault, the
coverage of the kernel cases, the host refusals of ``ops.token_cat`` and of the yaml key, the wiring of the key and of the reservation, and the
bookkeeping of ``RowArena`` on CPU tensors (views, 256-byte offsets, grow-only, release before grow)."""
import argparse
import ctypes
import weakref

import numpy as np
import pytest
import torch

import _token_cat_cases as TC
import _token_strong_cases as TS
from semireward_amd import _lib, ops
from semireward_amd.core.algorithmbase import AlgorithmBase, check_token_len_bucket
from semireward_amd.nets import bert
from semireward_amd.nets.surface import RowArena


# ---- 1. the restatement and its checker ------------------------------------------------------------------------------------------------------------
def _fixture():
    ids0 = np.arange(1, 16, dtype=np.int64).reshape(3, 5)
    ids1 = np.arange(101, 115, dtype=np.int64).reshape(2, 7)
    return [(ids0, np.array([5, 2, 4], dtype=np.int32), None), (ids1, np.array([3, 6], dtype=np.int32), np.array([4, 7], dtype=np.int32))]


def test_restatement_equals_an_independent_formulation():
    for c in TC.kernel_cases():
        want = TC.token_cat_ref(c["sources"], c["L_out"], c["pad_id"])
        ids = np.concatenate([np.pad(i, ((0, 0), (0, c["L_out"] - i.shape[1])), constant_values=c["pad_id"]) for i, _, _ in c["sources"]])
        kl = np.concatenate([k for _, k, _ in c["sources"]])
        sl = np.concatenate([s if s is not None else np.full(i.shape[0], i.shape[1], dtype=np.int32) for i, _, s in c["sources"]])
        assert TC.mismatches((ids, kl, sl), want) == [], c["name"]
        assert want[0].dtype == np.int64 and want[1].dtype == want[2].dtype == np.int32
        assert (want[1] <= want[2]).all() and (want[2] <= c["L_out"]).all()


def test_bucket_rule():
    assert [TC.bucket_ref(L, 16, 64) for L in (1, 15, 16, 17, 33, 48, 49, 63, 64)] == [16, 16, 16, 32, 48, 48, 64, 64, 64]
    assert [TC.bucket_ref(L, 16, 60) for L in (47, 49, 60)] == [48, 60, 60]                       # capped by the positions
    assert [TC.bucket_ref(L, None, 64) for L in (1, 17, 64)] == [1, 17, 64] and TC.bucket_ref(5, 1, 64) == 5
    for L in range(1, 65):
        for N in (None, 1, 7, 16, 32, 64, 100):
            assert ops.token_len_bucket(L, N, 64) == TC.bucket_ref(L, N, 64)


@pytest.mark.parametrize("fault", TC.FAULTS)
def test_checker_rejects_planted_faults(fault):
    src = _fixture()
    want = TC.token_cat_ref(src, 9, 0)
    assert TC.mismatches(want, want) == []
    bad = TC.plant(fault, src, 9, 0)
    found = TC.mismatches(bad, want)
    assert found, fault
    assert {f[0] for f in found} == {dict(filler_not_pad="ids", seq_len_is_L_out="seq_len", row_at_previous_offset="ids",
                                          key_len_of_wrong_source="key_len", last_element_dropped="ids")[fault]}


def test_kernel_cases_cover_what_they_claim():
    cases = TC.kernel_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    pairs, seq, off, n_src, kinds, odd = set(), set(), set(), set(), set(), 0
    for c in cases:
        n_src.add(len(c["sources"]))
        kinds.add(c["name"].rsplit("_", 1)[1])
        Lmax = max(i.shape[1] for i, _, _ in c["sources"])
        assert c["L_out"] >= Lmax and c["L_out"] in (Lmax, Lmax + 1, TC.bucket_ref(Lmax, TC.BUCKET, TC.MAX_POS))
        odd += c["L_out"] % 2
        for (i, _, s), o in zip(c["sources"], c["off8"]):
            pairs.add(i.shape)
            seq.add(s is not None)
            off.add(o)
    assert pairs == {(S, L) for S in TC.S_SET for L in TC.L_SET} and seq == off == {True, False}
    assert n_src == {1, 2, 3, 4} and kinds == {"max", "plus1", "bucket"} and odd > 20


# ---- 2. the C ABI entry and the wrapper's refusals -----------------------------------------------------------------------------------------------------
def test_abi_entry_and_struct_layout():
    assert _lib.SIGNATURES["srhip_token_cat"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p])
    assert ctypes.sizeof(_lib.TokenSrc) == 32 and [f[0] for f in _lib.TokenSrc._fields_] == ["ids", "key_len", "seq_len", "S", "L"]
    assert _lib.TokenSrc.S.offset == 24 and _lib.TokenSrc.L.offset == 28
    assert hasattr(_lib.lib(), "srhip_token_cat") and ops.TOKEN_CAT_MAX_SRC == 4


def _src(S=2, L=3, seq=False, dtype=torch.int64, ldtype=torch.int32):
    return (torch.ones(S, L, dtype=dtype), torch.ones(S, dtype=ldtype), torch.ones(S, dtype=ldtype) if seq else None)


def test_wrapper_refuses_on_the_host_before_launching(monkeypatch):
    sent = []
    read = lambda a: [(s.S, s.L, s.seq_len) for s in ctypes.cast(a[0], ctypes.POINTER(_lib.TokenSrc))[:a[1]]]   # noqa: E731  (the table lives for the call)
    monkeypatch.setattr(ops, "_call", lambda name, *a: sent.append((name, a, read(a))))
    monkeypatch.setattr(ops, "_p", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(ops, "_s", lambda: None)
    with pytest.raises(ValueError, match="takes 1 .. 4 sources, got 5"):
        ops.token_cat([_src()] * 5, 3)
    with pytest.raises(ValueError, match="takes 1 .. 4 sources, got 0"):
        ops.token_cat([], 3)
    with pytest.raises(ValueError, match="L_out = 4 is below the L = 5 of source 1"):
        ops.token_cat([_src(), _src(L=5)], 4)
    wide = torch.ones(2, 6, dtype=torch.int64)
    with pytest.raises(ValueError, match="ids of source 0 is not contiguous"):
        ops.token_cat([(wide[:, :3], torch.ones(2, dtype=torch.int32), None)], 3)
    with pytest.raises(ValueError, match="ids of source 1 is not contiguous"):
        ops.token_cat([_src(), (wide.t()[:3].t(), torch.ones(2, dtype=torch.int32), None)], 3)
    with pytest.raises(ValueError, match="ids of source 0 is int64"):
        ops.token_cat([_src(dtype=torch.int32)], 3)
    with pytest.raises(ValueError, match="ids of source 0 is int64"):
        ops.token_cat([(torch.ones(6, dtype=torch.int64), torch.ones(2, dtype=torch.int32), None)], 3)
    with pytest.raises(ValueError, match="key_len of source 0 is int32"):
        ops.token_cat([_src(ldtype=torch.int64)], 3)
    with pytest.raises(ValueError, match="seq_len of source 0 is int32"):
        ops.token_cat([(torch.ones(2, 3, dtype=torch.int64), torch.ones(2, dtype=torch.int32), torch.ones(2, dtype=torch.int64))], 3)
    with pytest.raises(ValueError, match=r"key_len of source 0 is int32 \[2\]"):
        ops.token_cat([(torch.ones(2, 3, dtype=torch.int64), torch.ones(3, dtype=torch.int32), None)], 3)
    with pytest.raises(ValueError, match="pad_id is a token id"):
        ops.token_cat([_src()], 3, pad_id=-1)
    with pytest.raises(ValueError, match=r"out is \(int64 \[4, 5\], int32 \[4\], int32 \[4\]\)"):
        ops.token_cat([_src(), _src()], 5, out=(torch.ones(4, 6, dtype=torch.int64), torch.ones(4, dtype=torch.int32), torch.ones(4, dtype=torch.int32)))
    assert not sent                                                                              # ... before launching
    out = ops.token_cat([_src(), _src(S=1, L=5, seq=True)], 6, pad_id=7)
    (name, a, table), = sent
    assert name == "srhip_token_cat" and a[1:3] == (2, 7) and a[4] == 6 and a[3] == out[0].data_ptr()
    assert tuple(out[0].shape) == (3, 6) and out[0].dtype == torch.int64 and all(t.dtype == torch.int32 and tuple(t.shape) == (3,) for t in out[1:])
    assert table[0] == (2, 3, None) and table[1][:2] == (1, 5) and table[1][2] is not None


def test_token_batch_cat_paths(monkeypatch):
    """Equal lengths, no seq_len, no bucket: torch.cat and seq_len None, nothing launched.  Anything else: ONE token_cat call at the bucketed
    length, its outputs taken from the buffer."""
    calls = []

    def fake(sources, L_out, pad_id=0, out=None):
        calls.append((len(sources), L_out, pad_id, out is not None))
        ref = TC.token_cat_ref([(i.numpy(), k.numpy(), None if s is None else s.numpy()) for i, k, s in sources], L_out, pad_id)
        return tuple(torch.from_numpy(a) for a in ref)
    monkeypatch.setattr(ops, "token_cat", fake)
    mk = lambda S, L: bert.TokenBatch(torch.arange(1, S * L + 1, dtype=torch.int64).view(S, L), torch.full((S,), L, dtype=torch.int32))   # noqa: E731
    same = bert.TokenBatch.cat([mk(2, 5), mk(3, 5)])
    assert same.seq_len is None and (same.S, same.L) == (5, 5) and not calls
    buf = bert.TokenCatBuffer("cpu")
    mixed = bert.TokenBatch.cat([mk(2, 5), mk(3, 17), mk(1, 33)], out=buf)
    assert calls == [(3, 33, 0, True)] and mixed.seq_len.tolist() == [5, 5, 17, 17, 17, 33] and (mixed.S, mixed.L) == (6, 33)
    b = bert.TokenBatch.cat([mk(2, 5), mk(3, 17), mk(1, 33)], bucket=16, max_pos=64, pad_id=0, out=buf)
    assert calls[-1] == (3, 48, 0, True) and b.L == 48 and b.seq_len.tolist() == [5, 5, 17, 17, 17, 33]
    one = bert.TokenBatch.cat([mk(2, 5)], bucket=16, max_pos=64)                                  # a single batch is a cat of one source
    assert calls[-1] == (1, 16, 0, False) and one.L == 16 and one.seq_len.tolist() == [5, 5] and (one.ids[:, 5:] == 0).all()
    capped = bert.TokenBatch.cat([mk(1, 61)], bucket=16, max_pos=62)
    assert capped.L == 62
    again = bert.TokenBatch.cat([b, mk(1, 7)], bucket=16, max_pos=64)                             # a source's own seq_len is kept
    assert again.seq_len.tolist() == [5, 5, 17, 17, 17, 33, 7] and again.L == 48
    with pytest.raises(ValueError, match="a bucket needs max_pos"):
        bert.TokenBatch.cat([mk(1, 3)], bucket=16)
    # the buffer: grow-only, leading views, rows as aligned as a fresh tensor's
    i1, k1, s1 = buf.take(6, 48)
    store = buf.ids
    i2, k2, s2 = buf.take(3, 16)
    assert buf.ids is store and i2.data_ptr() == i1.data_ptr() and i2.is_contiguous() and tuple(i2.shape) == (3, 16)
    assert k2.data_ptr() == k1.data_ptr() and s2.data_ptr() == s1.data_ptr() != k1.data_ptr()
    buf.take(7, 48)
    assert buf.ids is not store and buf.ids.numel() == 7 * 48 and buf.lens.shape == (2, 7)


# ---- 3. the yaml key ---------------------------------------------------------------------------------------------------------------------------------
TINY = dict(vocab=120, hidden=128, layers=2, heads=2, inter=512, max_pos=64)       # bert_tiny_test's configuration


def _args(**kw):
    c = TS.LOADER
    d = dict(num_classes=c["num_classes"], num_train_iter=c["num_train_iter"], epoch=c["epoch"], algorithm="host",
             max_length=c["max_length"], batch_size=c["batch_size"], uratio=c["uratio"], eval_batch_size=c["eval_batch_size"],
             train_sampler="RandomSampler", seed=c["seed"], gpu=None, rank=0, world_size=1, distributed=False)
    d.update(kw)
    return argparse.Namespace(**d)


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


class _NoTokens(_HostOnly):
    def set_model(self):
        m = super().set_model()
        m.takes_tokens = False
        return m


def test_key_refusals_name_the_key():
    assert check_token_len_bucket(None) is None and check_token_len_bucket(16) == 16 and check_token_len_bucket(np.int64(32)) == 32
    for v in (0, -16, True, False, "16", 16.0, 1.5, [16]):
        with pytest.raises(ValueError, match="token_len_bucket: a positive integer"):
            check_token_len_bucket(v)
        with pytest.raises(ValueError, match="token_len_bucket: a positive integer"):
            _HostOnly(_args(token_len_bucket=v), None)
    with pytest.raises(ValueError, match="token_len_bucket: 16 .* does not take token batches"):
        _NoTokens(_args(token_len_bucket=16), None)
    assert _NoTokens(_args(), None).token_len_bucket is None                                      # absent: today's lengths, nothing refused
    assert _HostOnly(_args(token_len_bucket=16), None).token_len_bucket == 16


def test_device_tokens_reserves_the_largest_batch_once():
    """Every sequence of a step (labelled + weak + strong) at the longest stored row, bucketed and capped like the batches: the arenas are made
    once, when the algorithm is built, and the workspaces made later start at that size."""
    c = TS.LOADER
    n_seq = c["batch_size"] + 2 * c["batch_size"] * c["uratio"]
    for kw, L in ((dict(), 64), (dict(token_len_bucket=16), 64), (dict(token_len_bucket=48), 64)):
        alg = _HostOnly(_args(device_tokens=True, device_tokens_strong=True, dataset="aclImdb", dataset_dict=TS.loader_dataset_dict(), **kw), None)
        m = alg.model
        longest = max(int(alg.loader_dict[k].dataset.row_len_host.max()) for k in ("train_lb", "train_ulb"))
        assert longest == 64 and m._reserved == (n_seq * L, n_seq)
        ctx_arena = m._arenas[("ctx", "")]
        assert (ctx_arena.rows, ctx_arena.seqs) == (n_seq * L, n_seq) and m.arena_allocations == len(m._arenas) == 2
        assert all(a.rows == n_seq * L and a.allocations == 1 for a in m._arenas.values())
        # nothing a later call at any smaller shape asks for makes an arena again
        for B, Lb in ((n_seq, 64), (3, 19), (1, 1), (n_seq, 17)):
            ctx = m._ctx_buffers(B, Lb, "")
            assert ctx.arena is ctx_arena and tuple(ctx.qkv[1].shape) == (B * Lb, 3 * 128) and tuple(ctx.lse[0].shape) == (B, 2, Lb)
            m.enc_bwd_arena(B * Lb, ctx)
        assert m.arena_allocations == 2
        assert m._buf_rows("ix", (5, 128), torch.float32, 5).data_ptr() == m._buf_cache["ix"][0].data_ptr() and m._buf_cache["ix"][0].numel() == n_seq * L * 128
        assert m.token_cat_out.ids.numel() == n_seq * L
    # host loaders: nothing is reserved, the arenas grow on demand
    m = bert.ClassificationBert(bert.BertConfig(num_classes=4, **TINY), device="cpu")
    assert m._reserved == (0, 0) and m.arena_allocations == 0 and not m._arenas
    with pytest.raises(ValueError, match="reserve_tokens: n_seq >= 1 sequences of 1 .. 64"):
        m.reserve_tokens(4, 65)


# ---- 4. the arena ------------------------------------------------------------------------------------------------------------------------------------
SPEC = [("a", 3, "row", 5, torch.bfloat16), ("st", 2, "row", 2, torch.float32), ("lse", 2, "row", 2, torch.float32), ("f", 1, "seq", 7, torch.float32)]


def test_arena_views_and_offsets():
    a = RowArena("cpu", SPEC)
    assert a.store is None and a.allocations == 0
    assert a.reserve(24, 4) and (a.rows, a.seqs, a.allocations) == (24, 4, 1)
    off, total = a.layout(24, 4)
    assert off == a.offsets and total == a.nbytes == a.store.numel()
    starts = [o for name, *_ in SPEC for o in off[name]]
    assert starts == sorted(starts) and all(o % 256 == 0 for o in starts) and a.store.data_ptr() % 256 == 0
    sizes = dict(a=24 * 5 * 2, st=24 * 2 * 4, lse=24 * 2 * 4, f=4 * 7 * 4)
    for name, count, *_ in SPEC:                                                                  # blocks do not overlap: each holds its capacity
        assert all(b - o >= sizes[name] for o, b in zip(starts[starts.index(off[name][0]):], starts[starts.index(off[name][0]) + 1:] + [total])
                   if o in off[name])
    base = a.store.data_ptr()
    v = a.view("a", 2, (6, 5))
    assert v.dtype == torch.bfloat16 and tuple(v.shape) == (6, 5) and v.is_contiguous() and v.data_ptr() == base + off["a"][2]
    st = a.view("st", 1, (2, 6))                                                                  # the (2, M) statistics: two row views of one block
    assert st[0].data_ptr() == base + off["st"][1] and st[1].data_ptr() == st[0].data_ptr() + 6 * 4
    lse = a.view("lse", 0, (3, 2, 2))                                                             # [B, H, L] over a flat block
    assert tuple(lse.shape) == (3, 2, 2) and lse.is_contiguous() and lse.data_ptr() == base + off["lse"][0]
    f = a.view("f", 0, (4, 7))
    assert f.dtype == torch.float32 and f.data_ptr() == base + off["f"][0]
    # views of the same block at two shapes share their leading elements; writes through one are seen through the other
    a.view("a", 0, (24, 5)).fill_(3.0)
    assert float(a.view("a", 0, (2, 5)).sum()) == 30.0
    with pytest.raises(AssertionError):
        a.view("a", 0, (25, 5))                                                                   # beyond the capacity
    with pytest.raises(AssertionError):
        a.view("f", 0, (5, 7))


def test_arena_starts_large_blocks_where_the_allocator_would():
    a = RowArena("cpu", SPEC)
    off, total = a.layout(1 << 18, 4)                                                              # a: 2.5 MiB per block, st / lse: 2 MiB, f: 112 bytes
    assert all(o % (2 << 20) == 0 for name in ("a", "st", "lse") for o in off[name]) and off["f"][0] % 256 == 0
    assert off["a"] == [0, 4 << 20, 8 << 20] and off["st"][0] == 12 << 20 and total == off["f"][0] + 256
    small, _ = a.layout(100, 4)                                                                    # small blocks stay packed at 256 bytes
    assert small["a"] == [0, 1024, 2048] and small["st"] == [3072, 3072 + 1024]


def test_arena_grows_only_and_releases_before_it_grows():
    events = []

    def alloc(n):
        events.append(("alloc", n, arena.store is None, alive() is None if alive is not None else True))
        return RowArena._aligned_empty(arena, n)
    alive = None
    arena = RowArena("cpu", SPEC, on_alloc=lambda a: events.append(("made", a.allocations)), alloc=alloc)
    arena.on_release.append(lambda: events.append(("release", arena.rows)))
    assert arena.reserve(10, 2)
    old = arena.store
    alive = weakref.ref(old._base if old._base is not None else old)
    del old
    assert not arena.reserve(10, 2) and not arena.reserve(4, 1) and not arena.reserve(0, 0)     # smaller or equal: nothing happens
    assert [e[0] for e in events] == ["release", "alloc", "made"]
    assert arena.reserve(4, 3) and (arena.rows, arena.seqs) == (10, 3)                            # one capacity grows, the other is kept
    assert arena.reserve(11, 1) and (arena.rows, arena.seqs) == (11, 3) and arena.allocations == 3
    assert [e[0] for e in events] == ["release", "alloc", "made"] * 3
    # the hooks ran, and the old allocation was gone (no reference left in the arena) before the new one was asked for
    assert all(e[2] and e[3] for e in events if e[0] == "alloc")
    assert [e[1] for e in events if e[0] == "release"] == [0, 10, 10]
    assert [e[1] for e in events if e[0] == "alloc"] == [arena.layout(10, 2)[1], arena.layout(10, 3)[1], arena.layout(11, 3)[1]]
    arena.release()
    assert arena.store is None and (arena.rows, arena.seqs) == (0, 0) and events[-1] == ("release", 11)


def test_bert_context_is_views_of_one_arena_per_tag():
    m = bert.ClassificationBert(bert.BertConfig(num_classes=4, **TINY), device="cpu")
    c1 = m._ctx_buffers(3, 19, "")
    a = c1.arena
    assert m.arena_allocations == 1 and (a.rows, a.seqs) == (57, 3) and m._ctx_buffers(3, 19, "") is c1
    ref = argparse.Namespace()
    m.enc_alloc_ctx(ref, 3, 19)
    m.head_alloc_ctx(ref, 3)
    for name, want in vars(ref).items():                                                          # the shapes and dtypes of the separate buffers
        got = getattr(c1, name)
        for g, w in zip(got if isinstance(got, list) else [got], want if isinstance(want, list) else [want]):
            assert g.shape == w.shape and g.dtype == w.dtype and g.is_contiguous() and (g.data_ptr() - a.store.data_ptr()) % 256 == 0, name
        assert not isinstance(want, list) or len(got) == len(want)
    assert tuple(c1.st0.shape) == (2, 57) and len(c1.xb) == 3
    store = a.store
    c2 = m._ctx_buffers(2, 7, "")                                                                 # smaller: the same allocation, leading views
    assert a.store is store and c2.qkv[0].data_ptr() == c1.qkv[0].data_ptr() and m.arena_allocations == 1
    plan = m.enc_bwd_arena(57, c1)
    plan["by_M"][57] = "tables that hold the arena's pointers"
    assert m.arena_allocations == 2
    c3 = m._ctx_buffers(6, 64, "")                                                                # larger: replaced, every earlier view set and table dropped
    assert a.store is not store and (a.rows, a.seqs) == (384, 6) and m.arena_allocations == 3 and list(a.views) == [(6, 64)] and not plan["by_M"]
    assert m._ctx_buffers(1, 1, "other").arena is not a and m.arena_allocations == 4              # another tag: another arena
    assert c3.arena is a
