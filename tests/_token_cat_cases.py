"""Shared material of tests/test_{cpu,gpu}_token_cat.py and tools/token_buckets_time.py: the numpy restatement of srhip_token_cat
(csrc/token_cat.hip, include/srhip.h) -- ids, key_len and seq_len element for element --, the bucket rule of ``token_len_bucket``, the checker the
GPU test holds the launch to, the faults it must reject, and the kernel cases.  Nothing here needs a GPU."""
import numpy as np

SENTINEL, SENTINEL32 = -0x0123456789ABCDEF, -0x01234567
S_SET, L_SET = (1, 3, 8), (1, 2, 3, 7, 8, 9, 63, 64)
MAX_POS, BUCKET = 64, 16                                   # bert_tiny_test's positions; the bucket of the "bucketed" cases


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
def bucket_ref(L, bucket, max_pos):
    """``token_len_bucket: bucket``: a batch of padded length L enters the backbone at min(ceil(L / bucket) * bucket, max_pos); no bucket: L."""
    if not bucket:
        return int(L)
    return min(-(-int(L) // int(bucket)) * int(bucket), int(max_pos))


def token_cat_ref(sources, L_out, pad_id):
    """sources: [(ids int64 [S, L], key_len int32 [S], seq_len int32 [S] or None)] -> (ids int64 [sum S, L_out], key_len int32, seq_len int32).
    Written element by element on purpose: output row b is row r of source j, then pad_id up to L_out."""
    total = sum(ids.shape[0] for ids, _, _ in sources)
    out = np.empty((total, L_out), dtype=np.int64)
    kl, sl = np.empty(total, dtype=np.int32), np.empty(total, dtype=np.int32)
    b = 0
    for ids, key_len, seq_len in sources:
        S, L = ids.shape
        assert L <= L_out
        for r in range(S):
            for t in range(L_out):
                out[b, t] = ids[r, t] if t < L else pad_id
            kl[b] = key_len[r]
            sl[b] = seq_len[r] if seq_len is not None else L
            b += 1
    return out, kl, sl


def mismatches(got, want):
    """What differs between two (ids, key_len, seq_len) triples, as a list of (what, row[, column]); [] when they are the same bits."""
    bad = []
    for name, g, w in zip(("ids", "key_len", "seq_len"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        if g.shape != w.shape or g.dtype != w.dtype:
            bad.append((name, "shape/dtype", g.shape, str(g.dtype), w.shape, str(w.dtype)))
            continue
        bad += [(name,) + tuple(int(i) for i in idx) for idx in np.argwhere(g != w)[:8]]
    return bad


# ---- planted faults: what a wrong kernel could plausibly write; the checker must reject each ------------------------------------------------------
def plant(fault, sources, L_out, pad_id):
    """The restatement's result with one fault planted.  The fixtures these are used on make every fault visible (asserted by the CPU test)."""
    ids, kl, sl = (a.copy() for a in token_cat_ref(sources, L_out, pad_id))
    S0, L0 = sources[0][0].shape
    if fault == "filler_not_pad":                   # a filler id that is not pad_id
        ids[0, L_out - 1] = pad_id + 1
    elif fault == "seq_len_is_L_out":               # seq_len set to L_out instead of the row's own padded length
        sl[:] = L_out
    elif fault == "row_at_previous_offset":         # a row of source 1 written at source 0's offset
        ids[0] = ids[S0]
    elif fault == "key_len_of_wrong_source":        # key_len of source 1's first row taken from source 0
        kl[S0] = sources[0][1][0]
    elif fault == "last_element_dropped":           # the last element of a row not written: the buffer's old content shows
        ids[S0 - 1, L0 - 1] = SENTINEL
    else:
        raise KeyError(fault)
    return ids, kl, sl


FAULTS = ("filler_not_pad", "seq_len_is_L_out", "row_at_previous_offset", "key_len_of_wrong_source", "last_element_dropped")


# ---- kernel cases --------------------------------------------------------------------------------------------------------------------------------
def _source(rng, S, L, with_seq):
    ids = rng.integers(1, 30000, size=(S, L)).astype(np.int64)
    seq = rng.integers(1, L + 1, size=S).astype(np.int32) if with_seq else None
    key = np.array([rng.integers(1, (seq[r] if with_seq else L) + 1) for r in range(S)], dtype=np.int32)
    return ids, key, seq


def kernel_cases():
    """dict(name, sources, off8, L_out, pad_id): one to four sources; over the cases every S of S_SET meets every L of L_SET, sources come with
    and without a seq_len, with ids that start on a 16-byte boundary and 8 bytes off one; L_out = the longest L, that + 1 (a pitch the
    sources do not have: an odd one forces the 8-byte path on every second row) and the bucketed length (tests/test_cpu_token_cat.py
    asserts this coverage)."""
    rng = np.random.Generator(np.random.PCG64(31))
    out = []
    for n in (1, 2, 3, 4):
        for k in range(len(L_SET) * (3 if n == 1 else 1)):
            src, off8 = [], []
            for j in range(n):
                L, S = L_SET[(k + 3 * j) % len(L_SET)], S_SET[(k // len(L_SET) + (k if n > 1 else 0) + j) % len(S_SET)]
                src.append(_source(rng, S, L, with_seq=(k + j) % 2 == 1))
                off8.append((k + 2 * j) % 3 == 0)
            Lmax = max(s[0].shape[1] for s in src)
            for kind, L_out in (("max", Lmax), ("plus1", Lmax + 1), ("bucket", bucket_ref(Lmax, BUCKET, MAX_POS))):
                out.append(dict(name="n%d_k%02d_%s" % (n, k, kind), sources=src, off8=off8, L_out=L_out, pad_id=0 if kind != "plus1" else 103))
    return out


def launch(case, device):
    """The raw entry on outputs that lie inside a bit pattern (one guard row before and after ids, one guard element around the lengths):
    ((ids, key_len, seq_len) as numpy, whether every guard still holds the pattern).  A source marked off8 is a slice view that starts 8 bytes
    past a 16-byte boundary."""
    import ctypes

    import torch
    from semireward_amd import _lib, ops
    srcs, keep = [], []
    for (ids, kl, sl), off in zip(case["sources"], case["off8"]):
        flat = torch.zeros(ids.size + 2, dtype=torch.int64, device=device)
        assert flat.data_ptr() % 16 == 0
        d_ids = flat[1 if off else 0:][:ids.size].view(ids.shape)
        d_ids.copy_(torch.from_numpy(ids))
        assert d_ids.is_contiguous() and d_ids.data_ptr() % 16 == (8 if off else 0)
        d_kl = torch.from_numpy(kl).to(device)
        d_sl = None if sl is None else torch.from_numpy(sl).to(device)
        keep.append((flat, d_ids, d_kl, d_sl))
        srcs.append(_lib.TokenSrc(d_ids.data_ptr(), d_kl.data_ptr(), None if d_sl is None else d_sl.data_ptr(), ids.shape[0], ids.shape[1]))
    total, L_out = sum(s[0].shape[0] for s in case["sources"]), case["L_out"]
    buf = torch.full((total + 2, L_out), SENTINEL, dtype=torch.int64, device=device)
    lens = torch.full((2, total + 2), SENTINEL32, dtype=torch.int32, device=device)
    arr = (_lib.TokenSrc * len(srcs))(*srcs)
    ops._call("srhip_token_cat", ctypes.addressof(arr), len(srcs), case["pad_id"], buf[1:].data_ptr(), L_out, lens[0, 1:].data_ptr(),
              lens[1, 1:].data_ptr(), ops._s())
    buf, lens = buf.cpu().numpy(), lens.cpu().numpy()
    guards = (buf[0] == SENTINEL).all() and (buf[-1] == SENTINEL).all() and (lens[:, [0, -1]] == SENTINEL32).all()
    return (buf[1:-1], lens[0, 1:-1], lens[1, 1:-1]), bool(guards)
