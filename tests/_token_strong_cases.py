"""The specification of the device-made strong token view (``device_tokens_strong: True``; csrc/token_strong.hip, srhip_token_strong) and the
cases it is tested on: shared by tests/test_{cpu,gpu}_token_strong.py and tools/token_strong_time.py.  Nothing here needs a GPU.

The chain is the engine's own (it is not the reference's back-translation).  ``strong_row_ref`` restates it in exact integers:

  a row is t[0 .. n - 1], n = min(row_len, Lsrc); t[0] is [CLS], t[n - 1] is [SEP]: never moved, changed or removed.  The interior is positions
  1 .. n - 2, ni = max(0, n - 2) of them.  Two slots (op, c, seed) one after the other, slot 1 on the row and the ni slot 0 left; c is clamped
  to 0 .. ni; an op above 4 acts as COPY.
    COPY    nothing
    DELETE  interior position i is removed iff rank_i < c;  key_i = fmix32(seed + i * 0x9E3779B1) mod 2^32, rank_i = #{interior j: key_j < key_i},
            i the position in the row as THAT slot sees it.  The keys of a row are pairwise distinct (odd multiplier, fmix32 a bijection):
            asserted here, no tie rule.  n -= c
    MASK    the same selection; the selected tokens become mask_id
    CUTOFF  the c consecutive positions from start = 1 + fmix32(seed) % (ni - c + 1) are removed;  n -= c
    SWAP    for k = 0 .. c - 1 in order: a = 1 + fmix32(seed + 2k * 0x9E3779B1) % ni, b = 1 + fmix32(seed + (2k + 1) * 0x9E3779B1) % ni, t[a] <-> t[b];
            nothing when ni < 2
  The row then leaves like a token-view row: truncated at L (key_len with it), right-padded with pad_id; a src_row outside the store gives an
  all-pad row with key_len 0; columns L .. ld_ids and rows past B keep what they held.

``fault=`` plants one of FAULTS into the restatement: tests/test_cpu_token_strong.py shows that the checker (``mismatches``) trips on every one
of them on this case list -- a kernel with such a bug cannot pass."""
import numpy as np

COPY, DELETE, MASK, CUTOFF, SWAP = range(5)
GOLDEN, M32 = 0x9E3779B1, 0xFFFFFFFF
PAD, CLS, SEP, MASK_ID = 0, 2, 3, 103
SENTINEL, SENTINEL32 = -0x0123456789ABCDEF, -0x01234567
FAULTS = ("sep_dropped", "start_off_by_one", "rank_le", "swaps_reversed", "slot1_on_slot0_positions", "key_len_stale")


def fmix32(h):
    """csrc/common.h fmix32 (the MurmurHash3 finaliser), on a Python int."""
    h &= M32
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    return h ^ h >> 16


def pack(op, c, seed):
    """The int64 slot word: bits 0..7 op, 8..31 c, 32..63 seed (ops.pack_token_slot restates this; the CPU test compares them)."""
    w = (op & 0xFF) | (c & 0xFFFFFF) << 8 | (seed & M32) << 32
    return w - (1 << 64) if w >> 63 else w


def unpack(w):
    w &= (1 << 64) - 1
    return w & 0xFF, w >> 8 & 0xFFFFFF, w >> 32


def slot_keys(seed, positions):
    keys = [fmix32(seed + i * GOLDEN) for i in positions]
    assert len(set(keys)) == len(keys)                    # pairwise distinct: no tie rule is needed
    return keys


def apply_slot(t, op, c, seed, mask_id, origin=None, fault=None):
    """One slot on the list ``t`` -> the new list.  ``origin`` (the planted fault 'slot1_on_slot0_positions' only): where every token sat
    before slot 0, kept in step with ``t``."""
    n = len(t)
    ni = max(0, n - 2)
    c = min(max(int(c), 0), ni)
    if op in (DELETE, MASK):
        keys = slot_keys(seed, range(1, n - 1) if origin is None else origin[1:n - 1])
        order = sorted(range(ni), key=keys.__getitem__)
        rank = [0] * ni
        for r, i in enumerate(order):
            rank[i] = r                                   # the number of interior keys below key_i
        sel = {1 + i for i in range(ni) if (rank[i] <= c if fault == "rank_le" else rank[i] < c)}
        if op == MASK:
            return [mask_id if i in sel else x for i, x in enumerate(t)]
        gone = sel
    elif op == CUTOFF:
        start = (0 if fault == "start_off_by_one" else 1) + fmix32(seed) % (ni - c + 1)
        gone = set(range(start, start + c))
    elif op == SWAP:
        t = list(t)
        if ni >= 2:
            for k in (reversed(range(c)) if fault == "swaps_reversed" else range(c)):
                a = 1 + fmix32(seed + 2 * k * GOLDEN) % ni
                b = 1 + fmix32(seed + (2 * k + 1) * GOLDEN) % ni
                t[a], t[b] = t[b], t[a]
        return t
    else:
        return list(t)
    if fault == "sep_dropped" and gone:
        gone = gone | {n - 1}
    if origin is not None:
        origin[:] = [o for i, o in enumerate(origin) if i not in gone]
    return [x for i, x in enumerate(t) if i not in gone]


def strong_row_ref(row, slot0, slot1, Lsrc, mask_id, fault=None):
    """(tokens after both slots as a list of ints, their number).  ``slot0`` / ``slot1``: (op, c, seed)."""
    t = [int(x) for x in row[:Lsrc]]
    n0 = len(t)
    origin = list(range(n0)) if fault == "slot1_on_slot0_positions" else None
    t = apply_slot(t, *slot0, mask_id, fault=fault)
    if origin is not None:                                # where slot 0's survivors sat: replay slot 0 on the positions themselves
        origin = apply_slot(origin, *slot0, -1) if slot0[0] in (DELETE, CUTOFF) else origin
    t = apply_slot(t, *slot1, mask_id, origin=origin, fault=fault)
    return t, (n0 if fault == "key_len_stale" else len(t))


def strong_batch_ref(rows, src_row, slots, L, Lsrc, pad_id, mask_id, fault=None):
    """(ids int64 [B, L], key_len int32 [B]) of one launch; ``slots`` the packed words, int64 [2, B]."""
    src_row, slots = np.asarray(src_row, dtype=np.int64), np.asarray(slots, dtype=np.int64)
    ids = np.full((src_row.size, L), pad_id, dtype=np.int64)
    key_len = np.zeros(src_row.size, dtype=np.int32)
    for b, r in enumerate(src_row.tolist()):
        if 0 <= r < len(rows):
            t, n = strong_row_ref(rows[r], unpack(int(slots[0, b])), unpack(int(slots[1, b])), Lsrc, mask_id, fault)
            ids[b, :min(len(t), L)] = t[:L]
            key_len[b] = min(n, L)
    return ids, key_len


def out_len(n, slots):
    """The host's length rule, slot by slot, in plain ints (ops.token_strong_len restates it vectorised)."""
    for op, c, _ in slots:
        c = min(c, max(0, n - 2))
        n -= c if op in (DELETE, CUTOFF) else 0
    return n


# ---- the kernel cases ------------------------------------------------------------------------------------------------------------------------
ROW_NS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512)       # around a wave, the workgroup (one and two tokens a thread), the usual max_length
LONG_N = 4096                                                      # the cap: 16 tokens a thread, 32 KiB of LDS
PAIR_NS = (5, 12, 64, 257)


def make_rows(lengths, seed):
    """[CLS] w .. [SEP] rows of the given lengths, words in 5 .. 102 (never pad, never 103); a row of one token is [CLS] alone."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [np.concatenate([[CLS], rng.integers(5, 103, size=max(n - 2, 0)), [SEP]])[:n].astype(np.int32) if n > 1 else np.array([CLS], dtype=np.int32)
            for n in lengths]


def _counts(ni):
    return sorted({c for c in (0, 1, ni - 1, ni) if 0 <= c <= ni})


def _case(name, rows, src, slot_pairs, L, ld_ids, Lsrc=None, pad_id=PAD, mask_id=MASK_ID, tight=False, wrapper_ok=True):
    slots = np.array([[pack(*a) for a, _ in slot_pairs], [pack(*b) for _, b in slot_pairs]], dtype=np.int64)
    return dict(name=name, rows=rows, src_row=np.asarray(src, dtype=np.int64), slots=slots, L=L, ld_ids=ld_ids,
                Lsrc=max(len(r) for r in rows) if Lsrc is None else Lsrc, pad_id=pad_id, mask_id=mask_id, tight=tight, wrapper_ok=wrapper_ok)


def kernel_cases(long_rows=True):
    """Every launch the kernel is held to.  ``wrapper_ok``: False where the inputs are ones ops.check_token_strong refuses (the kernel's
    defensive rules), reachable through the raw entry only."""
    out = []
    rng = np.random.Generator(np.random.PCG64(77))
    seed = lambda: int(rng.integers(0, 2 ** 32))                   # noqa: E731
    # 1. each op at c = 0, 1, ni - 1, ni on every row length, in slot 0 (slot 1 copies) and in slot 1 (slot 0 copies)
    rows = make_rows(ROW_NS, 31)
    for which in (0, 1):
        src, sp = [], []
        for r, n in enumerate(ROW_NS):
            for op in (DELETE, MASK, CUTOFF, SWAP):
                for c in _counts(max(0, n - 2)):
                    src.append(r)
                    s = (op, c, seed())
                    sp.append((s, (COPY, 0, 0)) if which == 0 else ((COPY, 0, seed()), s))
        out.append(_case("counts_slot%d" % which, rows, src, sp, L=515 + which, ld_ids=515 + 3 * which))      # L 515 / 516 above the longest row, pitch 515 (odd) / 518 (even)
    if long_rows:
        rows4k = make_rows((LONG_N, LONG_N - 1, 7), 32)
        src, sp = [], []
        for r, n in ((0, LONG_N), (1, LONG_N - 1)):
            for op in (DELETE, MASK, CUTOFF, SWAP):
                for c in _counts(n - 2):
                    s0 = (op, c, seed())
                    src.append(r)
                    sp.append((s0, (DELETE, min(5, out_len(n, [s0]) - 2), seed())))
        out.append(_case("counts_4096", rows4k, src, sp, L=LONG_N, ld_ids=LONG_N))
    # 2. all 25 op pairs in one launch over rows of different lengths, a third of the interior each; once more from a tightly packed store
    rows = make_rows(PAIR_NS, 33)
    src, sp = [], []
    for r, n in enumerate(PAIR_NS):
        for op0 in range(5):
            for op1 in range(5):
                s0 = (op0, (n - 2 + 2) // 3, seed())
                s1 = (op1, (out_len(n, [s0]) - 2 + 2) // 3, seed())
                src.append(r)
                sp.append((s0, s1))
    out.append(_case("pairs", rows, src, sp, L=259, ld_ids=260))                                               # L % 4 = 3, above the longest row
    out.append(_case("pairs_tight", rows, src, sp, L=258, ld_ids=261, tight=True, pad_id=7, mask_id=4))       # rows start off a 16-byte boundary
    # 3. the defensive rules
    rows = make_rows((64, 9, 3, 30), 34)
    src = [0, -1, 4, 1, 1 << 40, 2, 3, 0, 3]
    sp = [((DELETE, 10, seed()), (SWAP, 9, seed())), ((DELETE, 1, seed()), (MASK, 1, seed())), ((MASK, 2, seed()), (COPY, 0, 0)),
          ((9, 3, seed()), (CUTOFF, 2, seed())),                   # op 9: a copy
          ((SWAP, 3, seed()), (SWAP, 3, seed())),
          ((DELETE, 5, seed()), (MASK, 70, seed())),               # c above ni = 1: clamped
          ((CUTOFF, 200, seed()), (255, 1, seed())),               # c above ni = 28: the whole interior goes
          ((MASK, 62, seed()), (DELETE, 0xFFFFFF, seed())),
          ((SWAP, 0xFFFFFF, seed()), (CUTOFF, 3, seed()))]        # c clamped to ni swaps
    out.append(_case("defensive", rows, src, sp, L=66, ld_ids=67, wrapper_ok=False))
    out.append(_case("truncated_at_L", rows, [0, 3, 1, 2], sp[:4], L=7, ld_ids=8, wrapper_ok=False))           # rows 0 and 3 come out longer than L
    out.append(_case("truncated_at_Lsrc", rows, [0, 3, 1, 2, 0], sp[4:9], L=41, ld_ids=41, Lsrc=40, wrapper_ok=False))     # n = min(row_len, Lsrc)
    return out


def expected(case, fault=None):
    """The two buffers of a launch as they must come back: (ids int64 [B + 2, ld_ids], key_len int32 [B + 2]) -- one guard row before and
    after and the columns L .. ld_ids still hold the sentinel."""
    B, L = case["src_row"].size, case["L"]
    buf = np.full((B + 2, case["ld_ids"]), SENTINEL, dtype=np.int64)
    kl = np.full(B + 2, SENTINEL32, dtype=np.int32)
    buf[1:-1, :L], kl[1:-1] = strong_batch_ref(case["rows"], case["src_row"], case["slots"], L, case["Lsrc"], case["pad_id"], case["mask_id"], fault)
    return buf, kl


def mismatches(case, buf, kl, want=None):
    """The checker: the rows of a launch's buffers that differ from the restatement (the whole [B + 2, ld_ids] buffer and key_len, bit for
    bit).  Empty: the launch is right."""
    want_buf, want_kl = want or expected(case)
    assert buf.shape == want_buf.shape and kl.shape == want_kl.shape and buf.dtype == np.int64 and kl.dtype == np.int32
    return sorted(set(np.flatnonzero((buf != want_buf).any(axis=1)).tolist()) | set(np.flatnonzero(kl != want_kl).tolist()))


def store_of(case, device):
    """The flat int32 store of a case on ``device``: rows on multiples of 4 ints, or -- ``tight`` -- packed back to back behind one leading
    int, so that rows start at every residue mod 4."""
    import torch
    lens = np.array([len(r) for r in case["rows"]], dtype=np.int32)
    if case["tight"]:
        off = 1 + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        assert len(set((off % 4).tolist())) > 1
    else:
        off = np.concatenate([[0], np.cumsum((lens.astype(np.int64) + 3) & ~3)[:-1]]).astype(np.int64)
    flat = np.full(int(off[-1] + lens[-1]), -7, dtype=np.int32)      # the gaps hold no token id: a read past a row would show
    for r, o in zip(case["rows"], off):
        flat[o:o + len(r)] = r
    return tuple(torch.from_numpy(a).to(device) for a in (flat, off, lens))


def launch(case, device, store=None):
    """The raw entry on sentinel-filled buffers -> (ids [B + 2, ld_ids], key_len [B + 2]) as numpy arrays."""
    import torch
    from semireward_amd import ops
    flat, off, lens = store or store_of(case, device)
    B = case["src_row"].size
    buf = torch.full((B + 2, case["ld_ids"]), SENTINEL, dtype=torch.int64, device=device)
    kl = torch.full((B + 2,), SENTINEL32, dtype=torch.int32, device=device)
    src, slots = torch.from_numpy(case["src_row"]).to(device), torch.from_numpy(case["slots"]).to(device)
    ops._call("srhip_token_strong", ops._p(flat), ops._p(off), ops._p(lens), len(case["rows"]), ops._p(src), ops._p(slots[0]), ops._p(slots[1]), B,
              case["Lsrc"], case["L"], case["pad_id"], case["mask_id"], ops._p(buf[1:]), case["ld_ids"], ops._p(kl[1:]), ops._s())
    return buf.cpu().numpy(), kl.cpu().numpy()


# ---- the loader configuration: 24 unlabelled rows of 2 .. 64 tokens, batch 8, bert_tiny_test (vocabulary 120) ----------------------------------
LOADER = dict(num_classes=4, batch_size=8, uratio=1, eval_batch_size=8, num_train_iter=6, epoch=2, max_length=64, seed=5, vocab=120)
ULB_LENS = (2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 20, 24, 29, 31, 32, 33, 40, 47, 48, 55, 60, 63, 64)
assert len(ULB_LENS) == 24


def loader_dataset_dict(data_s=False):
    rng = np.random.Generator(np.random.PCG64(41))
    lb_lens, ev_lens = rng.integers(2, 65, size=16), rng.integers(2, 65, size=10)
    dd = {"train_lb": {"data": make_rows(lb_lens, 42), "targets": rng.integers(0, LOADER["num_classes"], size=16)},
          "train_ulb": {"data": make_rows(ULB_LENS, 43), "targets": None},
          "eval": {"data": make_rows(ev_lens, 44), "targets": rng.integers(0, LOADER["num_classes"], size=10)}}
    if data_s:
        dd["train_ulb"]["data_s"] = [make_rows(ULB_LENS, 45 + v) for v in range(2)]
    return dd


def loader_batch_ref(loader, t, rows, mask_id=MASK_ID, pad_id=PAD):
    """Batch ``t`` of the epoch ``loader`` last started, restated from its recorded draws: strong_batch_ref on ``loader.strong_draws``."""
    sd, B = loader.strong_draws, loader.batch_size
    src = loader.draws["x_ulb_s"][0][B * t:B * t + B]
    slots = np.array([[pack(int(sd["op"][s, i]), int(sd["c"][s, i]), int(sd["seed"][s, i])) for i in range(B * t, B * t + B)] for s in (0, 1)],
                     dtype=np.int64)
    L = max(out_len(len(rows[r]), [unpack(int(slots[0, b])), unpack(int(slots[1, b]))]) for b, r in enumerate(src.tolist()))
    return strong_batch_ref(rows, src, slots, L, max(len(r) for r in rows), pad_id, mask_id)
