"""Shared material of tests/test_{cpu,gpu}_device_tokens.py, tools/device_tokens_golden.py and tools/device_tokens_time.py: the tiny
vocabulary, the seeded fixture sentences (ori, aug_0, aug_1), the test configuration of the loaders, the srhip_token_view kernel cases and
the numpy oracle of a view.  Nothing here needs transformers or a GPU: the token ids of the sentences and the reference collator's batches
come from tests/golden/device_tokens.npz (written by tools/device_tokens_golden.py in the build container)."""
import os

import numpy as np

# ---- the tiny vocabulary: BertTokenizerFast's vocab.txt, one token per line, the id is the line number (< 120 = bert_tiny_test's table) ----
SPECIAL = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
WORDS = ("the a an of and to in is was it this that film movie plot actor scene story good bad great poor boring funny long short "
         "very not never always really quite love hate like watch play act end start cat dog man woman time year day . , ! ?").split()
PIECES = ["##ing", "##s", "##ed", "##er", "##ly", "##est"]
VOCAB = SPECIAL + WORDS + PIECES
assert len(VOCAB) == len(set(VOCAB)) and len(VOCAB) <= 120
PAD, UNK, CLS, SEP = 0, 1, 2, 3
# what the sentences are drawn from: vocabulary words, words that split into pieces ("watching" -> watch ##ing), words outside the vocabulary
POOL = WORDS[:-4] + ["watching", "plays", "acted", "longer", "really", "shortest", "cats", "ended"] + ["zebra", "quantum", "xylophone"]
MAX_LENGTHS = (16, 64)


def write_vocab_dir(path):
    """A directory BertTokenizerFast.from_pretrained(path) loads offline: vocab.txt alone (uncased, the class defaults)."""
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "vocab.txt"), "w") as f:
        f.write("\n".join(VOCAB) + "\n")
    return path


def _sentence(rng, n_words):
    words = [POOL[i] for i in rng.integers(0, len(POOL), size=n_words)]
    return " ".join(words) + (" ." if n_words and rng.integers(0, 2) else "")


def sentences(split):
    """The seeded (ori, aug_0, aug_1) string triples of a split; evaluation carries the literal 'None' as augmentations (json_data.py:42).
    Sentence 0 of every training split is longer than any max_length, sentence 1 is the empty string, sentence 2 splits into word pieces,
    sentence 3 holds a word outside the vocabulary."""
    n, seed = SPLITS[split]
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for i in range(n):
        tri = [_sentence(rng, int(rng.integers(1, 9))) for _ in range(3)]
        if i == 0:
            tri = [_sentence(rng, 80 + v) for v in range(3)]
        elif i == 1:
            tri[0] = ""
        elif i == 2:
            tri[0] = "watching cats"
        elif i == 3:
            tri[0] = "the zebra ended"
        out.append(tuple(tri) if split != "eval" else (tri[0], "None", "None"))
    return out


SPLITS = {"train_lb": (10, 11), "train_ulb": (21, 12), "eval": (7, 13)}          # (sentences, seed)
LOADER = dict(num_classes=4, batch_size=4, uratio=2, eval_batch_size=3, num_train_iter=4, epoch=2, max_length=16, seed=7)


def targets(split):
    n, seed = SPLITS[split]
    return np.random.Generator(np.random.PCG64(100 + seed)).integers(0, LOADER["num_classes"], size=n).astype(np.int64)


def fixture_rows(g, split, max_length):
    """The recorded token ids of a split as lists of int32 arrays: (sentences, [variant 0 of every sentence, variant 1 ...] or None)."""
    flat, lens = g["tok/%d/%s/flat" % (max_length, split)], g["tok/%d/%s/len" % (max_length, split)]
    rows = np.split(flat.astype(np.int32), np.cumsum(lens)[:-1])
    n = SPLITS[split][0]
    assert len(rows) in (n, 3 * n)
    return rows[:n], ([rows[n:2 * n], rows[2 * n:]] if len(rows) == 3 * n else None)


def loader_dataset_dict(g, max_length=None):
    """The dataset_dict of the test configuration from already-tokenised rows (no tokenizer needed)."""
    ml = max_length or LOADER["max_length"]
    dd = {}
    for split in SPLITS:
        data, data_s = fixture_rows(g, split, ml)
        dd[split] = {"data": data, "targets": None if split == "train_ulb" else targets(split)}
        if data_s is not None and split == "train_ulb":
            dd[split]["data_s"] = data_s
    return dd


def loader_pair(dd, device, strong=True, seed=None):
    from semireward_amd.data import device_tokens as DT
    from semireward_amd.data.device_loader import EpochSampler
    c = LOADER
    seed = c["seed"] if seed is None else seed
    per_epoch = c["num_train_iter"] // c["epoch"]
    out = []
    for role, (name, bs, keys) in enumerate((("train_lb", c["batch_size"], ("idx_lb", "x_lb", "y_lb")),
                                             ("train_ulb", c["batch_size"] * c["uratio"], ("idx_ulb", "x_ulb_w", "x_ulb_s")))):
        ds = DT.DeviceTokenDataset.from_reference(dd[name], device, None, c["max_length"])
        out.append(DT.TokenTrainLoader(ds, bs, EpochSampler(len(ds), per_epoch * bs, 1, 0), strong=strong, keys=keys, seed=(seed, 0, role)))
    return out


def store_rows(ds):
    flat = ds.store.cpu().numpy()
    return [flat[o:o + n].copy() for o, n in zip(ds.row_off_host.tolist(), ds.row_len_host.tolist())]


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------------
def token_view_oracle(rows, src_row, L, pad_id):
    """(ids int64 [B, L], key_len int32 [B]): row b = the first L tokens of rows[src_row[b]], right-padded with pad_id; a src_row outside the
    rows gives an all-pad row of length 0."""
    src_row = np.asarray(src_row, dtype=np.int64)
    ids = np.full((src_row.size, L), pad_id, dtype=np.int64)
    key_len = np.zeros(src_row.size, dtype=np.int32)
    for b, r in enumerate(src_row.tolist()):
        if 0 <= r < len(rows):
            n = min(len(rows[r]), L)
            ids[b, :n] = rows[r][:n]
            key_len[b] = n
    return ids, key_len


def padded_batch(rows, src_row, pad_id=PAD):
    """The collator's tokenizer.pad(padding=True): (input_ids, attention_mask) padded to the batch's own longest row."""
    L = max(len(rows[r]) for r in src_row)
    ids, kl = token_view_oracle(rows, src_row, L, pad_id)
    return ids, (np.arange(L)[None, :] < kl[:, None]).astype(np.int64)


# ---- kernel cases -----------------------------------------------------------------------------------------------------------------------------
# lengths around the 4-int load (1 .. 9), a row longer than L = 512; the first row, and a last row that ends on the store's last int (8 % 4 == 0)
ROW_LENS = (5, 1, 2, 3, 4, 7, 8, 9, 13, 16, 600, 8)
KERNEL_L = (1, 4, 7, 9, 16, 512, 601)               # odd / even, 1, shorter than / equal to / longer than the longest row, 512
SENTINEL, SENTINEL32 = -0x0123456789ABCDEF, -0x01234567


def kernel_rows():
    rng = np.random.Generator(np.random.PCG64(21))
    return [rng.integers(1, 30000, size=n).astype(np.int32) for n in ROW_LENS]


def kernel_cases():
    """dict(name, src_row, L, ld_ids, pad_id) over kernel_rows(): B = 24 (every row, repeats, first and last row) at every L with ld_ids = L
    (odd L: odd pitch, every second row misaligned for 16-byte stores), L + 1 and L + 2, pad_id 0 and 103; B = 1 on the first and last row."""
    n = len(ROW_LENS)
    src24 = np.array([0, n - 1] + list(range(n)) + [10, 10, 1, 7, 7, 0, n - 1, 4, 5, 6], dtype=np.int64)
    assert src24.size == 24
    out = []
    for L in KERNEL_L:
        for extra, pad in ((0, 0), (1, 103), (2, 0)):
            out.append(dict(name="b24_L%d_ld%d_pad%d" % (L, L + extra, pad), src_row=src24, L=L, ld_ids=L + extra, pad_id=pad))
    for r, L in ((0, 5), (0, 4), (0, 9), (n - 1, 8), (n - 1, 7), (n - 1, 12), (1, 1), (10, 600)):
        out.append(dict(name="b1_r%d_L%d" % (r, L), src_row=np.array([r], dtype=np.int64), L=L, ld_ids=L + (r == 0), pad_id=7 * (L == 9)))
    return out


def launch(ds, src_row, L, ld_ids, pad_id, n_rows=None):
    """The raw entry on sentinel-filled buffers with one guard row before and after and guard columns L .. ld_ids:
    (ids [B, L], key_len [B], everything else of the two buffers as one int64 array: must still be the sentinel)."""
    import torch
    from semireward_amd import ops
    dev, B = ds.store.device, len(src_row)
    buf = torch.full((B + 2, ld_ids), SENTINEL, dtype=torch.int64, device=dev)
    kl = torch.full((B + 2,), SENTINEL32, dtype=torch.int32, device=dev)
    src = torch.as_tensor(np.asarray(src_row, dtype=np.int64), device=dev)
    ops._call("srhip_token_view", ops._p(ds.store), ops._p(ds.row_off), ops._p(ds.row_len), len(ds.row_len_host) if n_rows is None else n_rows,
              ops._p(src), B, L, pad_id, ops._p(buf[1:]), ld_ids, ops._p(kl[1:]), ops._s())
    buf, kl = buf.cpu().numpy(), kl.cpu().numpy()
    guard = np.concatenate([buf[0], buf[-1], buf[1:-1, L:].ravel()])
    return buf[1:-1, :L], kl[1:-1], (guard == SENTINEL).all() and kl[0] == SENTINEL32 and kl[-1] == SENTINEL32
