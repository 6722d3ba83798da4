"""srhip_token_cat on the MI355X (csrc/token_cat.hip): every launch against the numpy restatement of tests/_token_cat_cases.py -- the whole
guarded output block, key_len and seq_len, bit for bit, every launch made twice --; ``ops.token_cat`` and ``TokenBatch.cat`` on top of it.
Integer results: every comparison is exact, there is no tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _token_cat_cases as TC                                          # noqa: E402
from semireward_amd import ops                                         # noqa: E402
from semireward_amd.nets import bert                                   # noqa: E402

DEV = "cuda:0"
CASES = {c["name"]: c for c in TC.kernel_cases()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_token_cat_against_the_restatement(name):
    c = CASES[name]
    want = TC.token_cat_ref(c["sources"], c["L_out"], c["pad_id"])
    (first, guards1), (second, guards2) = TC.launch(c, DEV), TC.launch(c, DEV)
    assert TC.mismatches(first, want) == [], (name, [(s[0].shape, s[2] is not None, o) for s, o in zip(c["sources"], c["off8"])], c["L_out"])
    assert guards1 and guards2                                                       # nothing outside the outputs was written
    assert TC.mismatches(second, first) == []                                        # equal inputs give equal bits


def _dev(src):
    return [(torch.from_numpy(i).to(DEV), torch.from_numpy(k).to(DEV), None if s is None else torch.from_numpy(s).to(DEV)) for i, k, s in src]


def test_wrapper_allocates_or_fills_the_outputs_it_is_given():
    c = CASES["n3_k05_bucket"]
    want = TC.token_cat_ref(c["sources"], c["L_out"], 7)
    got = ops.token_cat(_dev(c["sources"]), c["L_out"], 7)
    assert got[0].is_contiguous() and TC.mismatches([t.cpu().numpy() for t in got], want) == []
    total = want[0].shape[0]
    out = (torch.full((total, c["L_out"]), -1, dtype=torch.int64, device=DEV), torch.full((total,), -1, dtype=torch.int32, device=DEV),
           torch.full((total,), -1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    src = _dev(c["sources"])
    held = torch.cuda.memory_allocated()
    back = ops.token_cat(src, c["L_out"], 7, out=out)
    assert torch.cuda.memory_allocated() == held > before                            # nothing allocated when the outputs are passed in
    assert all(a is b for a, b in zip(back, out)) and TC.mismatches([t.cpu().numpy() for t in out], want) == []
    # what the entry refuses itself (the wrapper refuses these on the host first)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops._call("srhip_token_cat", None, 1, 0, out[0].data_ptr(), 4, out[1].data_ptr(), out[2].data_ptr(), ops._s())


def test_token_batch_cat_of_unequal_lengths_and_the_equal_path():
    rng = np.random.Generator(np.random.PCG64(5))
    mk = lambda S, L: (rng.integers(1, 120, size=(S, L)).astype(np.int64), rng.integers(1, L + 1, size=S).astype(np.int32), None)   # noqa: E731
    src = [mk(4, 5), mk(8, 17), mk(8, 33)]
    batches = [bert.TokenBatch(i, k) for i, k, _ in _dev(src)]
    buf = bert.TokenCatBuffer(DEV)
    for bucket, L_out in ((None, 33), (16, 48), (64, 64)):
        want = TC.token_cat_ref(src, L_out, 0)
        tb = bert.TokenBatch.cat(batches, bucket=bucket, max_pos=64, out=buf)
        assert (tb.S, tb.L) == (20, L_out) and tb.ids.is_contiguous() and tb.ids.data_ptr() == buf.ids.data_ptr()
        assert TC.mismatches((tb.ids.cpu().numpy(), tb.key_len.cpu().numpy(), tb.seq_len.cpu().numpy()), want) == []
        fresh = bert.TokenBatch.cat(batches, bucket=bucket, max_pos=64)             # without a buffer: the same tensors, freshly allocated
        assert torch.equal(fresh.ids, tb.ids) and torch.equal(fresh.seq_len, tb.seq_len) and fresh.ids.data_ptr() != tb.ids.data_ptr()
    # a joined batch as a source: its rows keep their own padded lengths
    joined = bert.TokenBatch.cat(batches)
    again = bert.TokenBatch.cat([joined, batches[0]], bucket=16, max_pos=64)
    assert again.L == 48 and again.seq_len.cpu().tolist() == [5] * 4 + [17] * 8 + [33] * 8 + [5] * 4
    # equal lengths, no seq_len, no bucket: concatenated as they are
    same = bert.TokenBatch.cat([batches[1], batches[1]])
    assert same.seq_len is None and (same.S, same.L) == (16, 17) and torch.equal(same.ids[:8], batches[1].ids) and torch.equal(same.ids[8:], batches[1].ids)
    assert torch.equal(same.key_len, torch.cat([batches[1].key_len] * 2))
