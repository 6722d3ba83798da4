"""The backward's small sums over all rows as extra workgroups of the grouped weight-gradient launch (srhip_gemm_tn_grouped_tail_f32) against
the separate launches they replace: every output must carry the same bits -- each element is summed by one thread in the same order in both
forms, and the tiles of the product run the same code on the same remapped tile index.

What this comparison does NOT guard: the separate kernels call the same device bodies (csrc/tail_ops.h) as the merged launch, so a slip in a body
itself shows on both sides.  The bodies' arithmetic is pinned by the float64 tests of tests/test_gpu_vit_kernels.py (patch_embed_bwd_ws,
ln_grad_reduce, cls_head_bwd, the backward replays), which run the separate kernels and, through the model, the merged launch.  The tables here
have at most 108 tiles, fewer than the 768 resident slots: the small workgroups never start behind a full second round of tiles, which changes
when they run, not what they compute."""
import pytest
import torch

from semireward_amd import ops
from semireward_amd.nets import vit

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32, bf16 = torch.float32, torch.bfloat16


def _randn(shape, g, dtype=f32, scale=1.0):
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).to(dtype).to(DEV)


# (tag, img, patch, in_chans, D, hidden, depth, classes): ViT-tiny of the test suite and ViT-S/2 of the headline, both at 2 images.
# ViT-tiny: 17 tokens per image (one partial 32-token chunk), D = 128 < the 256 threads of a tail workgroup, 3 tiles in the table;
# ViT-S/2: 257 tokens (8 full chunks), D = 384 (a thread owns two features of a row), 108 tiles of one block's four products.
SHAPES = [("tiny", 8, 2, 3, 128, 512, 2, 10), ("small_p2_32", 32, 2, 3, 384, 1536, 12, 100)]


def _case(tag, HW, ps, Cin, D, Hd, depth, C, seed):
    g = torch.Generator().manual_seed(seed)
    B = 2
    N = (HW // ps) ** 2 + 1
    M, K = B * N, Cin * ps * ps
    n_ln, n_rep = 2 * depth, vit.LN_REP
    t = dict(B=B, N=N, M=M, K=K, D=D, C=C, HW=HW, ps=ps, Cin=Cin, n_ln=n_ln, n_rep=n_rep)
    # one block's four Linears: (out features, in features) = qkv, proj, fc1, fc2
    t["ops_in"] = [(_randn((M, mo), g, bf16), _randn((M, no), g, bf16)) for mo, no in ((3 * D, D), (D, D), (Hd, D), (D, Hd))]
    t["dW0"] = [_randn((a.shape[1], b.shape[1]), g) for a, b in t["ops_in"]]
    t["db0"] = [_randn((a.shape[1],), g) for a, _ in t["ops_in"]]
    t["ln_grads0"] = _randn((n_ln, 2, D), g)
    t["part0"] = _randn((n_ln, n_rep, 2, D), g)
    t["dl"], t["feat"] = _randn((B, C), g), _randn((B, D), g)
    t["dWh0"], t["dbh0"] = _randn((C, D), g), _randn((C,), g)
    t["img"] = _randn((B + 1, Cin, HW, HW), g)
    t["idx"] = torch.tensor([2, 0], dtype=torch.int32, device=DEV)
    t["dx"] = _randn((B, N, D), g)
    t["dWp0"], t["dbp0"], t["dcls0"], t["dpos0"] = _randn((D, K), g), _randn((D,), g), _randn((D,), g), _randn((N, D), g)
    return t


def _run(t, merged, n_problems):
    dW, db = [x.clone() for x in t["dW0"]], [x.clone() for x in t["db0"]]
    lng, part = t["ln_grads0"].clone(), t["part0"].clone()
    dWh, dbh = t["dWh0"].clone(), t["dbh0"].clone()
    dWp, dbp, dcls, dpos = t["dWp0"].clone(), t["dbp0"].clone(), t["dcls0"].clone(), t["dpos0"].clone()
    B, N, D, C = t["B"], t["N"], t["D"], t["C"]
    probs = [(a, b, dW[i], db[i], a.shape[1], b.shape[1], t["M"]) for i, (a, b) in enumerate(t["ops_in"])][:n_problems]
    desc, npb, ntiles, _, _ = ops.make_group_tn_desc(probs, DEV)
    ln_desc = ops.make_ln_reduce_desc([(lng[i, 0], lng[i, 1]) for i in range(t["n_ln"])], DEV)
    ws = torch.full((ops.patch_embed_bwd_ws_floats(B, t["Cin"], t["HW"], t["ps"], D),), float("nan"), dtype=f32, device=DEV)
    pe_args = (t["dx"], t["img"], t["idx"], dWp, dbp, dcls, dpos, ws, B, t["Cin"], t["HW"], t["ps"], D)
    if merged:
        ops.gemm_tn_grouped_tail_f32(desc, npb, ntiles, D, ln=(ln_desc, part, t["n_ln"], t["n_rep"]), head=(t["dl"], t["feat"], dWh, dbh, B, C),
                                     pe=(t["dx"], t["img"], t["idx"], dpos, dcls, ws, B, t["Cin"], t["HW"], t["ps"]))
        part_done = True
        ops.patch_embed_bwd_ws(*pe_args, part_done)
    else:
        ops.cls_head_bwd(t["dl"], None, None, t["feat"], None, None, None, dWh, dbh, None, None, B, N, D, C)
        ops.ln_grad_reduce(ln_desc, part, t["n_ln"], t["n_rep"], D)
        ops.gemm_tn_grouped_f32(desc, npb, ntiles, alpha=1.0, beta=1.0)
        ops.patch_embed_bwd_ws(*pe_args)
    torch.cuda.synchronize()
    out = dict(lng=lng, part=part, dWh=dWh, dbh=dbh, dWp=dWp, dbp=dbp, dcls=dcls, dpos=dpos, ws=ws)
    for i in range(len(dW)):
        out["dW%d" % i], out["db%d" % i] = dW[i], db[i]
    return out


@pytest.mark.parametrize("n_problems", [1, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_merged_tail_matches_the_separate_launches(shape, n_problems):
    t = _case(*shape, seed=31 + n_problems)
    want, got = _run(t, False, n_problems), _run(t, True, n_problems)
    for k in want:
        a, b = want[k], got[k]
        assert not bool(torch.isnan(b).any()), k                       # (the workspace too: every word is written before the fold reads it)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s: %d of %d words differ" % (
            k, int((a.view(torch.int32) != b.view(torch.int32)).sum()), a.numel())
    assert int(torch.count_nonzero(got["part"])) == 0                  # the LayerNorm copies are cleared for the next step
    for i in range(n_problems, 4):                                     # problems outside the table stay as they were
        assert torch.equal(got["dW%d" % i], t["dW0"][i]) and torch.equal(got["db%d" % i], t["db0"][i])
    for i in range(n_problems):                                        # ... and the ones inside it moved
        assert not torch.equal(got["dW%d" % i], t["dW0"][i])


def test_tail_parts_are_optional():
    """No LayerNorm copies, no head, no patch embedding: the launch is the plain product; each part alone matches its own launch."""
    t = _case(*SHAPES[0], seed=5)
    B, N, D, C = t["B"], t["N"], t["D"], t["C"]
    a, b = t["ops_in"][1]
    dW, dW2 = t["dW0"][1].clone(), t["dW0"][1].clone()
    d1 = ops.make_group_tn_desc([(a, b, dW, None, D, D, t["M"])], DEV)
    d2 = ops.make_group_tn_desc([(a, b, dW2, None, D, D, t["M"])], DEV)
    ops.gemm_tn_grouped_f32(d1[0], d1[1], d1[2], alpha=1.0, beta=1.0)
    ops.gemm_tn_grouped_tail_f32(d2[0], d2[1], d2[2], D)
    assert torch.equal(dW, dW2)
    dWh, dbh, dWh2, dbh2 = t["dWh0"].clone(), t["dbh0"].clone(), t["dWh0"].clone(), t["dbh0"].clone()
    ops.cls_head_bwd(t["dl"], None, None, t["feat"], None, None, None, dWh, dbh, None, None, B, N, D, C)
    ops.gemm_tn_grouped_tail_f32(d2[0], d2[1], d2[2], D, head=(t["dl"], t["feat"], dWh2, dbh2, B, C), beta=0.0)
    assert torch.equal(dWh, dWh2) and torch.equal(dbh, dbh2)


def test_vit_backward_takes_the_merged_launch(monkeypatch):
    """The model's whole-batch backward goes through the merged launch once and through none of the launches it replaces."""
    from oracle import vit_ref as V
    from semireward_amd.utils import synth
    cfg = V.VitCfg(num_classes=10, **V.VIT_TINY_TEST)
    model = vit.vit_tiny_test(num_classes=10, device=DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_params(V.param_shapes(cfg), 3).items()})
    n = {}
    for name in ("gemm_tn_grouped_tail_f32", "ln_grad_reduce", "gemm_tn_grouped_f32"):
        def wrapped(*a, _f=getattr(ops, name), _n=name, **k):
            n[_n] = n.get(_n, 0) + 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, wrapped)
    g = torch.Generator().manual_seed(9)
    img = _randn((2, 3, 8, 8), g)
    lg, _, ctx = model.forward_features(img, None, None, save=True)
    model.zero_grad()
    model.backward(ctx, _randn(tuple(lg.shape), g))
    torch.cuda.synchronize()
    assert n == {"gemm_tn_grouped_tail_f32": 1}, n
    assert bool(torch.isfinite(model.grad).all()) and float(model.view("pos_embed", model.grad).abs().sum()) > 0
    model.zero_grad()


def test_a_tail_output_inside_the_table_is_refused(monkeypatch):
    """The tail's workgroups run beside the tiles: with argument checks on, a tail output that a tile also writes is refused before the launch."""
    monkeypatch.setattr(ops, "_CHECK_ARGS", True)
    t = _case(*SHAPES[0], seed=6)
    B, D, C = t["B"], t["D"], t["C"]
    a, b = t["ops_in"][1]
    dW = t["dW0"][1].clone()                                           # [D, D] >= [C, D]: the head gradient is pointed into it
    d = ops.make_group_tn_desc([(a, b, dW, None, D, D, t["M"])], DEV)
    with pytest.raises(AssertionError, match="overlaps"):
        ops.gemm_tn_grouped_tail_f32(d[0], d[1], d[2], D, head=(t["dl"], t["feat"], dW[:C], t["dbh0"].clone(), B, C))
    torch.cuda.synchronize()
    assert torch.equal(dW, t["dW0"][1])                                # nothing was launched
