"""Behind the last block's attention a forward without a backward computes only what the head reads -- the class token's row of every image:
  * srhip_mlp_fused_proj_strided (ops.mlp_fused_proj(row_pitch=...)): B rows at pitch N * D against the dense launch over all B * N rows,
  * forward_features with vit._LAST_BLOCK_CLASS_ROWS on against off, plain, scattered and over a pass-prefix tree.
Everything is bit for bit: the strided launch runs the same instructions on the rows it keeps, and touches no other row."""
import pytest
import torch

from semireward_amd import ops
from semireward_amd.algorithms.srflexmatch import _PassTree
from semireward_amd.nets import vit
from semireward_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, HD = 384, 1536
BF = torch.bfloat16


def _mlp_operands(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                       # noqa: E731
    M = B * N
    t = dict(x=(r(M, D) * 1.5 + 0.2), ao=(r(M, D) * 0.7).to(BF), Wp=(r(D, D) * 0.05).to(BF), bp=r(D) * 0.1,
             gam=torch.rand(D, generator=g) + 0.5, bet=r(D) * 0.2, W1=(r(HD, D) * 0.05).to(BF), b1=r(HD) * 0.1, W2=(r(D, HD) * 0.03).to(BF),
             b2=r(D) * 0.1)
    # per-image DropPath factors of the two branches: kept (1 / keep_prob), dropped (0) and the identity
    t["s1"] = torch.tensor([1.0 / 0.85, 0.0, 1.0, 1.0 / 0.85] * B)[:B].contiguous()
    t["s2"] = torch.tensor([1.0 / 0.8, 1.0 / 0.8, 0.0, 1.0, 0.0] * B)[:B].contiguous()
    return {k: v.to(DEV) for k, v in t.items()}


def _mlp(t, x, M, rps, **kw):
    ops.mlp_fused_proj(x, t["ao"], t["Wp"], t["bp"], t["s1"], t["gam"], t["bet"], 1e-6, t["W1"], t["b1"], t["W2"], t["b2"], t["s2"], rps, M, D, HD,
                       **kw)


@pytest.mark.parametrize("B,N", [(130, 3), (3, 257)])       # two tiles (the second with 2 valid rows); one partly filled tile at the real pitch
@pytest.mark.parametrize("ao_scaled", [False, True])
def test_strided_fused_mlp_equals_the_dense_launch_on_the_class_rows(B, N, ao_scaled):
    t = _mlp_operands(B, N, 1000 * B + N)
    M = B * N
    full = t["x"].clone()
    _mlp(t, full, M, N, ao_scaled=ao_scaled)
    cls = torch.arange(B, device=DEV) * N
    other = torch.ones(M, dtype=torch.bool, device=DEV)
    other[cls] = False
    # in place
    xs = t["x"].clone()
    _mlp(t, xs, B, 1, ao_scaled=ao_scaled, row_pitch=N * D)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(full).all())
    assert torch.equal(xs[cls], full[cls])
    assert torch.equal(xs[other], t["x"][other])
    assert not torch.equal(full[other], t["x"][other])                 # (the dense launch did compute them)
    # into another buffer
    xo = torch.full((M, D), -7.5, device=DEV)
    xin = t["x"].clone()
    _mlp(t, xin, B, 1, ao_scaled=ao_scaled, row_pitch=N * D, x_out=xo)
    torch.cuda.synchronize()
    assert torch.equal(xo[cls], full[cls])
    assert bool((xo[other] == -7.5).all())
    assert torch.equal(xin, t["x"])


def test_strided_fused_mlp_argument_errors():
    B, N = 3, 4
    t = _mlp_operands(B, N, 7)
    x = t["x"].clone()
    ln = torch.empty(B * N, D, dtype=BF, device=DEV)
    for kw in (dict(row_pitch=D - 8),                                  # rows would overlap
               dict(row_pitch=D + 4),                                  # row starts of the bf16 operand off 16 bytes
               dict(row_pitch=2 * D, ln_next=ln, next_gamma=t["gam"], next_beta=t["bet"])):     # the next norm1 rows are packed
        with pytest.raises(RuntimeError, match="code -1"):
            _mlp(t, x, B, 1, **kw)
    torch.cuda.synchronize()
    assert torch.equal(x, t["x"])
    # a pitch of D is the dense launch (next norm1 output included)
    full, ln0 = t["x"].clone(), torch.empty_like(ln)
    _mlp(t, full, B * N, N, ln_next=ln0, next_gamma=t["gam"], next_beta=t["bet"])
    s1, s2 = t["s1"].repeat_interleave(N), t["s2"].repeat_interleave(N)
    t2 = dict(t, s1=s1, s2=s2)
    _mlp(t2, x, B * N, 1, row_pitch=D, ln_next=ln, next_gamma=t["gam"], next_beta=t["bet"])
    torch.cuda.synchronize()
    assert torch.equal(x, full) and torch.equal(ln, ln0)


_MODELS = {}


def _model(tag):
    if tag not in _MODELS:
        m = (vit.vit_small_patch16_224 if tag == "small_p16_224" else vit.vit_small_patch2_32)(num_classes=100, device=DEV)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_params(m.names_shapes, 5).items()})
        m.seed = 99
        _MODELS[tag] = m
    return _MODELS[tag]


def _spy(monkeypatch):
    """Records (M, row_pitch) of every fused proj + MLP launch."""
    seen = {"mlp": []}
    mlp0 = ops.mlp_fused_proj

    def mlp(*a, **kw):
        seen["mlp"].append((a[14], kw.get("row_pitch")))
        return mlp0(*a, **kw)

    monkeypatch.setattr(ops, "mlp_fused_proj", mlp)
    return seen


# B = 5 at 1024 rows: 5 * 257 rows take the fused chain by themselves; 5 * 197 = 985 rows take it as rows split off a launch of 6 images
# (kernels_as_images), the way the step's read rows do
@pytest.mark.parametrize("tag,kai", [("small_p2_32", None), ("small_p16_224", 6)])
@pytest.mark.parametrize("scatter", [False, True])
def test_backbone_outputs_do_not_change_with_the_switch(tag, kai, scatter, monkeypatch):
    monkeypatch.setattr(vit, "_FUSED_MLP_MIN_ROWS", 1024)
    m = _model(tag)
    cfg = m.cfg
    B, N = 5, cfg.num_tokens
    g = torch.Generator().manual_seed(11)
    img = torch.randn(B, cfg.in_chans, cfg.img_size, cfg.img_size, generator=g).to(DEV)
    dp = torch.from_numpy(synth.synth_droppath(3, m.dp_probs_host.numpy(), B)).to(DEV)
    rows = torch.tensor([6, 2, 9, 0, 4], device=DEV)
    seen = _spy(monkeypatch)
    res = {}
    for on in (False, True):
        monkeypatch.setattr(vit, "_LAST_BLOCK_CLASS_ROWS", on)
        seen["mlp"].clear()
        if scatter:
            out = (torch.full((10, cfg.num_classes), float("nan"), device=DEV), torch.full((10, D), float("nan"), device=DEV), rows)
            m.forward_features(img, None, dp, save=False, out=out, kernels_as_images=kai)
            res[on] = (out[0].clone(), out[1].clone())
        else:
            lg, ft, _ = m.forward_features(img, None, dp, save=False, kernels_as_images=kai)
            res[on] = (lg.clone(), ft.clone())
        torch.cuda.synchronize()
        # the path under test did run: 12 fused launches, the last one over B rows at pitch N * D iff the switch is on
        assert len(seen["mlp"]) == cfg.depth and seen["mlp"][:-1] == [(B * N, None)] * (cfg.depth - 1)
        assert seen["mlp"][-1] == ((B, N * D) if on else (B * N, None))
    lg0, ft0 = res[False]
    lg1, ft1 = res[True]
    sel = rows if scatter else slice(None)
    assert bool(torch.isfinite(lg0[sel]).all()) and bool(torch.isfinite(ft0[sel]).all())
    assert torch.equal(lg0[sel], lg1[sel]) and torch.equal(ft0[sel], ft1[sel])
    if scatter:
        assert torch.equal(torch.isnan(lg0), torch.isnan(lg1))


@pytest.mark.parametrize("tag", ["small_p2_32", "small_p16_224"])
def test_backbone_over_a_pass_prefix_tree_does_not_change_with_the_switch(tag, monkeypatch):
    monkeypatch.setattr(vit, "_FUSED_MLP_MIN_ROWS", 1024)
    m = _model(tag)
    cfg = m.cfg
    Bt, passes = 2, 3
    g = torch.Generator().manual_seed(5)
    img = torch.randn(Bt, cfg.in_chans, cfg.img_size, cfg.img_size, generator=g).to(DEV)
    cols_img = [j for _ in range(passes) for j in range(Bt)]
    n = len(cols_img)                                                    # 6 columns: 1542 / 1182 rows
    idx = torch.tensor(cols_img, dtype=torch.int32, device=DEV)
    dpn = synth.synth_droppath(passes, m.dp_probs_host.numpy(), n)
    dp = torch.from_numpy(dpn).to(DEV)
    codes = _PassTree.codes_from_table(dpn)
    rows = torch.arange(n, device=DEV)
    seen = _spy(monkeypatch)
    res = {}
    for on in (False, True):
        monkeypatch.setattr(vit, "_LAST_BLOCK_CLASS_ROWS", on)
        seen["mlp"].clear()
        out = (torch.empty(n, cfg.num_classes, device=DEV), torch.empty(n, D, device=DEV), rows)
        tree = _PassTree(cols_img, codes, cfg.depth).upload(DEV, dp)
        m.forward_features(img, idx, tree.dp, save=False, out=out, tree=tree)
        torch.cuda.synchronize()
        last = tree.level_n[-1]
        assert seen["mlp"][-1] == ((last, cfg.num_tokens * D) if on else (last * cfg.num_tokens, None))
        res[on] = out
    # ... and both equal the unshared forward
    out_u = (torch.empty(n, cfg.num_classes, device=DEV), torch.empty(n, D, device=DEV), rows)
    m.forward_features(img, idx, dp, save=False, out=out_u)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(res[False][0]).all())
    for o in (res[True], out_u):
        assert torch.equal(res[False][0], o[0]) and torch.equal(res[False][1], o[1])
