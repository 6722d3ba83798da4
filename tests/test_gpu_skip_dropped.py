"""A branch whose DropPath factor is exactly 0 is skipped on the bf16 inference rows instead of being computed and multiplied by zero:
  * srhip_vit_droppath_plan against the numpy stable partition of tests/_droppath_plan_cases.py, exactly,
  * srhip_attn_block_fused: an image whose out_scale is 0 gets +0 rows, the others do not notice,
  * srhip_mlp_fused_proj_planned against srhip_mlp_fused_proj on the same inputs, bit for bit, every row,
  * forward_features with vit._SKIP_DROPPED_BRANCHES on against off, plain, scattered and beside a pass-prefix tree."""
import numpy as np
import pytest
import torch

import _droppath_plan_cases as C
from semireward_amd import _lib, ops
from semireward_amd.algorithms.srflexmatch import _PassTree
from semireward_amd.nets import vit
from semireward_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 384
BF = torch.bfloat16
KEPT = float(C.KEPT)


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", C.DEPTHS)
@pytest.mark.parametrize("B", C.BATCHES)
def test_plan_kernel_equals_the_stable_partition(B, depth):
    t = C.table(depth, B)
    want = C.plan_ref(t)
    # a contiguous table
    dp = torch.from_numpy(t).to(DEV)
    plan = torch.full((depth, 1 + B), -1, dtype=torch.int32, device=DEV)
    ops.vit_droppath_plan(dp, depth, B, plan)
    # a column slice of a wider table (strided blocks and branches), as a launch train's share of the step's table is
    wide = torch.from_numpy(C.wide_table(depth, B)).to(DEV)
    sl = wide[:, :, C.MARGIN:C.MARGIN + B]
    assert not sl.is_contiguous() or B == wide.shape[2]
    plan_s = torch.full((depth, 1 + B), -1, dtype=torch.int32, device=DEV)
    ops.vit_droppath_plan(sl, depth, B, plan_s)
    torch.cuda.synchronize()
    assert np.array_equal(plan.cpu().numpy(), want)
    assert np.array_equal(plan_s.cpu().numpy(), want)


def test_plan_argument_errors():
    lib = _lib.lib()
    a = 0x10000
    assert lib.srhip_vit_droppath_plan(None, 10, 5, 2, 5, a, None) == -1
    assert lib.srhip_vit_droppath_plan(a, 10, 5, 2, 5, None, None) == -1
    assert lib.srhip_vit_droppath_plan(a, 10, 5, 0, 5, a, None) == -1
    assert lib.srhip_vit_droppath_plan(a, 10, 5, 2, 0, a, None) == -1


# ---- attention early exit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [257, 197])
@pytest.mark.parametrize("B", [2, 43, 86, 130])             # 6, 3, 2 and 1 head groups per image
def test_attention_leaves_a_dropped_image_with_zero_rows(N, B):
    g = torch.Generator().manual_seed(100 * N + B)
    xn = torch.randn(B * N, D, generator=g).to(BF).to(DEV)
    W = (torch.randn(3 * D, D, generator=g) * 0.05).to(BF).to(DEV)
    bias = (torch.randn(3 * D, generator=g) * 0.1).to(DEV)
    qkvx = torch.empty(B, 3 * D, dtype=BF, device=DEV) if N == 257 else None
    drop = torch.zeros(B, dtype=torch.bool)
    drop[0] = True                                           # the first image, every third, and the last one when there is room for a kept one
    drop[2::3] = True
    if B > 2:
        drop[B - 1] = True
    assert bool(drop.any()) and not bool(drop.all())
    osc = torch.full((B,), KEPT)
    osc[drop] = 0.0
    outs = []
    for scale_row in (osc, torch.full((B,), KEPT)):
        out = torch.full((B * N, D), float("nan"), dtype=BF, device=DEV)         # the poison
        assert bool(torch.isnan(out).all())
        ops.attn_block_fused(xn, W, bias, out, B, N, D, 6, 64 ** -0.5, qkv_extra=qkvx, out_scale=scale_row.to(DEV))
        outs.append(out.view(B, N * D))
    torch.cuda.synchronize()
    first, second = (o.view(torch.int16) for o in outs)
    drop = drop.to(DEV)
    assert not bool(torch.isnan(outs[0]).any()) and not bool(torch.isnan(outs[1]).any())       # no element keeps the poison
    assert torch.equal(first[~drop], second[~drop])          # kept images: the same bits
    assert bool((first[drop] == 0).all())                    # dropped images: +0 everywhere
    assert bool((second[drop] != 0).any(dim=1).all())        # (which the launch without the zeros did compute)


# ---- planned proj + MLP against the dense launch ---------------------------------------------------------------------------------------
def _operands(N, B, Hd, seed):
    g = torch.Generator().manual_seed(seed)
    def r(*s):
        # N(0, 1); the generator's Box-Muller draw is an exact 0 about once in 2^23 values (cos of a quarter turn): those become 1
        v = torch.randn(*s, generator=g)
        return torch.where(v == 0, torch.ones_like(v), v)
    M = B * N
    t = dict(x=r(M, D), ao=r(M, D).to(BF), Wp=(r(D, D) * 0.05).to(BF), bp=r(D) * 0.1, gam=torch.rand(D, generator=g) + 0.5, bet=r(D) * 0.2,
             W1=(r(Hd, D) * 0.05).to(BF), b1=r(Hd) * 0.1, W2=(r(D, Hd) * 0.03).to(BF), b2=r(D) * 0.1, gn=torch.rand(D, generator=g) + 0.5,
             bn=r(D) * 0.2, perm=torch.randperm(B, generator=g))
    # no exact zero among the inputs: the bit comparison below leaves nothing out
    for k in ("x", "ao", "Wp", "W1", "W2", "bp", "b1", "b2"):
        assert bool((t[k] != 0).all()), k
    return {k: v.to(DEV) for k, v in t.items()}


def _factors(t, B, n_mlp):
    """s1, s2 [B]: the MLP branch kept for n_mlp samples picked by a seeded permutation (not the first ones), the attention branch dropped
    for every other sample -- with 1 < n_mlp < B - 1 all four combinations occur; ao with the rows of attention-dropped samples zero."""
    perm = t["perm"]
    s2 = torch.zeros(B, device=DEV)
    s2[perm[:n_mlp]] = KEPT
    s1 = torch.full((B,), KEPT, device=DEV)
    s1[perm[0::2]] = 0.0
    return s1, s2


def _launch(t, x, x_out, s1, s2, N, M, Hd, ln, plan):
    ops.mlp_fused_proj(x, t["ao_z"], t["Wp"], t["bp"], s1, t["gam"], t["bet"], 1e-6, t["W1"], t["b1"], t["W2"], t["b2"], s2, N, M, D, Hd,
                       x_out=x_out, ln_next=ln, next_gamma=t["gn"] if ln is not None else None, next_beta=t["bn"] if ln is not None else None,
                       ao_scaled=True, plan_row=plan)


def _compare_with_dense(N, B, Hd, n_mlps, seed):
    t = _operands(N, B, Hd, seed)
    M = B * N
    combos = set()
    for n_mlp in n_mlps:
        s1, s2 = _factors(t, B, n_mlp)
        combos |= set(zip((s1 != 0).tolist(), (s2 != 0).tolist()))
        t["ao_z"] = (t["ao"].view(B, N * D) * (s1 != 0).to(BF)[:, None]).view(M, D).contiguous()     # as the attention launch leaves it
        dpt = torch.stack([s1, s2])[None].cpu().numpy()                   # [1, 2, B]
        plan = torch.from_numpy(C.plan_ref(dpt)[0]).to(DEV)
        assert int(plan[0]) == n_mlp
        # the reference: the dense launch
        want_x, want_ln = torch.empty(M, D, device=DEV), torch.empty(M, D, dtype=BF, device=DEV)
        _launch(t, t["x"], want_x, s1, s2, N, M, Hd, want_ln, None)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(want_x).all()) and bool((want_x != 0).all())
        for in_place in (False, True):
            for with_ln in (True, False):
                x = t["x"].clone()
                xo = x if in_place else torch.full((M, D), float("nan"), device=DEV)
                ln = torch.full((M, D), float("nan"), dtype=BF, device=DEV) if with_ln else None
                _launch(t, x, xo, s1, s2, N, M, Hd, ln, plan)
                torch.cuda.synchronize()
                what = (N, B, Hd, n_mlp, in_place, with_ln)
                assert torch.equal(xo.view(torch.int32), want_x.view(torch.int32)), what
                if with_ln:
                    assert torch.equal(ln.view(torch.int16), want_ln.view(torch.int16)), what
                if not in_place:
                    assert torch.equal(x, t["x"]), what
    return combos


@pytest.mark.parametrize("Hd", [128, 1536])
@pytest.mark.parametrize("N,B", [(257, 3), (197, 2), (5, 30), (1, 130)])
def test_planned_fused_mlp_equals_the_dense_launch(N, B, Hd):
    # n_mlp = 0 (the boundary on the launch's first tile edge: every tile light), 1 and B - 1 (inside a tile), B (nowhere: every tile heavy);
    # beyond those, half of the samples (all four factor combinations) and, at one row per sample, a boundary on an inner tile edge
    n_mlps = sorted({0, 1, B - 1, B} | ({B // 2} if B >= 4 else set()) | ({128} if N == 1 else set()))
    combos = _compare_with_dense(N, B, Hd, n_mlps, 1000 * N + B + Hd)
    if B >= 4:
        assert combos == {(False, False), (False, True), (True, False), (True, True)}


def test_planned_fused_mlp_with_heavy_and_light_tiles_in_one_workgroup():
    # 130 * 257 rows = 262 tiles on 256 workgroups: workgroups 0 .. 5 run a heavy tile (100 * 257 rows = tiles 0 .. 200) and then a light one
    _compare_with_dense(257, 130, 1536, [100], 77)


def test_planned_fused_mlp_argument_errors():
    N, B, Hd = 5, 6, 128
    t = _operands(N, B, Hd, 3)
    t["ao_z"] = t["ao"]
    M = B * N
    s1, s2 = _factors(t, B, 3)
    plan = torch.from_numpy(C.plan_ref(torch.stack([s1, s2])[None].cpu().numpy())[0]).to(DEV)
    x = t["x"].clone()
    with pytest.raises(RuntimeError, match="code -1"):        # M = 30 rows are no whole number of samples of 7 rows
        _launch(t, x, x, s1, s2, 7, M, Hd, None, plan)
    p = lambda v: v.data_ptr() if v is not None else None     # noqa: E731
    args = [p(x), p(x), p(t["ao"]), p(t["Wp"]), p(t["bp"]), p(s1), 1, p(t["gam"]), p(t["bet"]), 1e-6, p(t["W1"]), p(t["b1"]), p(t["W2"]), p(t["b2"]),
            p(s2), N, None, None, None, M, D, Hd]
    lib = _lib.lib()
    assert lib.srhip_mlp_fused_proj_planned(*args, None, B, None) == -1                       # no plan
    assert lib.srhip_mlp_fused_proj_planned(*args, p(plan), B + 1, None) == -1                # M != B * rows_per_sample
    assert lib.srhip_mlp_fused_proj_planned(*args, p(plan), 0, None) == -1
    torch.cuda.synchronize()
    assert torch.equal(x, t["x"])


# ---- the model -----------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(tag):
    if tag not in _MODELS:
        m = (vit.vit_small_patch16_224 if tag == "small_p16_224" else vit.vit_small_patch2_32)(num_classes=100, device=DEV)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_params(m.names_shapes, 5).items()})
        m.seed = 99
        _MODELS[tag] = m
    return _MODELS[tag]


def _spy(monkeypatch):
    """Records (M, row_pitch, planned) of every fused proj + MLP launch and the number of plan launches."""
    seen = {"mlp": [], "plans": 0}
    mlp0, plan0 = ops.mlp_fused_proj, ops.vit_droppath_plan

    def mlp(*a, **kw):
        seen["mlp"].append((a[14], kw.get("row_pitch"), kw.get("plan_row") is not None))
        return mlp0(*a, **kw)

    def plan(*a, **kw):
        seen["plans"] += 1
        return plan0(*a, **kw)

    monkeypatch.setattr(ops, "mlp_fused_proj", mlp)
    monkeypatch.setattr(ops, "vit_droppath_plan", plan)
    return seen


def _table(m, B):
    """A drawn table with dropped branches in several blocks, attention and MLP (seed 4 of the synthetic draw at B = 5 or 6)."""
    dpn = synth.synth_droppath(4, m.dp_probs_host.numpy(), B)
    for j in (0, 1):
        assert int(((dpn[:, j] == 0).sum(axis=1) > 0).sum()) >= 3
    return dpn


# B = 5 at 1024 rows: 5 * 257 rows take the fused chain by themselves; 5 * 197 = 985 rows take it as rows split off a launch of 6 images
@pytest.mark.parametrize("tag,kai", [("small_p2_32", None), ("small_p16_224", 6)])
@pytest.mark.parametrize("scatter", [False, True])
def test_backbone_outputs_do_not_change_with_the_switch(tag, kai, scatter, monkeypatch):
    monkeypatch.setattr(vit, "_FUSED_MLP_MIN_ROWS", 1024)
    m = _model(tag)
    cfg = m.cfg
    B, N = 5, cfg.num_tokens
    g = torch.Generator().manual_seed(11)
    img = torch.randn(B, cfg.in_chans, cfg.img_size, cfg.img_size, generator=g).to(DEV)
    dp = torch.from_numpy(_table(m, B)).to(DEV)
    rows = torch.tensor([6, 2, 9, 0, 4], device=DEV)
    seen = _spy(monkeypatch)
    res = {}
    for on in (False, True):
        monkeypatch.setattr(vit, "_SKIP_DROPPED_BRANCHES", on)
        seen["mlp"].clear()
        seen["plans"] = 0
        if scatter:
            out = (torch.full((10, cfg.num_classes), float("nan"), device=DEV), torch.full((10, D), float("nan"), device=DEV), rows)
            m.forward_features(img, None, dp, save=False, out=out, kernels_as_images=kai)
            res[on] = (out[0].clone(), out[1].clone())
        else:
            lg, ft, _ = m.forward_features(img, None, dp, save=False, kernels_as_images=kai)
            res[on] = (lg.clone(), ft.clone())
        torch.cuda.synchronize()
        # the path under test did run: one plan, 11 planned launches, the class-row launch of the last block as it was
        assert seen["plans"] == (1 if on else 0)
        assert seen["mlp"][:-1] == [(B * N, None, on)] * (cfg.depth - 1) and seen["mlp"][-1] == (B, N * D, False)
    lg0, ft0 = res[False]
    lg1, ft1 = res[True]
    sel = rows if scatter else slice(None)
    assert bool(torch.isfinite(lg0[sel]).all()) and bool(torch.isfinite(ft0[sel]).all())
    assert torch.equal(lg0[sel], lg1[sel]) and torch.equal(ft0[sel], ft1[sel])
    if scatter:
        assert torch.equal(torch.isnan(lg0), torch.isnan(lg1))


@pytest.mark.parametrize("tag", ["small_p2_32", "small_p16_224"])
def test_backbone_over_a_pass_prefix_tree_keeps_its_launches(tag, monkeypatch):
    monkeypatch.setattr(vit, "_FUSED_MLP_MIN_ROWS", 1024)
    m = _model(tag)
    cfg = m.cfg
    Bt, passes = 2, 3
    g = torch.Generator().manual_seed(5)
    img = torch.randn(Bt, cfg.in_chans, cfg.img_size, cfg.img_size, generator=g).to(DEV)
    cols_img = [j for _ in range(passes) for j in range(Bt)]
    n = len(cols_img)
    idx = torch.tensor(cols_img, dtype=torch.int32, device=DEV)
    dpn = _table(m, n)
    dp = torch.from_numpy(dpn).to(DEV)
    codes = _PassTree.codes_from_table(dpn)
    rows = torch.arange(n, device=DEV)
    seen = _spy(monkeypatch)
    res = {}
    for on in (False, True):
        monkeypatch.setattr(vit, "_SKIP_DROPPED_BRANCHES", on)
        seen["mlp"].clear()
        seen["plans"] = 0
        out = (torch.empty(n, cfg.num_classes, device=DEV), torch.empty(n, D, device=DEV), rows)
        tree = _PassTree(cols_img, codes, cfg.depth).upload(DEV, dp)
        m.forward_features(img, idx, tree.dp, save=False, out=out, tree=tree)
        torch.cuda.synchronize()
        assert seen["plans"] == 0 and not any(p for _, _, p in seen["mlp"])          # the tree path is unchanged
        res[on] = out
    # ... and both equal the unshared forward, which takes the plan
    monkeypatch.setattr(vit, "_SKIP_DROPPED_BRANCHES", True)
    seen["plans"] = 0
    out_u = (torch.empty(n, cfg.num_classes, device=DEV), torch.empty(n, D, device=DEV), rows)
    m.forward_features(img, idx, dp, save=False, out=out_u)
    torch.cuda.synchronize()
    assert seen["plans"] == 1
    assert bool(torch.isfinite(res[False][0]).all())
    for o in (res[True], out_u):
        assert torch.equal(res[False][0], o[0]) and torch.equal(res[False][1], o[1])
