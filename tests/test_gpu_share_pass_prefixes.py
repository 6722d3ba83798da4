"""share_pass_prefixes on the GPU: the host replica of the DropPath draw against the device table, forward_features over a pass-prefix tree
against the unshared forward (bit for bit: logits and features of every column), whole training steps with the option on against the same
steps with it off, the block evaluations the trees save, and the StepGraph staying eager."""
import argparse

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_stepgraph as TG                                           # noqa: E402  (the step helpers)
from semireward_amd import ops                                            # noqa: E402
from semireward_amd.algorithms import get_algorithm, srflexmatch as SF   # noqa: E402
from semireward_amd.algorithms.srflexmatch import _PassTree               # noqa: E402
from semireward_amd.nets import vit                                       # noqa: E402
from semireward_amd.utils import synth                                    # noqa: E402

DEV = "cuda:0"


@pytest.mark.parametrize("B,seed", [(7, 1), (216, (4321 << 32) + 17), (500, (1 << 63) + 5)])
def test_host_replica_equals_droppath_fill(B, seed):
    probs_h = torch.linspace(0, 0.2, 12)
    probs = probs_h.to(DEV)
    dp = torch.empty(12, 2, B, device=DEV)
    ops.droppath_fill(dp, probs, 12, B, seed)
    assert np.array_equal(dp.cpu().numpy() != 0, vit.droppath_keep_host(probs_h.numpy(), 12, B, seed))
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(B))
    dpc = torch.empty(12, 2, B, device=DEV)
    ops.droppath_fill(dpc, probs, 12, B, seed, cols=perm.to(DEV))
    assert np.array_equal(dpc.cpu().numpy() != 0, vit.droppath_keep_host(probs_h.numpy(), 12, B, seed, cols=perm.tolist()))


def _model(tag):
    if tag == "tiny":
        m = vit.vit_tiny_test(num_classes=10, device=DEV)
    elif tag == "small_p16_224":
        m = vit.vit_small_patch16_224(num_classes=100, device=DEV)
    elif tag == "base_p16_96":
        m = vit.vit_base_patch16_96(num_classes=10, device=DEV)
    else:
        m = vit.vit_small_patch2_32(num_classes=100, device=DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_params(m.names_shapes, 5).items()})
    m.seed = 99
    return m


@pytest.mark.parametrize("tag", ["tiny", "small_p2_32", "small_p16_224", "base_p16_96"])
@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("passes", [9, 12])
@pytest.mark.parametrize("draws", ["make_droppath", "synth"])
def test_forward_over_a_tree_equals_the_unshared_forward(tag, precision, passes, draws):
    m = _model(tag)
    cfg = m.cfg
    Bt = 8 if tag != "tiny" else 6
    g = torch.Generator().manual_seed(passes)
    img = torch.randn(Bt + 3, cfg.in_chans, cfg.img_size, cfg.img_size, generator=g).to(DEV)
    cols_img = [3 + j for _ in range(passes) for j in range(Bt)]              # every pass forwards the same images (3 unused ones in front)
    n = len(cols_img)
    img_index = torch.tensor(cols_img, dtype=torch.int32, device=DEV)
    if draws == "make_droppath":
        perm = torch.randperm(n, generator=g)
        dp = m.make_droppath(n, cols=perm.to(DEV))
        codes = _PassTree.codes_from_keep(vit.droppath_keep_host(m.dp_probs_host.numpy(), cfg.depth, n, m.last_droppath_seed, cols=perm.tolist()))
    else:
        dpn = synth.synth_droppath(passes, m.dp_probs_host.numpy(), n)
        dp = torch.from_numpy(dpn).to(DEV)
        codes = _PassTree.codes_from_table(dpn)
    C, D = cfg.num_classes, cfg.embed_dim
    rows = (torch.randperm(n, generator=g) + 5).to(DEV)                       # the step's rows of the columns, scattered
    out0 = (torch.full((n + 5, C), float("nan"), device=DEV), torch.full((n + 5, D), float("nan"), device=DEV), rows)
    out1 = (torch.full((n + 5, C), float("nan"), device=DEV), torch.full((n + 5, D), float("nan"), device=DEV), rows)
    kw = dict(precision=precision)
    m.forward_features(img, img_index, dp, save=False, out=out0, **kw)
    tree = _PassTree(cols_img, codes, cfg.depth).upload(DEV, dp)
    m.forward_features(img, img_index, tree.dp, save=False, out=out1, tree=tree, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out0[0][rows], out1[0][rows]) and torch.equal(out0[1][rows], out1[1][rows])
    assert bool(torch.isnan(out1[0][:5]).all())                               # rows outside the train untouched
    assert tree.launched == tree.level_n and tree.U == Bt
    assert tree.evals < n * cfg.depth or cfg.depth < 3
    print("TREE %s %s passes=%d %s: %d of %d block evaluations, per block %s" % (tag, precision, passes, draws, tree.evals, n * cfg.depth,
                                                                                 tree.level_n))


def test_forward_over_a_tree_keeps_the_kernels_of_a_larger_launch():
    """kernels_as_images (the unread columns moved into the read launch): the tree forward pins the same kernels as the unshared one."""
    m = _model("small_p2_32")
    cfg = m.cfg
    g = torch.Generator().manual_seed(3)
    img = torch.randn(8, 3, 32, 32, generator=g).to(DEV)
    cols_img = [j for _ in range(6) for j in range(8)]                       # 48 images: unfused on their own, fused as part of 72
    n = len(cols_img)
    idx = torch.tensor(cols_img, dtype=torch.int32, device=DEV)
    dp = m.make_droppath(n)
    codes = _PassTree.codes_from_keep(vit.droppath_keep_host(m.dp_probs_host.numpy(), 12, n, m.last_droppath_seed))
    rows = torch.arange(n, device=DEV)
    for kai in (None, 72):
        o0 = (torch.empty(n, 100, device=DEV), torch.empty(n, 384, device=DEV), rows)
        o1 = (torch.empty(n, 100, device=DEV), torch.empty(n, 384, device=DEV), rows)
        m.forward_features(img, idx, dp, save=False, out=o0, kernels_as_images=kai, buftag="m")
        tree = _PassTree(cols_img, codes, 12).upload(DEV, dp)
        m.forward_features(img, idx, tree.dp, save=False, out=o1, kernels_as_images=kai, buftag="m", tree=tree)
        torch.cuda.synchronize()
        assert torch.equal(o0[0], o1[0]) and torch.equal(o0[1], o1[1]), kai


NS = dict(TG.NSa)
ALGS = {
    "srflexmatch": {},
    "srfixmatch": dict(algorithm="srfixmatch"),
    "srfreematch": dict(algorithm="srfreematch", ema_p=0.9, use_quantile=True, clip_thresh=False, ent_loss_ratio=0.01),
    "srsoftmatch": dict(algorithm="srsoftmatch", dist_align=True, dist_uniform=True, ema_p=0.9, n_sigma=2, per_class=False),
    "srpseudolabel": dict(algorithm="srpseudolabel", unsup_warm_up=0.4),
}


def _alg(name, share, monkeypatch, precision="bf16", it0=30008, K=None, defer_share=None):
    monkeypatch.setattr(SF, "_DEFER_AUTOTUNE", False)
    d = dict(NS)
    d.update(ALGS[name])
    alg = get_algorithm(argparse.Namespace(**d, share_pass_prefixes=share, read_rows_precision=precision), vit.vit_small_patch2_32)
    assert alg.share_pass_prefixes is share
    alg.model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_params(alg.model.names_shapes, 0).items()})
    alg.model.seed = 4321
    alg.it = it0
    alg.optimizer.sched_step = it0
    alg.optimizer.step_count = 7
    if K is not None:
        alg.sr_decay = lambda: K                                              # a regime of another K (early in a run sr_decay() walks through them)
    alg.defer_share = defer_share                                             # a share the tuner may choose (None: the untuned rule)
    rec = []
    orig = alg._forward_plan

    def recorded(*a, **k):
        r = orig(*a, **k)
        rec.append(r[:2])
        return r
    alg._forward_plan = recorded
    alg._rec = rec
    return alg


def _batch(alg, i):
    import inspect
    b = {k: torch.from_numpy(v) for k, v in synth.synth_batch(700 + i, 8, 8, 32, 100, 50000).items()}
    keep = set(inspect.signature(alg.train_step).parameters)
    return alg.process_batch(**{k: v for k, v in b.items() if k in keep})


def _step(alg, batch):
    alg.trace = {}
    alg._rec.clear()
    out, log = alg.train_step(**batch)
    alg.out_dict, alg.log_dict = out, log
    grad = alg.model.grad.clone()                                            # the backbone gradient of the step, before the update zeroes it
    alg.hooks_dict["ParamUpdateHook"].after_train_step(alg)
    alg.it += 1
    torch.cuda.synchronize()
    L, F = alg._rec[-1]
    tr = alg.trace or {}
    res = dict(L=L.clone(), F=F.clone(), flat=alg.model.flat.clone(), grad=grad)
    for k in ("max_probs", "pseudo", "reward", "mask2"):
        if tr.get(k) is not None:
            res[k] = tr[k].clone()
    if tr.get("masks") is not None:
        res["masks"] = torch.stack([x.reshape(-1) for x in tr["masks"]]).clone()
    h = alg.hooks_dict["MaskingHook"]
    for k in ("selected_label", "classwise_acc"):
        if hasattr(h, k):
            res[k] = getattr(h, k).clone()
    return res


def _same_steps(name, monkeypatch, nsteps, precision="bf16", **kw):
    """Option off (twice: the bound the default path meets against itself) and on, every step from the same state."""
    a0, a0b, a1 = (_alg(name, s, monkeypatch, precision, **kw) for s in (False, False, True))
    for i in range(nsteps):
        before = a0.model.flat.clone()
        batch = _batch(a0, i)
        x, xb, y = _step(a0, batch), _step(a0b, batch), _step(a1, batch)
        upd = float((x["flat"] - before).abs().max())
        ref_max = float((x["flat"] - xb["flat"]).abs().max())
        assert torch.equal(x["L"], y["L"]) and torch.equal(x["F"], y["F"]), (name, i)       # every column, bit for bit
        for k in x:
            if k not in ("L", "F", "flat", "grad"):
                assert torch.equal(x[k], y[k]), (name, i, k)
        # the backward's inputs are bit for bit the same: its gradient differs from the default one by no more than a second default run's does
        # (fp32 atomics reorder the weight-gradient sums; 1e-6 rel-L2 floor for a pair of default runs that happen to agree exactly)
        rel = lambda a, b: float((a - b).double().norm() / b.double().norm())      # noqa: E731
        g_ref = rel(xb["grad"], x["grad"])
        assert rel(y["grad"], x["grad"]) <= max(4.0 * g_ref, 1e-6), (name, i, rel(y["grad"], x["grad"]), g_ref)
        # parameters after one AdamW step: the StepGraph test's bound (a gradient within round-off of zero may flip the sign of its update)
        d = float((x["flat"] - y["flat"]).abs().max())
        assert d <= max(2.1 * upd, 2.0 * ref_max), (name, i, d, upd, ref_max)
        assert float((x["flat"] - y["flat"]).abs().mean()) <= 1e-2 * upd, (name, i)
        assert len(a1.pass_trees) >= 1 and not a0.pass_trees
        if i + 1 < nsteps:                                                   # (the FlexMatch table helper: multi-step runs are SRFlexMatch)
            for a in (a0b, a1):
                TG._copy_state(a, a0)
    return a1


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_srflexmatch_steps_with_and_without_sharing(precision, monkeypatch):
    _same_steps("srflexmatch", monkeypatch, 3, precision)


@pytest.mark.parametrize("K,share", [(5, 0.53), (8, 0.58), (12, 0.42)])
def test_srflexmatch_steps_at_tuned_shares(K, share, monkeypatch):
    """Shares and K where moving whole images between the trains would take a train across the fused MLP's launch size (K = 5, 0.53): the
    sharing plan keeps the default plan's kernels there, and every column stays bit for bit the same."""
    a1 = _same_steps("srflexmatch", monkeypatch, 1, K=K, defer_share=share)
    assert a1.trace["K"] == K


@pytest.mark.parametrize("name", ["srfixmatch", "srfreematch", "srsoftmatch", "srpseudolabel"])
def test_other_algorithms_one_step(name, monkeypatch):
    _same_steps(name, monkeypatch, 1)


def test_block_evaluations_of_the_reference_plan(monkeypatch):
    """configs[1] size (8 / 8 / 8, K = 8): the blocks actually launched are the trees' count, at most 0.6 of the unshared launches'."""
    a = _alg("srflexmatch", True, monkeypatch)
    _step(a, _batch(a, 0))
    assert a.trace["K"] == 8
    launched = sum(sum(t.launched) for _, t in a.pass_trees)
    evals = sum(t.evals for _, t in a.pass_trees)
    full = sum(t.n * t.depth for _, t in a.pass_trees)
    print("BLOCK_EVALS trains %s: %d of %d (%.3f); per train %s" % ([nm for nm, _ in a.pass_trees], evals, full, evals / full,
                                                                   [(nm, t.n, t.level_n) for nm, t in a.pass_trees]))
    assert launched == evals
    assert evals <= 0.6 * full


def test_stepgraph_stays_eager_with_sharing(monkeypatch):
    it0, n = 30008, 4
    a0, _ = TG._make(False, it0, monkeypatch)
    monkeypatch.setenv("SR_SHARE_PASS_PREFIXES", "1")
    a1, sg = TG._make(True, it0, monkeypatch)
    assert a1.share_pass_prefixes and not a0.share_pass_prefixes
    batches = [a0.process_batch(**{k: torch.from_numpy(v) for k, v in synth.synth_batch(700 + i, 8, 8, 32, 100, 50000).items()}) for i in range(n)]
    for i in range(n):
        before = a0.model.flat.clone()
        x, y = TG._one_step(a0, None, batches[i]), TG._one_step(a1, sg, batches[i])
        upd = float((x["flat"] - before).abs().max())
        assert torch.equal(x["feat"], y["feat"]), i
        np.testing.assert_allclose(y["loss"], x["loss"], rtol=1e-5, atol=1e-6, err_msg="step %d" % i)
        assert torch.equal(x["sel"], y["sel"]) and torch.equal(x["acc"], y["acc"]), i
        assert float((x["flat"] - y["flat"]).abs().max()) <= 2.1 * upd, i
        assert float((x["flat"] - y["flat"]).abs().mean()) <= 1e-2 * upd, i
        TG._copy_state(a1, a0)
    assert sg.replays == 0 and not sg.graphs and sg.eager_steps == n
