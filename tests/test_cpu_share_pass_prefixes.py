"""share_pass_prefixes without a GPU: option parsing and validation, the host replica of the DropPath draw, and the invariants of the pass-prefix
tree (algorithms/srflexmatch.py _PassTree) on synthetic draws."""
import argparse
import struct

import numpy as np
import pytest


def _args(**kw):
    return argparse.Namespace(**kw)


def test_option_resolution(monkeypatch):
    from semireward_amd.algorithms.srflexmatch import share_pass_prefixes
    from semireward_amd.nets import bert, hubert, vit, wave2vec, wrn
    monkeypatch.delenv("SR_SHARE_PASS_PREFIXES", raising=False)
    V = vit.VisionTransformer
    assert share_pass_prefixes(_args(), V) is False                       # off by default
    assert share_pass_prefixes(_args(share_pass_prefixes=True), V) is True
    assert share_pass_prefixes(_args(share_pass_prefixes="1"), V) is True
    assert share_pass_prefixes(_args(share_pass_prefixes=0), V) is False
    monkeypatch.setenv("SR_SHARE_PASS_PREFIXES", "1")
    assert share_pass_prefixes(_args(), V) is True                        # the environment variable is the fallback ...
    assert share_pass_prefixes(_args(share_pass_prefixes=False), V) is False     # ... the key wins
    monkeypatch.setenv("SR_SHARE_PASS_PREFIXES", "0")
    assert share_pass_prefixes(_args(share_pass_prefixes="1"), V) is True
    assert share_pass_prefixes(_args(), V) is False
    for bad in ("2", "maybe", "", "bf16x3"):
        with pytest.raises(ValueError):
            share_pass_prefixes(_args(share_pass_prefixes=bad), V)
    monkeypatch.setenv("SR_SHARE_PASS_PREFIXES", "yes please")
    with pytest.raises(ValueError):
        share_pass_prefixes(_args(), V)
    monkeypatch.delenv("SR_SHARE_PASS_PREFIXES")
    for cls in (bert.ClassificationBert, wave2vec.ClassificationWave2Vec, hubert.ClassificationHubert, wrn.WideResNet):
        assert share_pass_prefixes(_args(), cls) is False                 # off: nothing to refuse
        with pytest.raises(NotImplementedError, match=cls.__name__):
            share_pass_prefixes(_args(share_pass_prefixes=True), cls)


def test_backbones_declare_the_sharing():
    from semireward_amd.nets import bert, hubert, surface, vit, wave2vec, wrn
    assert surface.ModuleSurface.pass_prefix_sharing is False
    assert vit.VisionTransformer.pass_prefix_sharing is True
    for cls in (bert.ClassificationBert, wave2vec.ClassificationWave2Vec, hubert.ClassificationHubert, wrn.WideResNet):
        assert cls.pass_prefix_sharing is False, cls.__name__


@pytest.mark.parametrize("algorithm", ["srflexmatch", "srpseudolabel"])
def test_validation_comes_before_device_work(monkeypatch, algorithm):
    """The algorithm constructor refuses a bad value, or the option on a backbone that cannot share, before the backbone is built."""
    from semireward_amd.algorithms import get_algorithm
    from semireward_amd.nets import bert, hubert, vit, wave2vec, wrn
    for v in ("SR_SHARE_PASS_PREFIXES", "SR_READ_ROWS_PRECISION", "SR_GRAD_ROWS_PRECISION"):
        monkeypatch.delenv(v, raising=False)
    built = []

    def builder_of(mod):
        def b(*a, **k):
            built.append(mod.__name__)
            raise AssertionError("the backbone must not be built")
        b.__module__ = mod.__name__
        return b
    with pytest.raises(ValueError):
        get_algorithm(_args(algorithm=algorithm, share_pass_prefixes="sometimes", num_classes=10), builder_of(vit))
    for mod, name in ((bert, "ClassificationBert"), (wave2vec, "ClassificationWave2Vec"), (hubert, "ClassificationHubert"), (wrn, "WideResNet")):
        with pytest.raises(NotImplementedError, match=name):
            get_algorithm(_args(algorithm=algorithm, share_pass_prefixes=True, num_classes=10), builder_of(mod))
    assert not built


def _keep_scalar(probs, depth, B, seed, cols):
    """droppath_fill_kernel written out one element at a time with Python integers and IEEE single rounding (struct)."""
    f32 = lambda v: struct.unpack("f", struct.pack("f", v))[0]            # noqa: E731
    M = (1 << 64) - 1
    out = np.zeros((depth, 2, len(cols)), dtype=bool)
    for l in range(depth):
        for j in range(2):
            for q, c in enumerate(cols):
                i = (2 * l + j) * B + int(c)
                z = (seed + 0x9E3779B97F4A7C15 * (i + 1)) & M
                z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
                z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
                z ^= z >> 31
                u = f32((z >> 40) / 16777216.0)
                p = f32(probs[l])
                out[l, j, q] = p <= 0 or u < f32(1.0 - p)
    return out


@pytest.mark.parametrize("seed,B", [(1, 7), ((5 << 32) + 3, 216), ((1 << 64) - 3, 40)])
def test_host_replica_matches_the_kernel_formula(seed, B):
    import torch
    from semireward_amd.nets.vit import droppath_keep_host
    probs = torch.linspace(0, 0.2, 12).numpy()
    cols = [int(c) for c in np.random.RandomState(B).permutation(B)]
    assert np.array_equal(droppath_keep_host(probs, 12, B, seed, cols=cols), _keep_scalar(probs, 12, B, seed, cols))
    assert np.array_equal(droppath_keep_host(probs, 12, B, seed), _keep_scalar(probs, 12, B, seed, list(range(B))))
    assert droppath_keep_host(probs, 12, B, seed)[0].all()              # block 0 never drops


def _slots_per_level(tree):
    """Each column's slot at every level, walked back from the last level through the parent maps."""
    out = [tree.col_node]
    for b in range(tree.depth - 1, 0, -1):
        out.append(tree.parent[b][out[-1]])
    return out[::-1]


def _check_tree(tree, imgs, codes):
    imgs = np.asarray(imgs)
    n, depth = imgs.shape[0], tree.depth
    assert np.array_equal(tree.uimg, np.asarray(list(dict.fromkeys(imgs.tolist()))))
    slots = _slots_per_level(tree)
    prev_n = tree.U
    for b in range(depth):
        s = slots[b]
        nb = tree.level_n[b]
        # the nodes partition the columns
        assert s.shape == (n,) and s.min() >= 0 and s.max() < nb and np.unique(s).shape[0] == nb
        # a node = one distinct (image, draws of the blocks <= b); independent count with Python tuples
        prefix = [(int(imgs[j]),) + (tuple(int(codes[k][j]) for k in range(b + 1)) if codes is not None else ()) for j in range(n)]
        assert nb == len(set(prefix))
        for v in range(nb):
            members = np.flatnonzero(s == v)
            assert len({prefix[j] for j in members}) == 1
            assert tree.rep[b][v] in members
        # parents: nodes keep the slot of their parent or are appended behind the previous level
        par = tree.parent[b]
        assert par.shape == (nb,) and nb >= prev_n
        assert np.array_equal(par[:prev_n], np.arange(prev_n))
        assert (par[prev_n:] < prev_n).all()
        prev_slot = slots[b - 1] if b > 0 else np.asarray([tree.uimg.tolist().index(i) for i in imgs.tolist()])
        assert np.array_equal(par[s], prev_slot)
        prev_n = nb
    assert tree.evals == sum(tree.level_n)
    cover = sorted(j for c in tree.node_cols() for j in c)
    assert cover == list(range(n))


def _cat_columns(nl, nu, K):
    Bt = nl + 2 * nu
    return [j for _ in range(K + 1) for j in range(Bt)]


@pytest.mark.parametrize("K,seed", [(8, 11), (11, 12), (3, 13)])
def test_tree_invariants_on_draws(K, seed):
    import torch
    from semireward_amd.algorithms.srflexmatch import _PassTree
    from semireward_amd.nets.vit import droppath_keep_host
    imgs = _cat_columns(8, 8, K)
    n = len(imgs)
    rs = np.random.RandomState(seed)
    keep = droppath_keep_host(torch.linspace(0, 0.2, 12).numpy(), 12, n, seed, cols=list(rs.permutation(n)))
    codes = _PassTree.codes_from_keep(keep)
    tree = _PassTree(imgs, codes, 12)
    _check_tree(tree, imgs, codes)
    assert tree.level_n[0] == tree.U == 24                               # block 0 (rate 0) never splits
    assert tree.evals < n * 12
    # a subset of the columns (a launch train), out of order
    sub = sorted(rs.choice(n, n // 2, replace=False).tolist(), key=lambda c: (c * 7) % n)
    t2 = _PassTree([imgs[c] for c in sub], codes[:, sub], 12)
    _check_tree(t2, [imgs[c] for c in sub], codes[:, sub])


def test_tree_without_drops_collapses_each_image():
    from semireward_amd.algorithms.srflexmatch import _PassTree
    imgs = _cat_columns(4, 4, 8)
    n = len(imgs)
    for codes in (None, np.full((12, n), 3, dtype=np.int64), _PassTree.codes_from_keep(np.ones((12, 2, n), dtype=bool))):
        t = _PassTree(imgs, codes, 12)
        assert t.level_n == [12] * 12 and t.evals == 12 * 12
        _check_tree(t, imgs, codes)
        assert np.array_equal(t.col_node, np.asarray(imgs))


def test_tree_with_distinct_draws_after_block0():
    from semireward_amd.algorithms.srflexmatch import _PassTree
    imgs = _cat_columns(4, 4, 8)
    n = len(imgs)
    dp = np.ones((12, 2, n), dtype=np.float32)
    dp[1:, 0, :] = 1.0 + np.arange(n, dtype=np.float32)[None, :] * 1e-3      # every column its own scale from block 1 on
    codes = _PassTree.codes_from_table(dp)
    t = _PassTree(imgs, codes, 12)
    _check_tree(t, imgs, codes)
    assert t.level_n[0] == 12 and t.level_n[1:] == [n] * 11
    # the table codes see bit patterns, not rounding: 1.0 and the float just above it differ
    dp2 = np.ones((12, 2, 2), dtype=np.float32)
    dp2[3, 1, 1] = np.nextafter(np.float32(1), np.float32(2))
    t2 = _PassTree([0, 0], _PassTree.codes_from_table(dp2), 12)
    assert t2.level_n == [1, 1, 1] + [2] * 9


def test_sharing_plans_keep_every_columns_kernels():
    """With the option on, the plan may move whole images from the deferred train into the read train (more rows shared inside a train).  That
    changes the trains' sizes, so it is only taken where every column keeps the kernels the default plan gives it (fused or unfused MLP, the tile
    kernel of every GEMM): over batch shapes, K, the tuner's shares, both read precisions and both run-time tile settings."""
    from semireward_amd import ops
    from semireward_amd.algorithms.srflexmatch import _DeferTuner, _Plan, _column_kernels, _plan_for_sharing
    from semireward_amd.nets import vit
    cfgs = {"s2_32": vit.VitConfig(img_size=32, patch_size=2, embed_dim=384, num_heads=6, num_classes=100),
            "s16_224": vit.VitConfig(img_size=224, patch_size=16, embed_dim=384, num_heads=6, num_classes=100),
            "b16_96": vit.VitConfig(img_size=96, patch_size=16, embed_dim=768, num_heads=12, num_classes=10)}
    fracs = sorted(set(_DeferTuner.CANDIDATES) | {0.45, 0.5, 0.555, 0.605}) + [None]
    taken, kept, cases = 0, 0, {}
    try:
        for grid in (ops.GEMM_SMALL_ALONE, ops.GEMM_SMALL_CONTENDED):
            ops.gemm_small_max_grid(grid)
            for tag, cfg in cfgs.items():
                for nl, nu in ((4, 4), (8, 8), (8, 16), (16, 16)):
                    for K in range(0, 13):
                        for f in fracs:
                            for split in (False, True):
                                mk = lambda w: _Plan.cat_passes(nl, nu, K, "cpu", defer_unread=True, rows_per_col=cfg.num_tokens,   # noqa: E731
                                                                defer_fraction=f, split_read=split, whole_images=w)
                                d, w = mk(False), mk(True)
                                p = _plan_for_sharing(d, w, cfg)
                                assert _column_kernels(p, cfg) == _column_kernels(d, cfg), (tag, nl, nu, K, f, split)
                                if p is w and w.host_cols != d.host_cols:
                                    taken += 1
                                elif p is d and w.host_cols != d.host_cols:
                                    kept += 1
                                cases[(grid, tag, nl, nu, K, f, split)] = p is w
    finally:
        ops.gemm_small_max_grid(ops.GEMM_SMALL_ALONE)
    # both outcomes occur: the whole-image moves where they keep the kernels (the headline: ViT-S/2, 8 / 8 / 8, K = 8, untuned share), the
    # column-wise moves where they would not (ViT-S/2, 8 / 8 / 8, K = 5, share 0.53: the read train stays unfused, the deferred one fused)
    assert taken > 0 and kept > 0, (taken, kept)
    assert cases[(ops.GEMM_SMALL_CONTENDED, "s2_32", 8, 8, 8, None, False)]
    assert not cases[(ops.GEMM_SMALL_CONTENDED, "s2_32", 8, 8, 5, 0.53, False)]
