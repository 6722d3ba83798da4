"""Host side of the WideResNet steps of SRFixMatch / SRFlexMatch / SRFreeMatch / SRSoftMatch: the reference traces
(tests/golden/sr*match_wrn_trace.npz, tools/gen_wrn_strong_traces.py) as fixtures, the refusal of use_cat False, the authored yaml."""
import argparse
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGOS = ["srfixmatch", "srflexmatch", "srfreematch", "srsoftmatch"]


@pytest.mark.parametrize("algo", ALGOS)
def test_fixture_loads_with_margins_and_call_counts(golden, algo):
    """Every step of the trace made K + 1 model() calls, each of which moved num_batches_tracked; K = 0, the stage-1 rewarder update, K > 0 and
    an N_k update are covered; and no hard decision of the reference sits within 1e-2 of its threshold (the margin TRACE_PL_WRN has), so an
    engine with bf16 convolution operands has to reproduce every mask."""
    g = golden(algo + "_wrn_trace")
    its = [int(i) for i in g["meta/its"]]
    start, N_k, Bu = int(g["meta/start_timing"]), int(g["meta/N_k"]), int(g["meta/Bu"])
    assert its == sorted(its) and its[0] == 0
    nbt, Ks, upd = 0, [], []
    for it in its:
        p = "it%d" % it
        K = int(g[p + "/K"])
        assert K == (0 if it <= start else int(max(8, 1 + int(g["meta/num_train_iter"]) / it)))
        assert int(g[p + "/calls"]) == K + 1
        nbt += K + 1
        assert int(g[p + "/num_batches_tracked"]) == nbt
        assert g[p + "/masks"].shape == g[p + "/mask_probs"].shape == g[p + "/mask_thr"].shape == (K + 1, Bu)
        if algo != "srsoftmatch":
            assert float(np.abs(g[p + "/mask_probs"] - g[p + "/mask_thr"]).min()) > 1e-2, p
            assert set(np.unique(g[p + "/masks"])) <= {0.0, 1.0}
        if algo == "srflexmatch":
            assert float(np.abs(g[p + "/mask_probs"] - float(g["meta/p_cutoff"])).min()) > 1e-2, p
        used = g[p + "/masks"] > 0               # rows whose pseudo label reaches the loss: the argmax is a hard decision too
        assert g[p + "/label_gap"].shape == (K + 1, Bu) and (not used.any() or float(g[p + "/label_gap"][used].min()) > 1e-2), p
        for k in ("sup_loss", "unsup_loss", "total_loss"):
            assert np.isfinite(float(g[p + "/log/" + k]))
        assert any(k.endswith("running_var") for k in g.keys(p + "/buf/"))
        # the reference's own run with bf16-rounded convolution operands (CPU) stays inside the GPU test's bounds at this iteration
        n, d = its.index(it), (lambda k: float(g["bf16dev/" + p + "/" + k]))
        assert d("masks") <= (6e-2 if algo == "srsoftmatch" else 0.0), p
        for k in ("feat/x_lb", "feat/x_ulb_w", "feat/x_ulb_s", "running_mean"):
            assert d(k) < 5e-2 + 3e-2 * n, (p, k, d(k))
        assert d("running_var") < 1e-3
        for k in ("sup_loss", "unsup_loss", "total_loss"):
            assert d("log/" + k) <= max(5e-3, 6e-2 * abs(float(g[p + "/log/" + k]))), (p, k, d("log/" + k))
        Ks.append(K); upd.append(int(g[p + "/rewarder_updated"]))
    assert 0 in Ks and max(Ks) > 0 and float(g["bf16dev/param"]) < 3e-2
    assert upd[its.index(1)] == 1 and upd[its.index(0)] == 0                       # stage 1 (0 < it < start_timing)
    assert any(u for it, u in zip(its, upd) if it > start and it % N_k == 0)       # an N_k update
    if algo != "srsoftmatch":
        allm = np.concatenate([g["it%d/masks" % it].ravel() for it in its])
        assert 0.15 < float(allm.mean()) < 0.95                                    # selections and rejections
    else:
        allm = np.concatenate([g["it%d/masks" % it].ravel() for it in its])
        assert float(allm.min()) < 0.9 and float(allm.max()) <= 1.0                # the weight is exercised


@pytest.mark.parametrize("algo", ALGOS)
def test_use_cat_false_is_refused_on_a_batchnorm_backbone(algo):
    """Three model() calls per pass would be three BatchNorm statistics groups per pass: a ValueError that names the key, before any device work."""
    from semireward_amd.algorithms import get_algorithm
    from semireward_amd.nets import wrn
    args = argparse.Namespace(algorithm=algo, num_classes=10, use_cat=False, num_train_iter=10, epoch=1, ema_m=0.0, gpu=0, rank=0, world_size=1,
                              distributed=False)
    with pytest.raises(ValueError, match="use_cat"):
        get_algorithm(args, wrn.wrn_tiny_test)


def test_authored_yaml_resolves():
    from semireward_amd import config
    from semireward_amd.algorithms import ALGORITHMS
    a = config.get_config(os.path.join(ROOT, "configs", "classic_cv", "srflexmatch_cifar100_400_wrn_28_2.yaml"))
    assert (a.algorithm, a.net, a.num_classes, a.batch_size, a.uratio, a.use_cat, a.optim) == ("srflexmatch", "wrn_28_2", 100, 64, 7, True, "SGD")
    assert (a.feature_dim, a.N_k, a.sr_lr, a.sr_ema, a.sr_ema_m, a.start_timing) == (128, 10, 5e-4, False, 0.99, 100000)
    assert a.thresh_warmup is True and a.p_cutoff == 0.95 and a.ema_m == 0.999 and a.algorithm in ALGORITHMS
