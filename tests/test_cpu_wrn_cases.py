"""What tests/_wrn_cases.py promises, stated without a GPU: every convolution case reaches the template it names under srhip_wrn_conv_plan (all
nine direct and all six tile templates between them); the float64 references are right (torch's float64 conv2d, the adjoint identities, float64
autograd); the float32 restatement of every case passes the very functions the GPU tests hold the kernels to; the measured constants are what a
fresh measurement gives; the caps on the operand term and on the elements that may take either derivative hold for every case on the reference
alone; and each of twelve planted faults is rejected -- with the rel-norm the corresponding test of tests/test_gpu_wrn.py would have read."""
import numpy as np
import pytest
import torch

import _wrn_cases as WC
from semireward_amd import ops

IDS = lambda cs: [c["id"] for c in cs]          # noqa: E731


def test_every_convolution_case_reaches_the_template_it_names():
    seen = set()
    for c in WC.CONV_CASES:
        p = ops.wrn_conv_plan(*c["shape"])
        assert p.kernel == c["kernel"] and p.rounds == c["rounds"], (c["id"], p)
        seen.add(p.kernel)
    assert seen == {WC.DIRECT % (nt, ks) for nt in (1, 2, 4) for ks in (1, 2, 4)} | {WC.TILE % (nt, pg) for nt in (2, 4) for pg in (1, 2, 4)}
    for cid in WC.FALL_BACK:
        assert WC.conv_by_id(cid)["kernel"].startswith("wrn_conv_kernel<")
    assert any(c["rounds"] > 1 for c in WC.CONV_CASES)
    for k in ("wrn_conv_kernel", "wrn_conv_tile_kernel"):              # each kernel sees each form at least once
        cs = [c for c in WC.CONV_CASES if c["kernel"].startswith(k + "<")]
        assert {c["mode"] for c in cs} == {0, 1, 2, 3}
        for key, vals in (("resid", {False, True}), ("acc", {None, "zero", "add"}), ("publish", {False, True}), ("running", {False, True}),
                          ("ranks", {1, 2}), ("flip", {False, True})):
            assert {c[key] for c in cs} == vals, (k, key)


def test_float64_references():
    rng = np.random.default_rng(5)
    for B, H, W, C, Co, k, s in ((2, 7, 6, 3, 5, 3, 2), (1, 5, 9, 4, 2, 3, 1), (2, 6, 6, 3, 4, 1, 2)):
        a, Wf = rng.standard_normal((B, H, W, C)), rng.standard_normal((Co, C, k, k))
        want = torch.nn.functional.conv2d(torch.from_numpy(a).permute(0, 3, 1, 2), torch.from_numpy(Wf), stride=s, padding=k // 2)
        got = WC.conv_ref(a, WC.tap_major(Wf), k, s)
        assert np.abs(got - want.permute(0, 2, 3, 1).reshape(-1, Co).numpy()).max() < 1e-12
        # <col2im(d), a> == <d, im2col(a)>
        col = WC.im2col_ref(a, k, s)
        d = rng.standard_normal(col.shape)
        assert abs((WC.col2im_ref(d, B, H, W, C, k, s) * a).sum() - (d * col).sum()) < 1e-10
    # the convolution with the flipped filter is the adjoint of the forward one
    B, H, W, Ci, Co = 2, 5, 6, 3, 4
    Wf, dy = rng.standard_normal((Co, Ci, 3, 3)).astype(np.float32), rng.standard_normal((B, H, W, Co))
    Wq = WC.bf16_rne(Wf)
    flipped = WC.flip_ref(Wf, 64).double().numpy()[:, :9 * Co]
    adj = WC.col2im_ref(dy.reshape(-1, Co) @ WC.tap_major(Wq), B, H, W, Ci, 3, 1).reshape(-1, Ci)
    assert np.abs(WC.conv_ref(dy, flipped, 3, 1) - adj).max() < 1e-12
    x = rng.standard_normal((B, H, W, Ci))
    assert abs((adj * x.reshape(-1, Ci)).sum() - (WC.conv_ref(x, WC.tap_major(Wq), 3, 1) * dy.reshape(-1, Co)).sum()) < 1e-10
    # the BatchNorm + LeakyReLU backward against float64 autograd
    n, C = 50, 6
    x, dact, resid = (torch.from_numpy(rng.standard_normal((n, C))) for _ in range(3))
    g, b = torch.from_numpy(rng.standard_normal(C)).requires_grad_(), torch.from_numpy(rng.standard_normal(C)).requires_grad_()
    x.requires_grad_()
    mu, var = x.mean(0), x.var(0, unbiased=False)
    y = torch.nn.functional.leaky_relu(g * ((x - mu) / torch.sqrt(var + 1e-3)) + b, 0.1)
    (y * dact).sum().backward()
    isd = (1.0 / torch.sqrt(var + 1e-3)).detach().numpy()
    F = WC.bwd_ref(x.detach().numpy(), dact.numpy(), mu.detach().numpy(), isd, g.detach().numpy(), b.detach().numpy(), resid.numpy(), slope=0.1)
    assert np.abs(F["dx"] - (x.grad + resid).numpy()).max() < 1e-12
    assert np.abs(F["s2"] - g.grad.numpy()).max() < 1e-11 and np.abs(F["s1"] - b.grad.numpy()).max() < 1e-11
    # bn_finalize's statement: the fused variance of a constant channel is exactly zero, and one running step is two products and a sum
    mu, isd, rm, rv = WC.finalize_ref(np.array([7.5, 3.0]), np.array([5.625, 5.0]), 10, WC.EPS, (np.float32([1, 1]), np.float32([1, 1])))
    assert mu[0] == np.float32(0.75) and isd[0] == np.float32(1.0) / np.sqrt(np.float32(0.0) + WC.EPS)
    assert rv[1] == np.float32(np.float32(0.999) * np.float32(1)) + np.float32(np.float32(0.001) * np.float32(0.41 * 10 / 9))


def test_committed_constants_are_eight_times_the_measurement():
    got = dict(C_ACC=WC.measure_c_acc(), C_R=WC.measure_c_r(), C_SUM=WC.measure_c_sum(), C_BWD=WC.measure_c_bwd(), C_SGD=WC.measure_c_sgd())
    for k, v in got.items():
        committed, measured = getattr(WC, k), getattr(WC, k + "_MEASURED")
        print("%s: measured %.4f committed %.4f x 8 = %.3f" % (k, v, measured, committed))
        assert committed == 8.0 * measured and 4.0 * v <= committed <= 16.0 * v, k


# ---- the restatement of every case passes; the caps hold ------------------------------------------------------------------------------------
def check(H):
    assert all(v <= 1.0 for k, v in H.items() if k not in ("ulp1", "frac_w", "frac_amb")), H
    return H


@pytest.mark.parametrize("c", WC.CONV_CASES, ids=IDS(WC.CONV_CASES))
def test_convolution_restatement_and_caps(c):
    ex = WC.conv_expect(c["id"])
    print("%s: w > 0 on %.4f %% of the activation, %.2f %% of the outputs without an operand term" % (c["id"], 100 * ex["frac_w"], 100 * ex["frac_clean"]))
    assert ex["frac_w"] <= 0.01 and ex["frac_clean"] >= 0.80
    for reverse in ((False, True) if c["id"] not in WC.LARGE else (False,)):
        L = WC.ConvLaunch(c, "cpu")
        WC.conv_restate(L, reverse=reverse)
        H = check(WC.conv_verify(L, ex))
        assert H["ulp1"] == 0
        print(c["id"], "reverse" if reverse else "forward", {k: round(v, 4) for k, v in H.items()})


@pytest.mark.parametrize("cls,c,kw", [(cls, c, kw) for cls, cs, kw in (
    (WC.HeadLaunch, WC.HEAD_CASES, {}), (WC.BnLaunch, WC.BN_CASES, {}), (WC.BwdLaunch, WC.BWD_CASES, {}), (WC.ImLaunch, WC.IM_CASES, {}),
    (WC.WeightLaunch, WC.WEIGHT_TABLES, {}), (WC.WeightLaunch, WC.FLIP_TABLES, dict(flip=True)), (WC.FcLaunch, WC.FC_CASES, {}),
    (WC.PoolLaunch, WC.POOL_CASES, {}), (WC.SgdLaunch, WC.SGD_CASES, {})) for c in cs], ids=lambda v: v["id"] if isinstance(v, dict) and "id" in v else "")
def test_restatement_of_the_other_kernels_and_caps(cls, c, kw):
    L = cls(c, "cpu", **kw)
    L.restate()
    H = check(L.verify())
    print(c["id"], {k: round(v, 4) for k, v in H.items()})
    assert H.get("frac_w", 0.0) <= 0.01 and H.get("frac_amb", 0.0) <= 1e-3 and H.get("ulp1", 0) == 0


# ---- planted faults -----------------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def rejected(verify, what):
    with pytest.raises(AssertionError) as e:
        verify()
    print("%s -> %s" % (what, str(e.value)[:260]))


CONV_FAULTS = (     # fault, case, the rel-norm threshold of the corresponding test of tests/test_gpu_wrn.py
    ("left_border_wraps", "t22-tw16-16x48", 3e-6),                  # test_fused_conv_equals_the_unfused_chain (both sides share the tap arithmetic)
    ("last_tap_missing_on_one_tile", "d11-rounds2-64p", 3e-6),
    ("lane_stores_to_neighbour_pixel", "d11-rounds2-64p", 3e-6),
    ("resid_skipped_on_ragged_tile", "d11-ragged35", 3e-6),
    ("pass1_reads_pass0_acc", "d11-rounds2-64p", None),             # test_passes_sharing_their_launches...: bit-equality of two paths that share the indexing
    ("running_moved_by_pass1", "d11-rounds2-64p", None),
    ("acc_out_overwritten", "d21", None),                           # (no test read acc_out: the statistics were checked through the next layer)
    ("flip_no_rotation", "d12-flip", 4e-2),                         # the network-gradient check against autograd
)


@pytest.mark.parametrize("fault,cid,threshold", CONV_FAULTS, ids=[f[0] for f in CONV_FAULTS])
def test_checker_rejects_each_planted_convolution_fault(fault, cid, threshold):
    c = WC.conv_by_id(cid)
    ex = WC.conv_expect(cid)
    L = WC.ConvLaunch(c, "cpu")
    WC.conv_restate(L)
    check(WC.conv_verify(L, ex))
    good = L.y.numpy().copy()
    L = WC.ConvLaunch(c, "cpu")
    WC.conv_restate(L, fault=fault)
    rejected(lambda: WC.conv_verify(L, ex), fault)
    r = rel(L.y.numpy(), good)
    if threshold is None:
        print("%s at %s: rel-norm of y %.3e; no kernel-level test read what this fault changes" % (fault, cid, r))
    else:
        print("%s at %s: rel-norm of y against the faithful restatement %.3e; the threshold %.0e of the existing test would have %s it" % (
            fault, cid, r, threshold, "PASSED" if r < threshold else "rejected"))


def test_checker_rejects_each_planted_fault_of_the_other_kernels():
    # SyncBatchNorm apply dividing by this rank's rows; the derivative at the kink taken as 1
    for fault, cid in (("rows_instead_of_rows_total", "bwd-c16-2ranks"), ("kink_derivative_one", "bwd-c16-r300")):
        c = next(c for c in WC.BWD_CASES if c["id"] == cid)
        G = WC.BwdLaunch(c, "cpu")
        G.restate()
        check(G.verify())
        L = WC.BwdLaunch(c, "cpu")
        L.restate(fault=fault)
        rejected(L.verify, fault)
        r = max(rel(L.A[k].numpy(), G.A[k].numpy()) for k in ("dx0", "dg0", "db0"))
        print("%s at %s: largest rel-norm of dx / dgamma / dbeta %.3e; the threshold 5e-6 of test_batchnorm_leakyrelu would have %s it%s" % (
            fault, cid, r, "PASSED" if r < 5e-6 else "rejected",
            " (that test has one rank and no channel on the kink: it cannot plant either)"))
    # weight decay applied to the first element of the flag-0 chunk
    c = next(c for c in WC.SGD_CASES if c["id"] == "sgd-later")
    G = WC.SgdLaunch(c, "cpu")
    G.restate()
    check(G.verify())
    L = WC.SgdLaunch(c, "cpu")
    L.restate(fault="wd_on_flag0_first_element")
    rejected(L.verify, "wd_on_flag0_first_element")
    print("wd_on_flag0_first_element: rel-norm of p %.3e (one element of %d; no test called srhip_sgd_flat directly)" % (rel(L.A["p"].numpy(), G.A["p"].numpy()), L.n))
    # col2im taking a tap from ty / stride when ty is no multiple of the stride
    c = next(c for c in WC.IM_CASES if c["id"] == "im-7x7-c16-k3-s2")
    G = WC.ImLaunch(c, "cpu")
    G.restate()
    check(G.verify())
    L = WC.ImLaunch(c, "cpu")
    L.restate(fault="ignores_ty_mod_stride")
    rejected(L.verify, "ignores_ty_mod_stride")
    r = rel(L.A["dact"].numpy(), G.A["dact"].numpy())
    print("ignores_ty_mod_stride: rel-norm of dact %.3e; the threshold 1e-5 of test_conv_building_blocks would have %s it" % (r, "PASSED" if r < 1e-5 else "rejected"))
