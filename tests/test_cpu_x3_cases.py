"""tests/_x3_cases.py checked on the CPU: the checker accepts the float32 restatement of every case (in the kernels' chunk order and in
reverse: at a quarter of the bound or less wherever the bound carries a measured constant, inside it where it is the exact residue term),
rejects the same restatement with the lo planes zeroed, rejects each of the eighteen planted
faults; the constants are measured afresh; the six srhip_*_x3 entry points and srhip_layernorm_fwd_f32 refuse what they must, before any
launch; the float64 backward formula equals float64 autograd of the forward; and what the old whole-tensor thresholds make of every fault."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import _x3_cases as X

F = np.float32


# ---- (b) the restatement is accepted with room, (a) the bf16-operand product is rejected --------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in X.GEMM_CASES])
def test_gemm_restatement_accepted_and_bf16_operands_rejected(cid):
    c = X.GEMM_BY_ID[cid]
    for rev in (False, True):
        L = X.GemmLaunch(c, "cpu")
        L.restate(reverse=rev)
        r = L.verify()
        spec = max(v for n, v in L.ratios.items() if not n.endswith(":true"))
        print("headroom %s restatement%s %.3f (statements with a constant), %.3f (against a.b)" % (cid, " reversed" if rev else "", spec, r))
        assert spec <= 0.25 and r <= 1.0, (cid, rev, L.ratios)
    L = X.GemmLaunch(c, "cpu")
    L.restate(mode="bf16")
    with pytest.raises(AssertionError):
        L.verify()


@pytest.mark.parametrize("lid", [ln["id"] for ln in X.TN_LAUNCHES])
def test_tn_restatement_accepted_and_bf16_operands_rejected(lid):
    for rev in (False, True):
        L = X.TnLaunch(X.TN_BY_ID[lid], "cpu")
        L.restate(reverse=rev)
        r = L.verify()
        spec = max(v for n, v in L.ratios.items() if not n.endswith(":true"))
        print("headroom %s restatement%s %.3f (statements with a constant), %.3f (against a.b)" % (lid, " reversed" if rev else "", spec, r))
        assert spec <= 0.25 and r <= 1.0, (lid, rev, L.ratios)
    L = X.TnLaunch(X.TN_BY_ID[lid], "cpu")
    L.restate(mode="bf16")
    with pytest.raises(AssertionError):
        L.verify()


@pytest.mark.parametrize("cid", [c["id"] for c in X.LN_CASES])
def test_layernorm_restatement_accepted(cid):
    for order in ("tree", "pair"):
        L = X.LnLaunch(X.LN_BY_ID[cid], "cpu")
        L.restate(order)
        r = L.verify()
        print("headroom %s restatement %s %.3f" % (cid, order, r))
        assert r <= 0.25, (cid, order, r)


@pytest.mark.parametrize("cid", [c["id"] for c in X.ATTN_CASES])
def test_attention_restatement_accepted_and_bf16_operands_rejected(cid):
    ref = X.attn_reference(cid)
    c = ref["c"]
    least, margin = X.decisive_mass(c, ref["inp"])
    assert least >= X.DECISIVE, (cid, least)                       # every key is decisive for some query
    assert c["N"] < 4 or margin >= 40.0, (cid, margin)             # the row maximum of the spiked queries lies in the last valid block
    for b, h, qa, s1, qb, s2 in ref["inp"]["spikes"]:
        assert s2 >= (c["N"] - 1) // 16 * 16
    for rev in (False, True):
        r = X.restate_attn(cid, mode="f32", reverse=rev)          # the fp32 operations alone, against the fp32 terms alone
        rf = X.verify_fwd(cid, r["out"], r["lse"], ref["fwd"], f32_only=True)
        rb = X.verify_bwd(cid, r, ref["bwd"], f32_only=True)
        assert max(rf, rb) <= 0.25, (cid, rev, rf, rb)
        r = X.restate_attn(cid, reverse=rev)
        xf = X.verify_fwd(cid, r["out"], r["lse"], ref["fwd"])
        xb = X.verify_bwd(cid, r, ref["bwd"])
        print("headroom %s restatement%s fp32 terms: fwd %.3f bwd %.3f; whole bound: fwd %.3f bwd %.3f" % (cid, " reversed" if rev else "", rf, rb, xf, xb))
        assert xf <= min(1.0, 1.5 * X.ATT_X3_RESTATED[0]) and xb <= min(1.0, 1.5 * X.ATT_X3_RESTATED[1]), (cid, rev, xf, xb)
    if c["N"] >= 16:
        r = X.restate_attn(cid, mode="bf16")
        with pytest.raises(AssertionError):
            X.verify_fwd(cid, r["out"], r["lse"], ref["fwd"])
        with pytest.raises(AssertionError):
            X.verify_bwd(cid, r, ref["bwd"])


def test_backward_formula_is_autograd_of_the_forward():
    """head_bwd on unrounded out and lse against float64 autograd of softmax(scale Q K^T) V, to 1e-12"""
    for cid in ("attn-N17", "attn-N65"):
        ref = X.attn_reference(cid)
        inp = ref["inp"]
        q, k, v, do = (torch.from_numpy(inp[n][0, 1]).clone() for n in ("q", "k", "v", "do"))
        q.requires_grad_(True), k.requires_grad_(True), v.requires_grad_(True)
        o = torch.softmax(X.SC * (q @ k.T), -1) @ v
        o.backward(do)
        f = X.head_fwd(inp["q"][0, 1], inp["k"][0, 1], inp["v"][0, 1])
        assert np.abs(f["out"] - o.detach().numpy()).max() <= 1e-12
        g = X.head_bwd(inp["q"][0, 1], inp["k"][0, 1], inp["v"][0, 1], inp["do"][0, 1], f["out"], f["lse"])
        for n, t in (("dq", q), ("dk", k), ("dv", v)):
            assert np.abs(g[n] - t.grad.numpy()).max() <= 1e-12 * max(1.0, float(t.grad.abs().max())), n


# ---- the constants -------------------------------------------------------------------------------------------------------------------------
def test_constants_are_eight_times_a_fresh_measurement():
    cf, cb = X.measure_attn_constants()
    for name, committed, measured in (("C_X3", X.C_X3, X.measure_c_x3()), ("DGELU_ABS", X.DGELU_ABS, X.measure_dgelu_abs()), ("C_FN", X.C_FN, X.measure_c_fn()),
                                      ("C_ATT_F", X.C_ATT_F, cf), ("C_ATT_B", X.C_ATT_B, cb)):
        print("%s committed %.4g measured %.4g" % (name, committed, measured))
        assert 4.0 * measured <= committed <= 16.0 * measured, (name, committed, measured)
    for fresh, committed in zip(X.measure_attn_x3_restated(), X.ATT_X3_RESTATED):       # the x3 restatement's share of the attention bounds
        assert abs(fresh - committed) <= 0.1 * committed, (fresh, committed)
    assert X.C_FN == 8.0 * X.C_FN_MEASURED and X.DGELU_ABS == 8.0 * X.DGELU_ABS_MEASURED
    assert X.C_X3 == 8.0 * X.C_X3_MEASURED and X.C_ATT_F == 8.0 * X.C_ATT_F_MEASURED and X.C_ATT_B == 8.0 * X.C_ATT_B_MEASURED


# ---- the planted faults ----------------------------------------------------------------------------------------------------------------------
def _reject(fn, what):
    with pytest.raises(AssertionError) as e:
        fn()
    print("%s: %s" % (what, str(e.value)[:300]))


@pytest.mark.parametrize("fault", list(X.FAULTS))
def test_verify_rejects_every_planted_fault(fault):
    family, cid = X.FAULTS[fault]
    if family == "gemm":
        ok, bad = X.GemmLaunch(X.GEMM_BY_ID[cid], "cpu"), X.GemmLaunch(X.GEMM_BY_ID[cid], "cpu")
        ok.restate()
        ok.verify()
        bad.restate(fault=fault)
        assert not np.array_equal(ok.C.bits(), bad.C.bits()), "the fault changed nothing"
        _reject(bad.verify, fault)
    elif family == "tn":
        ok, bad = X.TnLaunch(X.TN_BY_ID[cid], "cpu"), X.TnLaunch(X.TN_BY_ID[cid], "cpu")
        ok.restate()
        ok.verify()
        bad.restate(fault=fault)
        _reject(bad.verify, fault)
    else:
        ref = X.attn_reference(cid)
        r = X.restate_attn(cid, fault=fault)

        def both():
            X.verify_fwd(cid, r["out"], r["lse"], ref["fwd"])
            X.verify_bwd(cid, r, ref["bwd"])
        _reject(both, fault)


# ---- what the whole-tensor thresholds of the old tests read ----------------------------------------------------------------------------------
def _old_thresholds():
    """the thresholds of the old tests, read from their source (importing a GPU test module here is not an option): a change there shows here"""
    here = os.path.dirname(os.path.abspath(__file__))
    read = open(os.path.join(here, "test_gpu_read_rows_precision.py")).read()
    grad = open(os.path.join(here, "test_gpu_grad_rows_precision.py")).read()

    def one(src, pattern):
        m = re.findall(pattern, src, flags=re.M)
        assert len(m) == 1, (pattern, m)
        return float(m[0])
    return (one(read, r"^GEMM_REL = ([0-9.e-]+)"), one(read, r"^ATTN_REL = ([0-9.e-]+)"), one(grad, r"^KERNEL_REL = ([0-9.e-]+)"),
            one(grad, r"assert e < ([0-9.e-]+), \(nm, e\)"), one(grad, r"assert rel\(lse, torch\.logsumexp\(s, -1\)\) < ([0-9.e-]+)"),
            one(grad, r"assert rel\(b, rb\) < ([0-9.e-]+),"))


GEMM_REL, ATTN_REL, KERNEL_REL, DQKV_REL, LSE_REL, DBIAS_REL = _old_thresholds()


def _rel(got, want):
    d = float(np.linalg.norm((got - want).ravel()) / np.linalg.norm(want.ravel()))
    return d if np.isfinite(d) else float("inf")


def _gemm_reading(fault, api, epi, M, N, K, rs=False):
    """the old test's own statistic on the faulty restatement at its own shape: [(reading, threshold)]; caught: an exact check of the old test"""
    L = X.GemmLaunch(X._g(api, epi, M, N, K, rs=rs, bias=api != "nn", rps=257), "cpu")      # (the old tests' rows_per_sample)
    L.restate(fault=fault)
    got = L.C.get()
    R = X._case_product(M, N, K, L.c["seed"], False)
    v = R["true"] + (0.0 if L.bias is None else L.bias.astype(np.float64))
    if epi == "resid":
        s = L.row_scales().astype(np.float64)
        keep = s != 0
        c0 = L.c0.astype(np.float64)
        if not np.array_equal(got[~keep], c0[~keep]):
            return [(float("inf"), 0.0)]                    # "a dropped path leaves the residual bit for bit"
        return [(_rel((got - c0)[keep], (s[:, None] * v)[keep]), GEMM_REL)]
    if epi == "gelu":
        return [(_rel(got, X.gelu64(v)), GEMM_REL)]
    if epi == "dgelu":
        return [(_rel(got, v * X.gelu_grad64(L.aux.astype(np.float64))), KERNEL_REL)]
    return [(_rel(got, v), GEMM_REL)]


def _tn_reading(fault):
    ln = dict(id="old-tn-shapes", pitched=False, problems=((384, 1536, 771, True), (384, 384, 771, True), (128, 512, 771, True)))
    L = X.TnLaunch(ln, "cpu")
    L.restate(fault=fault)
    out = []
    for p in L.P:
        A8, B8 = p["A"].astype(np.float64), p["B"].astype(np.float64)
        out.append((_rel(p["aC"].get(), p["c0"].astype(np.float64) + A8.T @ B8), KERNEL_REL))
        out.append((_rel(p["aD"].get()[0], p["d0"].astype(np.float64) + A8.sum(0)), DBIAS_REL))
    return out


@functools.lru_cache(maxsize=1)
def _old_attn_heads(B=3, N=257, H=6):
    rng = np.random.Generator(np.random.PCG64(N * H))
    heads = []
    for _ in range(B * H):
        q, k, v = (1.5 * rng.standard_normal((N, 64)).astype(F).astype(np.float64) for _ in range(3))
        do = 0.1 * rng.standard_normal((N, 64)).astype(F).astype(np.float64)
        f = X.head_fwd(q, k, v)
        heads.append((q, k, v, do, f, X.head_bwd(q, k, v, do, f["out"], f["lse"])))
    return heads


def _attn_reading(fault):
    """test_attention_backward_against_fp64: the backward behind the forward (its out and lse), Gaussian qkv of scale 1.5, dO of scale 0.1"""
    got = {n: [] for n in ("out", "lse", "dq", "dk", "dv")}
    want = {n: [] for n in got}
    for q, k, v, do, f, w in _old_attn_heads():
        o, l = X.restate_fwd(q, k, v, fault=fault)
        g = X.restate_bwd(q, k, v, do, o, l, fault=fault)
        for n, a, b in (("out", o, f["out"]), ("lse", l, f["lse"]), ("dq", g["dq"], w["dq"]), ("dk", g["dk"], w["dk"]), ("dv", g["dv"], w["dv"])):
            got[n].append(a)
            want[n].append(b)
    thr = dict(out=KERNEL_REL, lse=LSE_REL, dq=DQKV_REL, dk=DQKV_REL, dv=DQKV_REL)
    return [(_rel(np.stack(got[n]), np.stack(want[n])), thr[n]) for n in got]


def norm_readings(fault):
    if fault in ("al_zero_one_kstep", "split2_second_lo"):      # the 72-image read launch: 18504 rows of the proj product
        return _gemm_reading(fault, "nt3", "resid", 18504, 384, 384, rs=True)
    if fault in ("last_row_from_M-2", "bias_dropped_last_col"):
        return _gemm_reading(fault, "nt3", "f32", 2056, 1152, 384)
    if fault == "tanh_gelu_one_row":
        return _gemm_reading(fault, "nt3", "gelu", 2056, 1536, 384)
    if fault in ("resid_bias_unscaled", "row_scale_index_off", "scale0_changed_resid"):
        return _gemm_reading(fault, "nt3", "resid", 2056, 384, 384, rs=True)
    if fault == "aux_dense_pitch":
        return [(0.0, KERNEL_REL)]                              # the old test's aux IS dense (ldaux = N): the fault cannot show there at all
    if fault.startswith("tn_"):
        return _tn_reading(fault)
    return _attn_reading(fault)


def test_what_the_norm_thresholds_let_pass():
    """Every planted fault at the old tests' own shapes (2056- and 18504-row products of ViT-S, 771 tokens, 3 x 6 heads of 257 tokens; Gaussian operands):
    the statistic each old test computes, beside its threshold.  NORM_BLIND is the set that stays under every one of them."""
    blind = []
    for fault in X.FAULTS:
        rd = norm_readings(fault)
        passed = all(r < t for r, t in rd)
        print("%-30s %s  %s" % (fault, "PASSES the norms" if passed else "caught", " ".join("%.2e/%.0e" % rt for rt in rd)))
        if passed:
            blind.append(fault)
    assert tuple(blind) == X.NORM_BLIND, blind
    assert len(blind) >= 3


# ---- refusals (no launch: the guards return before any HIP call) -----------------------------------------------------------------------------
def test_x3_entry_points_refuse_bad_arguments_without_a_gpu():
    from semireward_amd import _lib
    lib = _lib.lib()
    a, E = 0x10000, -1                                             # a 16-byte-aligned address that is never dereferenced; SR_EINVAL

    def nt3(epi=0, A=a, lda=64, W=a, ldw=64, C=a, ldc=16, M=16, N=16, K=64, bias=None, rs=None, rps=0):
        return lib.srhip_gemm_nt_x3(epi, A, lda, W, ldw, C, ldc, M, N, K, bias, rs, rps, None)

    def x3(layout, epi, A=a, lda=64, B=a, ldb=64, C=a, ldc=16, M=16, N=16, K=64, bias=None, aux=None, aux_out=None, ldaux=0):
        return lib.srhip_gemm_x3(layout, epi, A, lda, B, ldb, C, ldc, M, N, K, bias, aux, aux_out, ldaux, None)

    for kw in (dict(K=48), dict(lda=66), dict(ldw=66), dict(lda=32), dict(ldw=32), dict(ldc=8), dict(A=a + 4), dict(W=a + 4),
               dict(epi=2, rs=a, rps=0), dict(epi=0, rs=a, rps=37), dict(epi=1, rs=a, rps=37), dict(epi=7), dict(epi=-1), dict(M=0), dict(A=None)):
        assert nt3(**kw) == E, kw
    NT, NN, F32, ACC, DGELU, PRE = 0, 1, 0, 1, 2, 3
    nt = dict(aux_out=a, ldaux=16)
    for kw in (dict(K=48), dict(lda=66), dict(ldb=66), dict(lda=32), dict(ldb=32), dict(ldc=8), dict(A=a + 4), dict(B=a + 4), dict(aux_out=None),
               dict(ldaux=12)):
        assert x3(NT, PRE, **dict(nt, **kw)) == E, kw
    for epi in (F32, ACC, DGELU, 9):
        assert x3(NT, epi, **nt) == E, epi                         # NT has the GELU_PRE epilogue only
    assert x3(2, F32, ldb=16) == E and x3(-1, F32, ldb=16) == E    # unknown layout
    for kw in (dict(bias=a), dict(N=14), dict(ldb=12), dict(K=48), dict(lda=32), dict(ldc=8), dict(A=a + 4), dict(B=a + 4)):
        assert x3(NN, F32, **dict(dict(ldb=16), **kw)) == E, kw
        assert x3(NN, ACC, **dict(dict(ldb=16), **kw)) == E, kw
    assert x3(NN, DGELU, ldb=16, aux=None, ldaux=16) == E          # DGELU without aux
    assert x3(NN, DGELU, ldb=16, aux=a, ldaux=12) == E
    assert x3(NN, PRE, ldb=16, aux_out=a, ldaux=16) == E and x3(NN, 9, ldb=16) == E      # unknown epilogue of NN
    for N in (0, 513):
        assert lib.srhip_attn_fwd_x3(a, a, 1, N, 2, 0.125, None) == E
        assert lib.srhip_attn_fwd_x3_lse(a, a, a, 1, N, 2, 0.125, None) == E
        assert lib.srhip_attn_bwd_x3(a, a, a, a, a, a, 1, N, 2, 0.125, None) == E
    assert lib.srhip_attn_fwd_x3(a + 4, a, 1, 17, 2, 0.125, None) == E and lib.srhip_attn_fwd_x3(a, a + 4, 1, 17, 2, 0.125, None) == E
    assert lib.srhip_attn_fwd_x3_lse(a + 4, a, a, 1, 17, 2, 0.125, None) == E and lib.srhip_attn_fwd_x3_lse(a, a + 4, a, 1, 17, 2, 0.125, None) == E
    assert lib.srhip_attn_fwd_x3_lse(a, a, None, 1, 17, 2, 0.125, None) == E                                # null lse
    for i in (0, 1, 2, 4):                                                                                  # qkv, out, d_out, dqkv misaligned
        p = [a] * 6
        p[i] = a + 4
        assert lib.srhip_attn_bwd_x3(*p, 1, 17, 2, 0.125, None) == E, i
    assert lib.srhip_attn_bwd_x3(a, a, a, None, a, a, 1, 17, 2, 0.125, None) == E                           # null lse
    assert lib.srhip_attn_bwd_x3(a, a, a, a, a, None, 1, 17, 2, 0.125, None) == E                           # null delta_ws
    assert lib.srhip_gemm_tn_x3_grouped(None, 1, 1, None) == E
    assert lib.srhip_gemm_tn_x3_grouped(a, 0, 1, None) == E and lib.srhip_gemm_tn_x3_grouped(a, 1, 0, None) == E
    assert lib.srhip_layernorm_fwd_f32(a, a, a, 1e-6, a, None, None, 4, 100, None) == E                     # D without an instantiation
    assert lib.srhip_layernorm_fwd_f32(a, a, a, 1e-6, a, a, None, 4, 384, None) == E                        # mean without rstd
    assert lib.srhip_layernorm_fwd_f32(a, a, a, 1e-6, a, None, None, 0, 384, None) == E
