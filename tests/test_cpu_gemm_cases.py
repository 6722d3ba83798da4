"""What tests/_gemm_cases.py promises, stated without a GPU: the two constants of its bound are 8 times what the float32 restatements measure and
stay below the rigorous bound; the float32 restatement of every case and form passes the very function the GPU tests hold the kernels to; that
function rejects each planted fault; the criterion the dense tests used before (rel-L2 of the whole tensor < 4e-3 ... 5e-3) lets three of those
faults pass at M = 70001; every case reaches the kernel it names under srhip_gemm_nt_plan; no dropout mask is trivial on a block of a last row tile."""
import numpy as np
import pytest
import torch

import _gemm_cases as GC
from semireward_amd import ops

PAIRS, IDS = GC.params()


@pytest.fixture(scope="module", autouse=True)
def small_grid_alone():
    prev = ops._small_max_grid
    ops.gemm_small_max_grid(ops.GEMM_SMALL_ALONE)
    yield
    ops.gemm_small_max_grid(prev if prev is not None else ops.GEMM_SMALL_ALONE)


_ACC = {}


def acc_of(c, overlap):
    """the forward float32 accumulation of a product (the last one stays cached: the forms of a shape follow each other)"""
    key = (c["id"], c["seed"], overlap)
    if key not in _ACC:
        _ACC.clear()
        _ACC[key] = GC.accumulate32(c, overlap)
    return _ACC[key]


def restated(c, f, **kw):
    L = GC.Launch(c, f, "cpu")
    GC.restate(L, acc_of(c, f["overlap"]), **kw)
    return L


def test_committed_constants_are_eight_times_the_measurement():
    c_acc, dg = GC.measure_c_acc(), GC.measure_dgelu_abs()
    print("C_ACC: measured %.4f committed %.4f x 8 = %.3f;  DGELU_ABS: measured %.4e committed %.4e x 8 = %.3e" % (
        c_acc, GC.C_ACC_MEASURED, GC.C_ACC, dg, GC.DGELU_ABS_MEASURED, GC.DGELU_ABS))
    assert GC.C_ACC == 8.0 * GC.C_ACC_MEASURED and GC.DGELU_ABS == 8.0 * GC.DGELU_ABS_MEASURED
    assert 4.0 * c_acc <= GC.C_ACC <= 16.0 * c_acc
    assert 4.0 * dg <= GC.DGELU_ABS <= 16.0 * dg
    # any order of K products, K - 1 additions and the bias is within (K + 1) 2^-24 S to first order: the bound asks for less at every K in use
    assert GC.C_ACC < min(c["K"] for c in GC.CASES)


@pytest.mark.parametrize("c,f", PAIRS, ids=IDS)
def test_float32_restatement_is_within_the_bound(c, f):
    ratio = GC.verify(restated(c, f))
    print("%s-%s: max |restatement - float64| / tol = %.3f" % (c["id"], f["name"], ratio))
    assert ratio <= 1.0


# ---- planted faults ------------------------------------------------------------------------------------------------------------------------
SMALL, TILE128 = GC.by_id("small64-771x384x384"), GC.by_id("tile128-8321x388x384")


def _rejected(L, what):
    with pytest.raises(AssertionError) as e:
        GC.verify(L)
    print("%s -> %s" % (what, str(e.value)[:300]))


@pytest.mark.parametrize("c", [SMALL, TILE128], ids=lambda c: c["id"])
def test_checker_rejects_each_planted_fault(c):
    M, N, K = c["M"], c["N"], c["K"]
    F = GC.form
    assert GC.verify(restated(c, F("bf16"))) <= 1.0 and GC.verify(restated(c, F("resid_rowscale"))) <= 1.0
    # the last valid row stored as zeros
    L = restated(c, F("bf16"))
    L.C[M - 1] = 0
    _rejected(L, "last row zeroed")
    # the bias left off one row
    for name in ("bf16", "gelu", "resid_inplace"):
        L = GC.Launch(c, F(name), "cpu")
        acc = acc_of(c, 0).clone()
        acc[M // 2] -= GC.bias_of(c)
        GC.restate(L, acc)
        _rejected(L, "bias omitted on row %d (%s)" % (M // 2, name))
    # one 32-wide k-chunk missing from one 16 x 16 block
    for name in ("bf16", "resid_aux", "dgelu"):
        L = GC.Launch(c, F(name), "cpu")
        acc = acc_of(c, 0).clone()
        rows, cols = slice(M - 1 - 16, M - 1), slice(32, 48)
        acc[rows, cols] -= GC.chunk32(c, 0, K - 32, rows, cols)
        GC.restate(L, acc)
        _rejected(L, "k-chunk missing from a 16 x 16 block (%s)" % name)
    # two neighbouring columns swapped inside one tile
    L = restated(c, F("bf16"))
    t = L.C[64:128, 17].clone()
    L.C[64:128, 17] = L.C[64:128, 18]
    L.C[64:128, 18] = t
    _rejected(L, "columns 17 and 18 swapped in one tile")
    # the first row of a sample scaled with the sample before
    L = GC.Launch(c, F("resid_rowscale"), "cpu")
    rs = L.row_scale_rows().clone()
    assert rs[GC.RPS] != rs[GC.RPS - 1]
    rs[GC.RPS] = rs[GC.RPS - 1]
    GC.restate(L, acc_of(c, 0), row_scale_rows=rs)
    _rejected(L, "row %d scaled as the sample before it" % GC.RPS)
    # the two elements of one dropout pair exchanged
    for name in ("gelu_drop", "dgelu_drop", "resid_drop"):
        L = restated(c, F(name))
        k = L.keep.reshape(-1)
        i = 2 * int((k[0::2] != k[1::2]).to(torch.int8).argmax())
        assert k[i] != k[i + 1]
        r, col = divmod(i, N)
        t = L.C[r, col].clone()
        L.C[r, col] = L.C[r, col + 1]
        L.C[r, col + 1] = t
        _rejected(L, "dropout pair (%d, %d..%d) exchanged (%s)" % (r, col, col + 1, name))
    # one element of the padding overwritten: after the last row, before the first, between N and ldc, in the saved pre-activations
    for name, where in (("bf16", "after"), ("resid_inplace", "front"), ("pitch4_bf16", "pitch"), ("gelu_aux_ld2", "aux")):
        L = restated(c, F(name))
        if where == "after":
            L.C_buf[GC.FRONT + M * L.ldc] = 1.0
        elif where == "front":
            L.C_buf[GC.FRONT - 1] = 1.0
        elif where == "pitch":
            L.C_buf[GC.FRONT + 5 * L.ldc + N] = 1.0
        else:
            L.aux_out_buf[GC.FRONT + 7 * L.ldaux + N + 1] = 1.0
        _rejected(L, "one pad element overwritten (%s)" % where)
    # one bf16 output one ulp off (away from the expectation)
    for name in ("bf16", "gelu", "dgelu"):
        L = restated(c, F(name))
        ex = GC.expect(L)
        r, col = M // 2, N // 2
        got, want = float(L.C[r, col]), float(ex["want"][r, col])
        away = (got >= want) == (got >= 0)            # a larger magnitude moves away from the expectation
        bits = L.C[r:r + 1, col:col + 1].clone().view(torch.int16)
        L.C[r, col] = (bits + (1 if away else -1)).view(torch.bfloat16)[0, 0]
        assert float(L.C[r, col]) != got
        _rejected(L, "one bf16 output one ulp off (%s)" % name)
    # the saved pre-activation one ulp off
    L = restated(c, F("gelu_aux"))
    r, col = M // 3, N // 3
    bits = L.aux_out[r:r + 1, col:col + 1].clone().view(torch.int16)
    got, want = float(L.aux_out[r, col]), float(GC.expect(L)["aux_want"][r, col])
    L.aux_out[r, col] = (bits + (1 if (got >= want) == (got >= 0) else -1)).view(torch.bfloat16)[0, 0]
    _rejected(L, "one saved pre-activation one ulp off")


def test_whole_tensor_norm_lets_these_faults_pass():
    """The criterion of test_gemm_epilogues (rel-L2 of the whole tensor: < 4e-3 on the bf16 output and the saved pre-activation, < 5e-3 on the GELU
    output), on that test's own inputs at its M = 70001 case.  A row without its bias (2.39e-3) and a 16 x 16 block without one k-chunk (1.74e-3)
    pass 4e-3 on the bf16 output beside a clean 1.66e-3; a last row of zeros adds 1 / sqrt(M) = 3.8e-3 in quadrature: 4.09e-3 on the bf16
    output -- caught there by 2 % of the bound, and only at this M or below -- and it passes the 5e-3 the same test holds the GELU output to.
    The recorded reason for the per-element bound."""
    M, N, K = 70001, 1152, 384

    def rnd(*shape, seed=0, scale=1.0):
        g = np.random.Generator(np.random.PCG64(seed))
        return torch.from_numpy((scale * g.standard_normal(shape)).astype(np.float32))
    A, B, bias = rnd(M, K, seed=1).to(torch.bfloat16).float(), rnd(N, K, seed=2, scale=0.1).to(torch.bfloat16).float(), rnd(N, seed=3)
    refb = A @ B.t() + bias                                   # (float32: 1e-7 beside a criterion of 4e-3)

    def relerr(C, ref):
        return float((C.double() - ref.double()).norm() / ref.double().norm())
    clean = refb.to(torch.bfloat16).float()
    base = relerr(clean, refb)
    C = clean.clone()
    C[M - 1] = 0
    zero_row = relerr(C, refb)
    C = clean.clone()
    C[M // 2] = (refb[M // 2] - bias).to(torch.bfloat16).float()
    no_bias = relerr(C, refb)
    C = clean.clone()
    rows, cols = slice(M - 17, M - 1), slice(32, 48)
    C[rows, cols] = (refb[rows, cols] - A[rows, K - 32:] @ B[cols, K - 32:].t()).to(torch.bfloat16).float()
    no_chunk = relerr(C, refb)
    refg = torch.nn.functional.gelu(refb)
    G = refg.to(torch.bfloat16).float()
    base_g = relerr(G, refg)
    G[M - 1] = 0
    zero_row_g = relerr(G, refg)
    print("rel-L2 at M = 70001, bf16 output: clean %.3e, last row zeroed %.3e, bias off one row %.3e, k-chunk off one block %.3e;  GELU output: "
          "clean %.3e, last row zeroed %.3e" % (base, zero_row, no_bias, no_chunk, base_g, zero_row_g))
    assert base < no_bias < 4e-3 and base < no_chunk < 4e-3
    assert base_g < zero_row_g < 5e-3
    assert 4e-3 < zero_row < 4.2e-3                           # what the bf16 output's 4e-3 does catch, by 2 %: one more row and it would not


# ---- the cases reach what they name --------------------------------------------------------------------------------------------------------
def test_every_case_reaches_the_kernel_it_names():
    for c in GC.CASES:
        for name in c["forms"]:
            f = GC.form(name)
            assert ops.gemm_nt_plan(f["epi"], c["M"], c["N"], c["K"], f["beta"]) == c["plan"], (c["id"], name)
    assert {c["plan"] for c in GC.CASES} == set(GC.PRODUCTION_PLANS)
    # the stores the cases are there for: wide needs N % 128 == 0 and ldc % 8 == 0 (and ldaux % 4 == 0 with aux_out)
    for plan in ("small64", "tile128", "pp256", "big256"):
        wide = {(c["N"] % 128 == 0 and (c["N"] + GC.form(n)["c_pad"]) % 8 == 0 and (c["N"] + GC.form(n)["aux_pad"]) % 4 == 0)
                for c in GC.CASES if c["plan"] == plan for n in c["forms"] if GC.form(n)["epi"] in GC.BF16_EPIS}
        assert wide == {True, False}, plan
    # split-K: 33 k-tiles over 4 splits of 9, 9, 9, 6
    assert GC.by_id("tile128-136x72x1056")["K"] // 32 == 33
    # the accumulation forms every kernel owes, by kernel
    for plan in GC.PRODUCTION_PLANS:
        names = {n for c in GC.CASES if c["plan"] == plan for n in c["forms"]}
        assert set(GC.FULL) <= names, plan
        assert ("resid_ln" in names) == (plan != "big256") and ("overlap_bf16" in names) == (plan != "big256")
        assert bool(set(GC._F32) & names) == (plan == "tile128")


def test_no_dropout_mask_is_trivial_on_a_block_of_the_last_row_tile():
    for c in GC.CASES:
        if not any(GC.form(n)["drop"] for n in c["forms"]):
            continue
        M, N, T = c["M"], c["N"], GC.TILE[c["plan"]]
        keep = GC.keep_of(M, N, c["dseed"])
        assert 0.08 < 1.0 - float(keep.float().mean()) < 0.12
        for r0 in range((M - 1) // T * T, M, 16):
            for c0 in range(0, N, 16):
                blk = keep[r0:min(r0 + 16, M), c0:c0 + 16]
                assert bool(blk.any()) and not bool(blk.all()), (c["id"], r0, c0)
