"""Every split-bf16 kernel of csrc/x3.hip, and the fp32-output LayerNorm, per element against
float64, through the C ABI: the cases, arenas, references and bounds of tests/_x3_cases.py.  Every launch is made twice (the same bits), from
operands whose padding is NaN into outputs whose padding must come back bit for bit.  Each test prints `headroom <id> <ratio>`, the largest
|got - want| / bound, and asserts it is at most 1; the HEADROOM| lines feed tools/x3_cases_headroom.py."""
import numpy as np
import pytest
import torch

import _x3_cases as X
from semireward_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _report(kernel, form, cid, ratios):
    for n, r in ratios.items():
        print("HEADROOM|%s|%s|%s|%.3f|%s" % (kernel, form, n, r, cid))
    top = max(ratios.values())
    print("headroom %s %.3f" % (cid, top))
    assert top <= 1.0, (cid, ratios)


@pytest.mark.parametrize("cid", [c["id"] for c in X.GEMM_CASES])
def test_single_product(cid):
    c = X.GEMM_BY_ID[cid]
    L = X.GemmLaunch(c, DEV)
    X.same_twice(cid, L.outs, L.run_hip)
    L.verify()
    _report(X.KERNEL[c["api"]], c["epi"] + ("-rs" if c["rs"] else ""), cid, L.ratios)


@pytest.mark.parametrize("lid", [ln["id"] for ln in X.TN_LAUNCHES])
def test_grouped_weight_gradient(lid):
    L = X.TnLaunch(X.TN_BY_ID[lid], DEV)
    X.same_twice(lid, L.outs, L.run_hip)
    L.verify()
    _report("gemm_tn_x3_grouped_kernel", "pitched" if L.ln["pitched"] else "dense", lid, L.ratios)


@pytest.mark.parametrize("cid", [c["id"] for c in X.LN_CASES])
def test_layernorm_fp32_output(cid):
    L = X.LnLaunch(X.LN_BY_ID[cid], DEV)
    X.same_twice(cid, L.outs, L.run_hip)
    r = L.verify()
    _report("ln_fwd_kernel<%d, float>" % (L.c["D"] // 128), "stats" if L.c["stats"] else "nostats", cid, {"out+stats": r})


@pytest.mark.parametrize("cid", [c["id"] for c in X.ATTN_CASES])
def test_attention_forward(cid):
    L = X.AttnLaunch(cid, DEV)
    outs = [L.out, L.out2, L.lse]
    X.same_twice(cid, outs, L.run_fwd)
    assert np.array_equal(L.out.bits(), L.out2.bits()), "%s: srhip_attn_fwd_x3 and srhip_attn_fwd_x3_lse differ in out" % cid
    out, lse = L.got_fwd()
    f = L.ref["fwd"]
    ratios = {"out": X.within(cid, "out", out, f["out"], f["out_tol"]), "lse": X.within(cid, "lse", lse, f["lse"], f["lse_tol"])}
    for a in outs:
        assert not a.pad_touched(), "%s: output padding overwritten" % cid
    _report("attn_fwd_x3_kernel<false> / attn_fwd_x3_kernel<true>", "fwd", cid, ratios)


@pytest.mark.parametrize("cid", [c["id"] for c in X.ATTN_CASES])
def test_attention_backward(cid):
    """on the float64 forward's out and lse rounded to fp32 -- not behind the forward kernel; dqkv starts as NaN: every element is written"""
    L = X.AttnLaunch(cid, DEV)
    outs = [L.dqkv, L.delta]
    X.same_twice(cid, outs, L.run_bwd)
    got, b = L.got_bwd(), L.ref["bwd"]
    ratios = {n: X.within(cid, n, got[n], b[n], b[n + "_tol"]) for n in ("dq", "dk", "dv")}
    ratios["delta_ws"] = X.within(cid, "delta_ws", got["delta"], b["delta"], b["delta_tol"])
    for a in outs:
        assert not a.pad_touched(), "%s: output padding overwritten" % cid
    _report("attn_bwd_x3_dq_kernel + attn_bwd_x3_dkv_kernel", "bwd", cid, ratios)


def _view_bits(arena):
    return arena.view.cpu().contiguous().view(torch.int32).numpy().copy()


@pytest.mark.parametrize("M,N,K", [(1, 1, 32), (129, 132, 96), (300, 127, 64)])
def test_both_gemm_entry_points_are_one_engine(M, N, K):
    """srhip_gemm_nt_x3 and srhip_gemm_x3 launch the same tile engine (csrc/x3.hip): on the same operands, with bias, ldc = N + 3 and
    ldaux = N + 4, the pre-activation GELU_PRE keeps has the bits of the F32 launch's C, and its C has the bits of the GELU_F32 launch's C.
    One tile with one row, a ragged 2 x 2 tile grid with three k-steps, a ragged N."""
    L = X.GemmLaunch(X._g("nt", "gelu_pre", M, N, K, ldc_pad=3), DEV)
    assert L.ldc == N + 3 and L.ldaux == N + 4 and L.Bias is not None
    got = {}
    for name, epi in (("f32", ops.X3_EPI_F32), ("gelu", ops.X3_EPI_GELU_F32)):
        ops.gemm_nt_x3(epi, L.A.ptr, L.B.ptr, L.C.ptr, M, N, K, lda=L.lda, ldw=L.ldb, ldc=L.ldc, bias=L.Bias.ptr)
        torch.cuda.synchronize()
        assert not L.C.pad_touched(), "%s: output padding overwritten" % name
        got[name] = _view_bits(L.C)
        L.C.reset()
    L.run_hip()                                            # srhip_gemm_x3(NT, GELU_PRE)
    for a in L.outs:
        assert not a.pad_touched(), "gelu_pre: output padding overwritten"
    assert np.isfinite(L.AuxOut.get()).all() and np.isfinite(L.C.get()).all()
    assert np.array_equal(_view_bits(L.AuxOut), got["f32"]), "aux_out of GELU_PRE and C of srhip_gemm_nt_x3(F32) differ"
    assert np.array_equal(_view_bits(L.C), got["gelu"]), "C of GELU_PRE and C of srhip_gemm_nt_x3(GELU_F32) differ"
