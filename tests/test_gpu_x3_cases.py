"""Every split-bf16 kernel of csrc/precise.hip, csrc/precise_bwd.hip and csrc/x3.h, and the fp32-output LayerNorm, per element against
float64, through the C ABI: the cases, arenas, references and bounds of tests/_x3_cases.py.  Every launch is made twice (the same bits), from
operands whose padding is NaN into outputs whose padding must come back bit for bit.  Each test prints `headroom <id> <ratio>`, the largest
|got - want| / bound, and asserts it is at most 1; the HEADROOM| lines feed tools/x3_cases_headroom.py."""
import numpy as np
import pytest

import _x3_cases as X

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
    _report("attn_fwd_x3_kernel / attn_fwd_x3_lse_kernel", "fwd", cid, ratios)


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
