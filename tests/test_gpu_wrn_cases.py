"""Every kernel of csrc/wrn_conv.hip, csrc/wrn_ops.hip and csrc/wrn_bn.h on the MI355X, element by element against float64: the cases, references,
bounds and verify functions of tests/_wrn_cases.py, which tests/test_cpu_wrn_cases.py shows accepting the float32 restatement of every case
and rejecting each planted fault.  Every convolution case asserts what srhip_wrn_conv_plan names before it launches and what
srhip_wrn_conv_last_plan reports after; no tuning variable is set: the shapes reach each template by the dispatcher's own rules.
Each test prints 'headroom <id> <max |got - want| / tol>' (profiles/wrn_cases_headroom.txt keeps the largest per kernel or template and form)."""
import pytest
import torch

import _wrn_cases as WC
from semireward_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def report(cid, H):
    for k, v in sorted(H.items()):
        print(("count %s %s %d" if k == "ulp1" else "headroom %s %s %.4f") % (cid, k, v))
    if not H:
        print("headroom %s same_bits 0.0000" % cid)             # (every output of the case is held to the same bits)
    assert all(v <= 1.0 for k, v in H.items() if k not in ("ulp1", "frac_w", "frac_amb")), H


def run(L):
    L.run_hip()
    torch.cuda.synchronize()
    H = L.verify()
    report(L.c["id"], H)
    return H


@pytest.mark.parametrize("c", WC.CONV_CASES, ids=[c["id"] for c in WC.CONV_CASES])
def test_conv_case(c):
    plan = ops.wrn_conv_plan(*c["shape"])
    assert plan.kernel == c["kernel"] and plan.rounds == c["rounds"], plan
    Wb = None
    if c["flip"]:                       # the filter operand of the input-gradient form comes from conv_weight_flip_grouped
        I, d = WC.conv_inputs(c["id"]), WC.conv_dims(c)
        Wf = torch.from_numpy(I["Wfwd"]).to(DEV)
        Wb = torch.full((d["Cout"], d["Kp"]), float("nan"), dtype=torch.bfloat16, device=DEV)
        desc, n, total = ops.make_conv_desc([(Wf, Wb, None, d["Cin"], d["Cout"], 3, d["Kp"])], DEV, lambda Cout, C, kk, Kpad: C * Kpad)
        ops.conv_weight_flip_grouped(desc, n, total)
        torch.cuda.synchronize()
        assert torch.equal(WC.bits(Wb.cpu()), WC.bits(I["Wb"]))
        Wb = Wb.cpu()
    L = WC.ConvLaunch(c, DEV, Wb=Wb)
    L.run_hip()
    torch.cuda.synchronize()
    assert ops.wrn_conv_last_kernel() == c["kernel"]
    report(c["id"], WC.conv_verify(L))


@pytest.mark.parametrize("c", WC.HEAD_CASES, ids=[c["id"] for c in WC.HEAD_CASES])
def test_head_case(c):
    run(WC.HeadLaunch(c, DEV))


@pytest.mark.parametrize("c", WC.BN_CASES, ids=[c["id"] for c in WC.BN_CASES])
def test_batchnorm_forward_case(c):
    run(WC.BnLaunch(c, DEV))


@pytest.mark.parametrize("c", WC.BWD_CASES, ids=[c["id"] for c in WC.BWD_CASES])
def test_batchnorm_backward_case(c):
    H = run(WC.BwdLaunch(c, DEV))
    assert H["frac_amb"] <= 1e-3


@pytest.mark.parametrize("c", WC.IM_CASES, ids=[c["id"] for c in WC.IM_CASES])
def test_im2col_col2im_case(c):
    run(WC.ImLaunch(c, DEV))


@pytest.mark.parametrize("c", WC.WEIGHT_TABLES, ids=[c["id"] for c in WC.WEIGHT_TABLES])
def test_filter_prep_and_unpad_case(c):
    run(WC.WeightLaunch(c, DEV))


@pytest.mark.parametrize("c", WC.FLIP_TABLES, ids=[c["id"] for c in WC.FLIP_TABLES])
def test_filter_flip_case(c):
    run(WC.WeightLaunch(c, DEV, flip=True))


@pytest.mark.parametrize("c", WC.FC_CASES, ids=[c["id"] for c in WC.FC_CASES])
def test_classifier_case(c):
    run(WC.FcLaunch(c, DEV))


@pytest.mark.parametrize("c", WC.POOL_CASES, ids=[c["id"] for c in WC.POOL_CASES])
def test_pooling_and_input_layout_case(c):
    run(WC.PoolLaunch(c, DEV))


@pytest.mark.parametrize("c", WC.SGD_CASES, ids=[c["id"] for c in WC.SGD_CASES])
def test_sgd_case(c):
    run(WC.SgdLaunch(c, DEV))
