"""Every attention kernel of csrc/attention.hip per element against float64, through the C ABI: the cases, inputs, references and bounds of
tests/_attn_cases.py.  A case asserts the kernel and grid srhip_attn_plan names before it launches.  On failure the message names the kernel,
the element, got / want / bound and the head, tile and lane group the element belongs to.  Each test prints its headroom (largest
|got - want| / bound) per output."""
import numpy as np
import pytest
import torch

import _attn_cases as A
from semireward_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _report(c, form, ratios):
    for n, r in ratios.items():
        print("HEADROOM|%s|%s|%s|%.3f|%s" % (A.kernel_name(c, "bwd" if n == "P(dv)" else form), form, n, r, c["id"]))


def _other_garbage(c, inp):
    """The same inputs with other large values in the padded K and V rows; None when the case has no padded row."""
    if c["key_len"] is None or all(x == c["N"] for x in c["key_len"]):
        return None
    g = dict(inp, k=inp["k"].copy(), v=inp["v"].copy())
    A.fill_garbage(g["k"], g["v"], g["klen"], 1)
    assert not np.array_equal(g["k"], inp["k"])
    return g


def _fwd(c, ref, with_lse):
    B, N, H, inp, drop = c["B"], c["N"], c["H"], ref["inp"], ref["drop"]
    kernel = A.kernel_name(c, "fwd")
    out, lse = A.launch_fwd(c, DEV, inp, drop, with_lse=with_lse)
    ratios = A.verify_fwd(kernel, A._unpack(out.values(), B, N, H), lse.values().reshape(B, H, N) if with_lse else None, ref["fwd"])
    assert out.padding_untouched(), kernel + ": out padding changed"
    assert lse is None or lse.padding_untouched(), kernel + ": lse padding changed"
    other = _other_garbage(c, inp)
    if other is not None:                                   # other finite values in the padded K / V rows: the same bits
        out2, lse2 = A.launch_fwd(c, DEV, other, drop, with_lse=with_lse)
        assert np.array_equal(out.bits(), out2.bits()), kernel + ": out depends on padded K / V rows"
        assert lse is None or np.array_equal(lse.bits(), lse2.bits()), kernel + ": lse depends on padded K / V rows"
    if B > 1:                                               # sequence 0 alone: the bytes it has in the batch
        out1, lse1 = A.launch_fwd(c, DEV, inp, drop, with_lse=with_lse, B=1)
        assert np.array_equal(out.bits()[:N], out1.bits()), kernel + ": sequence 0 alone differs from sequence 0 in the batch"
        assert lse is None or np.array_equal(lse.bits()[:H], lse1.bits())
    return ratios, out


def _bwd(c, ref):
    B, N, H, inp, drop = c["B"], c["N"], c["H"], ref["inp"], ref["drop"]
    kernel = A.kernel_name(c, "bwd")
    dqkv, delta = A.launch_bwd(c, DEV, inp, drop, ref["fwd"])
    got = A.split_dqkv(dqkv.values(), B, N, H)
    got["delta"] = delta.values().reshape(B, H, N)
    ratios = A.verify_bwd(kernel, got, ref["bwd"])
    for b in range(B):                                      # rows of padded keys: zero, either sign (their bound is zero; said again for the reader)
        L = int(inp["klen"][b])
        assert not got["dk"][b, :, L:].any() and not got["dv"][b, :, L:].any(), kernel
    assert dqkv.padding_untouched(), kernel + ": dqkv padding changed"
    assert delta.padding_untouched(), kernel + ": delta_ws padding changed"
    other = _other_garbage(c, inp)
    if other is not None:
        dqkv2, delta2 = A.launch_bwd(c, DEV, other, drop, ref["fwd"])
        assert np.array_equal(dqkv.bits(), dqkv2.bits()), kernel + ": dqkv depends on padded K / V rows"
        assert np.array_equal(delta.bits(), delta2.bits()), kernel + ": delta_ws depends on padded K / V rows"
    if B > 1:
        dqkv1, delta1 = A.launch_bwd(c, DEV, inp, drop, ref["fwd"], B=1)
        assert np.array_equal(dqkv.bits()[:N], dqkv1.bits()), kernel + ": sequence 0 alone differs from sequence 0 in the batch"
        assert np.array_equal(delta.bits()[:H], delta1.bits())
    return ratios


def _readout(c, ref):
    """The probability matrix itself, as the forward makes it and as the backward regenerates it, window by window."""
    B, N, H, inp, drop = c["B"], c["N"], c["H"], ref["inp"], ref["drop"]
    R = A.readout_reference(c, inp, ref["keep"], ref["fwd"])
    fk, bk = A.kernel_name(c, "fwd"), A.kernel_name(c, "bwd")
    got_f, got_b = np.zeros((B, H, N, N)), np.zeros((B, H, N, N))
    ratios = {"P(out)": 0.0, "P(dv)": 0.0}
    for j in range((N + 63) // 64):
        n = min(64, N - 64 * j)
        out, _ = A.launch_fwd(c, DEV, inp, drop, v=A.readout_v(c, inp, j), with_lse=False)
        g = A._unpack(out.values(), B, N, H)
        ratios["P(out)"] = max(ratios["P(out)"], A.verify(fk, "P(out) window %d" % j, g, A.readout_window(R["fwd"], j), A.readout_window(R["fwd_tol"], j)))
        got_f[:, :, :, 64 * j:64 * j + n] = g[..., :n]
        dqkv, _ = A.launch_bwd(c, DEV, inp, drop, ref["fwd"], do=A.readout_do(c, inp, j))
        g = A.split_dqkv(dqkv.values(), B, N, H)["dv"]
        ratios["P(dv)"] = max(ratios["P(dv)"], A.verify(bk, "P(dv) window %d" % j, g, A.readout_window(R["bwd"], j, True),
                                                        A.readout_window(R["bwd_tol"], j, True)))
        got_b[:, :, 64 * j:64 * j + n, :] = g[..., :n].transpose(0, 1, 3, 2)
    # dropped and masked entries are exactly zero, kept ones are not: one zero set, the oracle's
    assert np.array_equal(got_f == 0, R["zero"]), fk + ": the forward's zero set is not the oracle's"
    assert np.array_equal(got_b == 0, R["zero"]), bk + ": the backward's zero set is not the oracle's"
    return ratios


@pytest.mark.parametrize("cid,form", A.CASE_FORMS, ids=["%s-%s" % cf for cf in A.CASE_FORMS])
def test_attention_case(cid, form):
    ref = A.case_reference(cid)
    c = ref["c"]
    assert ops.attn_plan(c["B"], c["N"], c["H"]) == c["plan"], cid
    if form == "fwd":
        ratios, _ = _fwd(c, ref, True)
    elif form == "fwd_nolse":                               # lse = NULL: the same output bits as with lse
        ratios, out = _fwd(c, ref, False)
        with_lse, _ = A.launch_fwd(c, DEV, ref["inp"], ref["drop"], with_lse=True)
        assert np.array_equal(out.bits(), with_lse.bits())
    elif form == "bwd":
        ratios = _bwd(c, ref)
    else:
        ratios = _readout(c, ref)
    _report(c, form, ratios)


# ---- the fused block ---------------------------------------------------------------------------------------------------------------------
def _block_launch(c, inp, B=None, out_scale=None):
    """srhip_attn_block_fused through ops.attn_block_fused, qkv_extra computed as production does; operands in NaN-padded allocations."""
    B = c["B"] if B is None else B
    N, D, H = c["N"], A.BLOCK_D, A.BLOCK_H
    xn = A.Buf(DEV, c["B"] * N, D, torch.bfloat16, inp["xn"])
    W = A.Buf(DEV, 3 * D, D, torch.bfloat16, inp["W"])
    b = A.Buf(DEV, 1, 3 * D, torch.float32, inp["b"][None])
    out = A.Buf(DEV, B * N, D, torch.bfloat16)
    qx = torch.full((B, 3 * D), float("nan"), dtype=torch.bfloat16, device=DEV) if N == 257 else None
    sc = None if out_scale is None else torch.tensor(out_scale, dtype=torch.float32, device=DEV)
    ops.attn_block_fused(xn.block, W.block, b.block.view(-1), out.block, B, N, D, H, A.SCALE, qkv_extra=qx, out_scale=sc)
    torch.cuda.synchronize()
    return out, (xn, W, b)


@pytest.mark.parametrize("cid", [c["id"] for c in A.BLOCK_CASES])
def test_fused_block_case(cid):
    c = A.BLOCK_BY_ID[cid]
    B, N, D, H = c["B"], c["N"], A.BLOCK_D, A.BLOCK_H
    assert ops.attn_block_supported(N, D, H)
    kernel = "attn_block_kernel<%d>" % N
    inp = A.make_block_inputs(c)
    ref = A.block_reference(c, inp)
    out, (xn, W, b) = _block_launch(c, inp)
    ratios = {"out": A.verify_block(kernel, c, out.values(), ref["out"], ref["tol"])}
    assert out.padding_untouched(), kernel + ": out padding changed"
    # the unfused pair on the same operands; each of the two results inside both bounds
    qkv = torch.empty(B * N, 3 * D, dtype=torch.bfloat16, device=DEV)
    pair = A.Buf(DEV, B * N, D, torch.bfloat16)
    ops.gemm_nt(ops.EPI_BF16, xn.block, W.block, qkv, B * N, 3 * D, D, bias=b.block.view(-1))
    ops.attn_fwd(qkv, pair.block, None, B, N, H, A.SCALE)
    torch.cuda.synchronize()
    ratios["pair"] = A.verify_block("srhip_gemm_nt + srhip_attn_fwd", c, pair.values(), ref["out"], ref["tol_pair"])
    A.verify_block(kernel + " in the pair's bound", c, out.values(), ref["out"], ref["tol_pair"])
    A.verify_block("srhip_gemm_nt + srhip_attn_fwd in the fused bound", c, pair.values(), ref["out"], ref["tol"])
    # image 0 alone: the bytes it has in the batch
    if B > 1:
        out1, _ = _block_launch(c, inp, B=1)
        assert np.array_equal(out.bits()[:N], out1.bits())
    # out_scale: 1 is the identity on the bits, 0 gives zeros, 1 / 0.85 is the scaled fp32 value rounded once: held against the unscaled
    # launch above, half a bf16 ulp of the unrounded value and of the result (verify_out_scale), not against the wider float64 bound
    s = float(np.float32(1.0 / 0.85))
    sc = ([1.0, 0.0, s] * B)[:B] if B > 1 else [s]
    outs, _ = _block_launch(c, inp, out_scale=sc)
    assert outs.padding_untouched()
    got, gots = out.values(), outs.values()
    for img in range(B):
        rows = slice(img * N, (img + 1) * N)
        if sc[img] == 1.0:
            assert np.array_equal(outs.bits()[rows], out.bits()[rows])
        elif sc[img] == 0.0:
            assert not gots[rows].any()
        else:
            r, frac = A.verify_out_scale("%s out_scale, image %d" % (kernel, img), c, gots[rows], got[rows], s)
            ratios["out_scale"], ratios["out_scale_differs"] = max(ratios.get("out_scale", 0.0), r), frac
    for n, r in ratios.items():
        print("HEADROOM|%s|block|%s|%.3f|%s" % (kernel, n, r, cid))


def test_fused_block_probability_readout():
    """N = 257, head BLOCK_READ_HEAD, the window that holds key 256: the head's output is the probability of key 256 in column 0 and exactly zero
    in the other 63, for every query including the extra one."""
    c = A.BLOCK_BY_ID["block-N257B3"]
    N, j, h0 = c["N"], 4, A.BLOCK_READ_HEAD
    inp = A.make_block_inputs(c, readout_window_j=j)
    ref = A.block_reference(c, inp)
    out, _ = _block_launch(c, inp)
    got = out.values()
    r = A.verify_block("attn_block_kernel<257> read-out", c, got, ref["out"], ref["tol"])
    head = got[:, h0 * A.HD:(h0 + 1) * A.HD].reshape(c["B"], N, A.HD)
    assert np.array_equal(ref["out"][:, h0 * A.HD:(h0 + 1) * A.HD].reshape(c["B"], N, A.HD)[..., 0], ref["P"][:, :, 256])
    assert not head[..., 1:].any() and (head[..., 0] > 0).all()
    print("HEADROOM|attn_block_kernel<257>|block|P(out)|%.3f|%s" % (r, c["id"]))
