"""Audio front end (csrc/w2v_ops.hip and the grouped GEMM tables nets/wave2vec.py builds around it), kernel by kernel, against float64
references computed from the same bf16 / fp32 operands the kernels read: the bounds below measure only the kernel's own arithmetic and output
rounding.  Every comparison is over the full tensor, element by element.

Layout contract (w2v_ops.hip, header comment): activations are [clip, frame, channel] with a per-layer frame pitch P >= T + 1; rows t >= T are
filler -- finite values forward, exact zeros in every gradient buffer -- and the buffers carry slack rows past the last clip, which the
overlapping-row reads run into.  The tests fill every input's filler and slack rows with a large finite SENTINEL (0 x finite is the
contract, so NaN is not used) and check that the valid frames match the zero-filler reference, and that the outputs' filler frames are exact
zeros.

Bounds: u = 2^-24 (fp32 unit roundoff).  A sum of n terms accumulated in fp32 with a chain of at most L sequential additions is within
L * u * sum|terms| of the exact sum; L is stated per kernel.  A bf16 output may be off by one bf16 ulp of the exact value (round-to-nearest
of an fp32 value that is itself within half an ulp), plus the fp32 bound where there is a long sum in front of the rounding.  The GELU of
common.h (Abramowitz-Stegun erf, |erf error| <= 1.5e-7 + a few ulp of its fp32 evaluation) is within 2e-7 |z| + 3u |GELU| of GELU(z); its derivative within 4e-7 (|x phi(x)| <= 0.25
times a few ulp of the exponential, plus half the erf error)."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import w2v2_ref as WR                  # noqa: E402
from semireward_amd import ops                     # noqa: E402
from semireward_amd.nets import wave2vec           # noqa: E402

DEV = "cuda:0"
U = 2.0 ** -24
SENT = 3.0e4                                       # finite sentinel in filler frames and slack rows
SENT_BF = float(torch.tensor(SENT).to(torch.bfloat16))   # (29952 in a bf16 buffer)
SL = 16                                            # slack rows of the model's activation / gradient buffers (nets/wave2vec.py)
f32, f64, bf16 = torch.float32, torch.float64, torch.bfloat16


def rup(x, m):
    return (x + m - 1) // m * m


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def randn(shape, g, scale=1.0, dtype=f32):
    return (torch.randn(shape, generator=g, dtype=f64) * scale).to(dtype).to(DEV)


def bf16_ulp(x):
    """spacing of the bf16 numbers at |x| (float64)"""
    a = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def check(name, got, ref, tol):
    """|got - ref| <= tol element by element (float64); prints the largest deviation and its share of the bound."""
    got, ref = got.double(), ref.double()
    tol = torch.as_tensor(tol, dtype=f64, device=ref.device).expand_as(ref)
    err = (got - ref).abs()
    assert torch.isfinite(got).all(), name
    ratio = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("DEV %-44s max|err| %.3e  max err/tol %.3f" % (name, float(err.max()) if err.numel() else 0.0, ratio))
    bad = err > tol
    if bad.any():
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError("%s: %d of %d elements outside the bound; first at flat %d: got %.8g ref %.8g tol %.3g" % (
            name, int(bad.sum()), err.numel(), i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(tol.reshape(-1)[i])))


def check_bf16(name, got, ref, extra=0.0):
    check(name, got, ref, bf16_ulp(ref) + extra)


def pitched(valid, P, slack, fill=SENT):
    """[B, T, C] -> rows [B * P + slack, C] with the frame pitch P; filler frames and slack rows hold ``fill``"""
    B, T, C = valid.shape
    out = torch.full((B, P, C), fill, dtype=valid.dtype, device=valid.device)
    out[:, :T] = valid
    return torch.cat([out.reshape(B * P, C), torch.full((slack, C), fill, dtype=valid.dtype, device=valid.device)])


def frames_of(buf, B, P, T):
    return buf[:B * P].reshape(B, P, -1)[:, :T]


def filler_of(buf, B, P, T):
    return buf[:B * P].reshape(B, P, -1)[:, T:]


def gelu_grad64(z):
    with torch.enable_grad():
        z = z.detach().double().requires_grad_(True)
        F.gelu(z).backward(torch.ones_like(z))
    return z.grad


def conv_geometry(C, samples):
    cfg = wave2vec.W2vConfig(conv_dim=(C,) * 7)
    T, P, _ = wave2vec.ClassificationWave2Vec.geometry(types.SimpleNamespace(cfg=cfg), samples)
    return cfg, T, P


# ---- layer 0: conv + GroupNorm + GELU ---------------------------------------------------------------------------------------------------
CONV0 = [(128, 10, 5), (384, 10, 5), (512, 10, 5), (640, 10, 5), (128, 8, 4)]          # k10s5 kernel (C <= 512), then the generic kernel


@pytest.mark.parametrize("C,k,s", CONV0)
@pytest.mark.parametrize("T0", [100, 512, 769])          # below one 128-frame segment, 256 * 2, 256 * 3 + 1
@pytest.mark.parametrize("B", [1, 3])
def test_conv0_all_modes(C, k, s, T0, B):
    g = gen(1000 * C + 10 * T0 + B)
    S = s * (T0 - 1) + k + (s - 1)                        # the tail samples past the last window are read by nothing
    P0 = rup(T0 + 1, 8) + 8                               # filler rows in every clip
    eps = 1e-5
    wave = randn((B, S), g)
    W0 = randn((C, k), g, (2.0 / k) ** 0.5)
    gamma = (1.0 + 0.3 * torch.randn(C, generator=g)).float().to(DEV)
    beta = (0.3 * torch.randn(C, generator=g)).float().to(DEV)
    ws = torch.zeros(B, C, 2, dtype=f64, device=DEV)
    ws2 = torch.zeros(B, C, 2, dtype=f64, device=DEV)
    out = torch.full((B * P0 + SL, C), SENT, dtype=bf16, device=DEV)
    dY = pitched(randn((B, T0, C), g, 1.0, bf16), P0, SL)
    dW0_0, dg_0, db_0 = randn((C, k), g), randn(C, g), randn(C, g)
    dW0, dgam, dbet = dW0_0.clone(), dg_0.clone(), db_0.clone()
    a0 = (wave, W0, gamma, beta, ws, ws2)
    ops.w2v_conv0(0, *a0, None, None, None, None, None, B, S, T0, P0, C, k, s, eps)
    ops.w2v_conv0(1, *a0, out, None, None, None, None, B, S, T0, P0, C, k, s, eps)
    ops.w2v_conv0(2, *a0, None, dY, None, dgam, dbet, B, S, T0, P0, C, k, s, eps)
    ops.w2v_conv0(3, *a0, None, dY, dW0, None, None, B, S, T0, P0, C, k, s, eps)
    # float64 autograd reference: F.conv1d -> F.group_norm (groups = C) -> F.gelu
    w64 = W0.double().reshape(C, 1, k).requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.conv1d(wave.double()[:, None], w64, stride=s)                                       # [B, C, T0]
    assert y.shape[-1] == T0
    z = F.group_norm(y, C, g64, b64, eps)
    o = F.gelu(z)
    dy64 = frames_of(dY, B, P0, T0).double().transpose(1, 2)
    (o * dy64).sum().backward()
    with torch.no_grad():
        ya = F.conv1d(wave.double().abs()[:, None], w64.abs(), stride=s)                      # sum |terms| of each conv output
        mu, var = y.mean(-1, keepdim=True), y.var(-1, unbiased=False, keepdim=True)
        rs = (var + eps).rsqrt()
        xh = (y - mu) * rs
        gd = gelu_grad64(z)
        dgn = dy64 * gd
        dxh = dgn * g64[:, None]
        a1, a2 = dxh.mean(-1, keepdim=True), (dxh * xh).mean(-1, keepdim=True)
    # mode 0: sum and sum of squares per (clip, channel); fp32 runs of <= 2 segments x 128 frames (+ 10-tap dot products), then fp64 atomics
    L0 = 2 * 128 + k + 2
    check("conv0 ws sum C%d k%d T%d B%d" % (C, k, T0, B), ws[..., 0], y.sum(-1), L0 * U * ya.sum(-1))
    check("conv0 ws sumsq", ws[..., 1], (y * y).sum(-1), 2 * L0 * U * (ya * ya).sum(-1))
    # mode 1: per-element statistics error <= 256 u on mean / variance -> <= 4e-5 (1 + |xhat|) on xhat (mean and rstd each, x 2 margin);
    # output bf16: 1 ulp + GELU' x that + the A-S GELU error
    zerr = 4e-5 * (1.0 + xh.abs()) * g64.detach().abs()[:, None] + 4 * U * z.detach().abs()
    o_got = frames_of(out, B, P0, T0).transpose(1, 2)
    check_bf16("conv0 out", o_got, o.detach(), zerr * (gd.abs() + 0.2) + 2e-7 * z.detach().abs())
    assert (filler_of(out, B, P0, T0) == 0).all(), "filler frames of the layer-0 output are exact zeros"
    assert (out[B * P0:].float() == SENT_BF).all(), "nothing written past the last clip"
    # mode 2: backward statistics (fp32 runs of <= 128 frames, fp64 atomics) and dgamma / dbeta (fp32 atomics over B x segments):
    # per-term error <= 1e-4 relative (xhat as above, GELU' within 4e-7, |GELU''| <= 0.4)
    nseg = -(-T0 // 128)
    Lb = 128 + B * nseg + 2
    check("conv0 ws2 sum dxhat", ws2[..., 0], dxh.sum(-1), (Lb * U + 1e-4) * (dxh.abs().sum(-1) + 1e-30))
    check("conv0 ws2 sum dxhat*xhat", ws2[..., 1], (dxh * xh).sum(-1), (Lb * U + 1e-4) * ((dxh * xh).abs().sum(-1) + 1e-30))
    check("conv0 dgamma +=", dgam, dg_0.double() + g64.grad, (Lb * U + 1e-4) * (dgn * xh).abs().sum((0, 2)) + 2 * U * dg_0.double().abs())
    check("conv0 dbeta +=", dbet, db_0.double() + b64.grad, (Lb * U + 1e-4) * dgn.abs().sum((0, 2)) + 2 * U * db_0.double().abs())
    # mode 3: dW0 += sum_t dconv * wave; dconv = rstd (dxh - a1 - xh a2) has per-element error <= 1e-4 of rstd (|dxh| + |a1| + |xh a2|)
    with torch.no_grad():
        dca = rs * (dxh.abs() + a1.abs() + (xh * a2).abs())
        wu = wave.double().abs().unfold(1, k, s)[:, :T0]                                        # [B, T0, k]
        S_abs = torch.einsum("bct,btj->cj", dca, wu)
    check("conv0 dW0 +=", dW0, dW0_0.double() + w64.grad.reshape(C, k), (Lb * U + 2e-4) * S_abs + 2 * U * dW0_0.double().abs())


# ---- conv layers 1.. ------------------------------------------------------------------------------------------------------------------
def test_conv_weight_prep_is_bit_exact():
    g = gen(7)
    for Cout, Cin, k in [(128, 128, 3), (512, 512, 2), (256, 384, 5)]:
        W = randn((Cout, Cin, k), g)
        Wr = torch.full((Cout, k * Cin), SENT, dtype=bf16, device=DEV)
        WrT = torch.full((k * Cin, Cout), SENT, dtype=bf16, device=DEV)
        ops.w2v_conv_weight_prep(W, Wr, WrT, Cout, Cin, k)
        want = W.to(bf16).permute(0, 2, 1).reshape(Cout, k * Cin)                             # tap-major rows: [co][j][ci]
        assert torch.equal(Wr.view(torch.int16), want.view(torch.int16))
        assert torch.equal(WrT.view(torch.int16), want.t().contiguous().view(torch.int16))


def layer_shapes(Tprev, k, s):
    """frames / pitches of one conv layer with room for its overlapping reads (Pprev = s * P >= Tprev + 1)"""
    T = (Tprev - k) // s + 1
    P = rup(max(T + 1, -(-(Tprev + 1) // s)), 8)
    return T, P, s * P


@pytest.mark.parametrize("C", [128, 512])
@pytest.mark.parametrize("k,s", [(3, 2), (2, 2)])
@pytest.mark.parametrize("B,Tprev", [(1, 301), (3, 1600)])
def test_conv_layer_forward_gemm(C, k, s, B, Tprev):
    """conv layers 1..: gemm_nt(EPI_GELU_BF16, lda = s * C, aux_out = pre) exactly as forward_features issues it, the im2col operand being the
    previous activation read with overlapping rows"""
    g = gen(C + 10 * k + B)
    T, P, Pprev = layer_shapes(Tprev, k, s)
    xv = randn((B, Tprev, C), g, 1.0, bf16)
    W = randn((C, C, k), g, (2.0 / (C * k)) ** 0.5)
    Wr, WrT = torch.empty(C, k * C, dtype=bf16, device=DEV), torch.empty(k * C, C, dtype=bf16, device=DEV)
    ops.w2v_conv_weight_prep(W, Wr, WrT, C, C, k)
    res = []
    for fill in (0.0, SENT):
        act = pitched(xv, Pprev, SL, fill)
        out = torch.zeros(B * P + SL, C, dtype=bf16, device=DEV)
        pre = torch.zeros(B * P + SL, C, dtype=bf16, device=DEV)
        ops.gemm_nt(ops.EPI_GELU_BF16, act, Wr, out, B * P, C, k * C, lda=s * C, aux_out=pre, ldaux=C)
        res.append((frames_of(out, B, P, T).clone(), frames_of(pre, B, P, T).clone()))
    # the valid frames never read a filler row: bit-identical with zero and with sentinel filler
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    w64 = Wr.double().reshape(C, k, C).permute(0, 2, 1)                                       # the bf16 filter the GEMM reads, [co][ci][j]
    x64 = xv.double().transpose(1, 2)
    ref = F.conv1d(x64, w64, stride=s).transpose(1, 2)                                        # [B, T, C]
    S_abs = F.conv1d(x64.abs(), w64.abs(), stride=s).transpose(1, 2)
    # fp32 accumulation over k*C products in MFMA blocks: chain <= k*C / 16 + 4
    acc = (k * C / 16 + 4) * U * S_abs
    check_bf16("conv fwd pre C%d k%d s%d B%d" % (C, k, s, B), res[1][1], ref, acc)
    check_bf16("conv fwd GELU", res[1][0], F.gelu(ref), acc * gelu_grad64(ref).abs() + 2e-7 * ref.abs())


@pytest.mark.parametrize("C", [128, 512])
@pytest.mark.parametrize("k,s,Pextra", [(3, 2, 0), (2, 2, 0), (3, 1, 0), (3, 2, 24), (3, 1, 16)])
@pytest.mark.parametrize("with_pre", [True, False])
def test_col2im_dgelu(C, k, s, Pextra, with_pre):
    """adjoint of the overlapping-row read: dpre_prev[tau] = GELU'(pre_prev[tau]) * sum_{j, t: s t + j = tau} dcol[t, j]; Pextra > 0 gives
    Pprev > s * Pl (frames no tap reaches)"""
    g = gen(C + k + s + Pextra)
    B, Tprev = 2, 211
    T, Pl, Pprev = layer_shapes(Tprev, k, s)
    Pprev += Pextra
    dv = randn((B, T, k * C), g, 1.0, bf16)
    dcol = pitched(dv, Pl, 0, 0.0)                        # a gradient buffer: filler rows are zeros by contract
    prev = randn((B, Tprev, C), g, 1.0, bf16)
    pre_prev = pitched(prev, Pprev, SL) if with_pre else None
    out = torch.full((B * Pprev + SL, C), SENT, dtype=bf16, device=DEV)
    ops.w2v_col2im_dgelu(dcol, pre_prev, out, B, Pl, Pprev, C, k, s)
    fold = torch.zeros(B, Pprev + k, C, dtype=f64, device=DEV)
    d64 = dv.double().reshape(B, T, k, C)
    for j in range(k):
        fold[:, j:j + s * T:s] += d64[:, :, j]
    fold = fold[:, :Tprev]
    if with_pre:
        gd = gelu_grad64(prev)
        ref, extra = fold * gd, fold.abs() * 4e-7
    else:
        ref, extra = fold, 0.0
    # at most k / s + 1 bf16 terms summed in fp32 (exact), one GELU' factor: 1 ulp (+ the GELU' error)
    check_bf16("col2im C%d k%d s%d +%d pre=%d" % (C, k, s, Pextra, with_pre), frames_of(out, B, Pprev, Tprev), ref, extra)
    assert (filler_of(out, B, Pprev, Tprev) == 0).all(), "filler frames of a gradient are exact zeros"
    assert (out[B * Pprev:].float() == SENT_BF).all(), "nothing written past the last clip"


def conv_dw_table(plan, C, conv_kernel, conv_stride, dpre, act, dWr):
    """the conv weight-gradient table of ClassificationWave2Vec._bwd_front, from the host plan"""
    probs = []
    for l in range(1, len(conv_kernel)):
        kk, ss = conv_kernel[l], conv_stride[l]
        for c_, (r0, n) in enumerate(plan.chunks[l]):
            probs.append((ops._pa(dpre[l], r0 * C), C, ops._pa(act[l - 1], r0 * ss * C), ss * C, ops._pa(dWr[l], c_ * C * kk * C), kk * C, 0,
                          C, kk * C, n))
    return ops.make_group_tn_desc_ld(probs, DEV, tile=256 if plan.pp else 128)


def conv_dw_ref(dpre_l, act_prev, B, P, Pprev, T, k, s, C):
    """float64 sum over the valid frames: dW[co, ci, j] = sum_{b, t < T} dpre[b, t, co] act[b, s t + j, ci]; also sum |terms|"""
    d = frames_of(dpre_l, B, P, T).double().reshape(B * T, C)
    a = act_prev[:B * Pprev].reshape(B, Pprev, C)[:, :s * (T - 1) + k].double()
    a = a.unfold(1, k, s)[:, :T].reshape(B * T, C, k)                                       # [rows, ci, j]
    ref = torch.einsum("rc,rij->cij", d, a)
    S_abs = torch.einsum("rc,rij->cij", d.abs(), a.abs())
    return ref, S_abs


@pytest.mark.parametrize("C,B,samples", [(128, 8, 16001), (256, 3, 16001), (512, 3, 16001)])
def test_conv_weight_gradients_through_the_chunk_table(C, B, samples):
    """the table _bwd_front builds (wave2vec.conv_dw_chunks), gemm_tn_grouped_f32 (pp on the persistent 256 x 256 kernel), w2v_conv_wgrad_add
    (dW +=).  C = 128: the 128-tile table with chunks of 12800 frames; C = 256 / 512: the persistent kernel.  Several chunks per layer with a
    partial last one in both."""
    cfg, T, P = conv_geometry(C, samples)
    nl = len(cfg.conv_kernel)
    plan = wave2vec.conv_dw_chunks(C, cfg.conv_kernel, B, P)
    assert plan.pp == (C != 128)
    assert len(plan.chunks[1]) > 1 and plan.chunks[1][-1][1] < plan.CH, "layer 1 needs several chunks and a partial last one"
    g = gen(C + B)
    act = [pitched(randn((B, T[l], C), g, 1.0, bf16), P[l], SL) for l in range(nl)]
    dpre = [None] + [pitched(randn((B, T[l], C), g, 1.0, bf16), P[l], SL, 0.0) for l in range(1, nl)]
    dWr = [None] + [torch.full((len(plan.chunks[l]), C, cfg.conv_kernel[l] * C), SENT, dtype=f32, device=DEV) for l in range(1, nl)]
    desc, npb, ntiles, flops, nbytes = conv_dw_table(plan, C, cfg.conv_kernel, cfg.conv_stride, dpre, act, dWr)
    ops.gemm_tn_grouped_f32(desc, npb, ntiles, alpha=1.0, beta=0.0, flops=flops, nbytes=nbytes, pp=plan.pp)
    for l in range(1, nl):
        kk, ss = cfg.conv_kernel[l], cfg.conv_stride[l]
        dW0 = randn((C, C, kk), g)
        dW = dW0.clone()
        ops.w2v_conv_wgrad_add(dWr[l], dW, C, C, kk, len(plan.chunks[l]))
        ref, S_abs = conv_dw_ref(dpre[l], act[l - 1], B, P[l], P[l - 1], T[l], kk, ss, C)
        # fp32: MFMA accumulation over one chunk (chain <= CH / 16 + 4), then n_part partials and the += in wgrad_add
        L = plan.CH / 16 + 4 + len(plan.chunks[l]) + 1
        check("conv dW C%d B%d layer %d (%d chunks)" % (C, B, l, len(plan.chunks[l])), dW, dW0.double() + ref,
              L * U * S_abs + 2 * U * dW0.double().abs())


# ---- feature LayerNorm ----------------------------------------------------------------------------------------------------------------
def ln_xhat_err(xh, rs, D):
    """bound on |xhat_kernel - xhat| of a wave-per-row LayerNorm over D values: fp32 mean and centered variance (D / 64 sequential adds per lane
    + a 6-level butterfly) within (D / 64 + 8) u relative each, rsqrt within 2 ulp"""
    e = (D / 64 + 8) * U
    return 4 * e * (1.0 + xh.abs()) + 4 * U * xh.abs()


@pytest.mark.parametrize("C", [128, 256, 512, 768])
def test_featln_forward_and_backward(C):
    g = gen(C)
    B, T, eps = 3, 37, 1e-5
    P = rup(T + 1, 8)
    M = B * P
    xv = (randn((B, T, C), g) + 0.5).to(bf16)
    x = pitched(xv, P, SL)
    gamma, beta = (1.0 + 0.3 * torch.randn(C, generator=g)).float().to(DEV), (0.3 * torch.randn(C, generator=g)).float().to(DEV)
    out = torch.full((M, C), SENT, dtype=bf16, device=DEV)
    st = torch.full((2, M), SENT, dtype=f32, device=DEV)
    ops.w2v_featln_fwd(x, gamma, beta, eps, out, st[0], st[1], B, T, P, C)
    x64 = xv.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.layer_norm(x64, (C,), g64, b64, eps)
    with torch.no_grad():
        mu, rs = x64.mean(-1), (x64.var(-1, unbiased=False) + eps).rsqrt()
        xh = (x64 - mu[..., None]) * rs[..., None]
        xe = ln_xhat_err(xh, rs[..., None], C)
    check_bf16("featln out C%d" % C, frames_of(out, B, P, T), y.detach(), xe * g64.abs())
    check("featln mean", frames_of(st[0][:, None], B, P, T)[..., 0], mu, (C / 64 + 8) * U * x64.abs().mean(-1) + 1e-30)
    check("featln rstd", frames_of(st[1][:, None], B, P, T)[..., 0], rs, 4 * (C / 64 + 8) * U * rs)
    assert (filler_of(out, B, P, T) == 0).all() and (filler_of(st.t(), B, P, T) == 0).all()
    # backward fused with the GELU' of the last conv layer: dpre = LN'(dy) * GELU'(pre)
    dyv, prev = randn((B, T, C), g, 1.0, bf16), randn((B, T, C), g, 1.0, bf16)
    dy, pre = pitched(dyv, P, 0), pitched(prev, P, SL)
    dpre = torch.full((M, C), SENT, dtype=bf16, device=DEV)
    dg0, db0 = randn(C, g), randn(C, g)
    dgam, dbet = dg0.clone(), db0.clone()
    ops.w2v_featln_bwd(dy, x, pre, st[0], st[1], gamma, dpre, dgam, dbet, B, T, P, C)
    y.backward(dyv.double())
    gd = gelu_grad64(prev)
    with torch.no_grad():
        d64 = dyv.double()
        dh = d64 * g64
        c1, c2 = dh.mean(-1, keepdim=True), (dh * xh).mean(-1, keepdim=True)
        mag = rs[..., None] * (dh.abs() + c1.abs() + (xh * c2).abs())
        # LN' from the saved fp32 statistics: xhat as above, c1 / c2 fp32 row sums (chain C / 64 + 8)
        e = mag * (xe.amax(-1, keepdim=True) * 2 + 2 * (C / 64 + 8) * U)
    check_bf16("featln dpre", frames_of(dpre, B, P, T), x64.grad * gd, e * gd.abs() + x64.grad.abs() * 4e-7)
    assert (filler_of(dpre, B, P, T) == 0).all()
    # dgamma / dbeta: 8 rows per wave, 4 waves, one fp32 atomic per workgroup: chain <= 32 + M / 32
    L = 32 + M / 32 + 2
    check("featln dgamma +=", dgam, dg0.double() + g64.grad, (L * U) * (d64 * xh).abs().sum((0, 1)) + (d64.abs() * xe).sum((0, 1)) + 2 * U * dg0.double().abs())
    check("featln dbeta +=", dbet, db0.double() + b64.grad, L * U * d64.abs().sum((0, 1)) + 2 * U * db0.double().abs())


# ---- SpecAugment ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["mask", "whole_clip", "empty", "none"])
def test_spec_mask_forward_and_backward(case):
    g = gen({"mask": 1, "whole_clip": 2, "empty": 3, "none": 4}[case])
    B, T, D, k = 3, 45, 384, 128
    P, Pp = rup(T + 1, 8), rup(T + k, 8)
    M = B * P
    m = torch.zeros(B, P, dtype=torch.uint8)
    if case in ("mask", "whole_clip"):
        m[:, :T] = (torch.rand(B, T, generator=g) < 0.3).to(torch.uint8)
        m[1] = 0                                                        # a clip without masked frames
    if case == "whole_clip":
        m[2, :T] = 1
    mask = m.reshape(-1).to(DEV)
    embed = randn(D, g)
    x0 = randn((M, D), g)
    x = x0.clone()
    if case != "none":
        ops.w2v_spec_mask_fwd(x, mask, embed, M, D)
        want = torch.where(mask.bool()[:, None], embed[None], x0)
        assert torch.equal(x, want)
    dxv = randn((B, T, D), g)
    dx = pitched(dxv, P, 0)
    addv = randn((B, T, D), g)
    add = pitched(addv, Pp, 8)                                          # the positional-conv input gradient, pitch Pp
    de0 = randn(D, g)
    dembed = de0.clone()
    ops.w2v_spec_mask_bwd(dx, add, mask if case != "none" else None, dembed if case != "none" else None, B, T, P, Pp, D)
    v = dxv.double() + addv.double()
    mk = m[:, :T].bool().to(DEV)
    check("spec_mask dx (%s)" % case, frames_of(dx, B, P, T), torch.where(mk[..., None], 0.0, v), U * v.abs())      # one fp32 add
    assert (filler_of(dx, B, P, T) == 0).all()
    if case == "none":
        assert torch.equal(dembed, de0)
        return
    vm = (v * mk[..., None])
    # 4 frame lanes of P / 4 sequential adds, 4 partials, one fp32 atomic per clip
    L = P / 4 + 4 + B + 2
    check("spec_mask dembed += (%s)" % case, dembed, de0.double() + vm.sum((0, 1)), L * U * vm.abs().sum((0, 1)) + 2 * U * de0.double().abs())
    if case == "empty":
        assert torch.equal(dembed, de0)


# ---- positional conv: staging, weight norm, the three grouped products, encoder input ---------------------------------------------------
@pytest.mark.parametrize("D,G,k", [(768, 16, 128), (768, 16, 15), (384, 8, 16), (128, 4, 15), (768, 8, 128)])
@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_pos_stage_is_a_bit_exact_padded_copy(D, G, k, direction):
    g = gen(D + G + k)
    B, T = 3, 29
    P, Pp = rup(T + 1, 8), rup(T + k, 8)
    cg = D // G
    rows_total = B * Pp + k + 8
    pad = k // 2 if direction == "fwd" else k - 1 - k // 2
    srcv = randn((B, T, D), g)
    src = pitched(srcv, P, SL)
    out = torch.full((G, rows_total, cg), SENT, dtype=bf16, device=DEV)
    ops.w2v_pos_stage(src, out, B, T, P, Pp, D, G, pad, rows_total)
    want = torch.zeros(G, rows_total, cg, dtype=bf16, device=DEV)
    w = want[:, :B * Pp].reshape(G, B, Pp, cg)
    w[:, :, pad:pad + T] = srcv.to(bf16).reshape(B, T, G, cg).permute(2, 0, 1, 3)
    assert torch.equal(out.view(torch.int16), want.view(torch.int16)), (D, G, k, direction)


def wn_ref(v, gk):
    """oracle.w2v2_ref.pos_conv_weight: w = g * v / ||v|| over dims (0, 1), float64 with autograd leaves"""
    v64, g64 = v.double().requires_grad_(True), gk.double().reshape(1, 1, -1).requires_grad_(True)
    w = WR.pos_conv_weight({"model.encoder.pos_conv_embed.conv.parametrizations.weight.original0": g64,
                            "model.encoder.pos_conv_embed.conv.parametrizations.weight.original1": v64})
    return v64, g64, w


def wn_operands(D, G, k, g):
    cg = D // G
    v = randn((D, cg, k), g, 0.05)
    gk = (torch.rand(k, generator=g, dtype=f64) + 0.5).float().to(DEV)
    norms = torch.empty(k, dtype=f32, device=DEV)
    Wf = torch.empty(G, cg, k * cg, dtype=bf16, device=DEV)
    Wb = torch.empty(G, cg, k * cg, dtype=bf16, device=DEV)
    ops.w2v_weightnorm_prep(v, gk, norms, Wf, Wb, D, G, k)
    return v, gk, norms, Wf, Wb


def wf_layout(w, G):
    """[D, cg, k] -> Wf [G][co_l][j][ci]"""
    D, cg, k = w.shape
    return w.reshape(G, cg, cg, k).permute(0, 1, 3, 2).reshape(G, cg, k * cg)


def wb_layout(w, G):
    """[D, cg, k] -> Wb [G][ci][j'][co_l] with j' = k - 1 - j (the tap-reversed transpose)"""
    D, cg, k = w.shape
    return w.reshape(G, cg, cg, k).flip(-1).permute(0, 2, 3, 1).reshape(G, cg, k * cg)


WN_CASES = [(128, 4, 16), (768, 16, 128), (768, 8, 128), (1024, 8, 128), (128, 4, 24)]     # three-pass, > 48 KiB LDS, single kernel (x 2)


@pytest.mark.parametrize("D,G,k", WN_CASES)
def test_weightnorm_prep_and_backward(D, G, k):
    g = gen(D * k + G)
    cg = D // G
    path = wn_path(D, G, k)
    v, gk, norms, Wf, Wb = wn_operands(D, G, k, g)
    v64, g64, w = wn_ref(v, gk)
    nref = v.double().norm(dim=(0, 1))
    check("wn norms D%d G%d k%d" % (D, G, k), norms, nref, (D * cg / 256 + 10) * U * nref)
    # w = g v / norm in fp32 then bf16: 1 ulp (+ the norm's relative error)
    dn = (D * cg / 256 + 10) * U
    check_bf16("wn Wf", Wf, wf_layout(w.detach(), G), (dn + 4 * U) * wf_layout(w.detach().abs(), G))
    w_bf = Wf.reshape(G, cg, k, cg).permute(0, 1, 3, 2).reshape(D, cg, k)                   # the rounded filter, [co][ci][j]
    assert torch.equal(Wb.view(torch.int16), wb_layout(w_bf, G).view(torch.int16)), "Wb is the tap-reversed transpose of Wf, bit for bit"
    # backward: dv +=, dg += from an fp32 dWf in the Wf layout
    dWf = randn((G, cg, k * cg), g)
    dv0, dg0 = randn((D, cg, k), g, 0.1), randn(k, g)
    dv, dgk = dv0.clone(), dg0.clone()
    ws = torch.full((ops.w2v_weightnorm_ws_floats(D, k),), SENT, dtype=f32, device=DEV)
    ops.w2v_weightnorm_bwd(dWf, v, gk, norms, dv, dgk, ws, D, G, k)
    dW = dWf.double().reshape(G, cg, k, cg).permute(0, 1, 3, 2).reshape(D, cg, k)           # [co][ci][j]
    w.backward(dW)
    wn_check(path, D, G, k, v, gk, norms, dW, dv, dgk, dv0, dg0, v64.grad, g64.grad.reshape(k))


def wn_path(D, G, k):
    """which backward srhip_w2v_weightnorm_bwd runs: three passes (256 % k == 0, k (cg + 1) + 256 floats of LDS within 64 KiB; above 48 KiB
    through the dynamic-LDS attribute) or the single kernel"""
    lds = (k * (D // G + 1) + 256) * 4
    return "single" if (256 % k or lds > 65536) else ("3pass>48K" if lds > 49152 else "3pass")


def wn_check(label, D, G, k, v, gk, norms, dW, dv, dgk, dv0, dg0, dv_grad, dg_grad):
    cg = D // G
    with torch.no_grad():
        nn_, v64, gg = norms.double(), v.double(), gk.double()
        dot = (dW * v64).sum((0, 1))
        S = (dW * v64).abs().sum((0, 1))
        dn = (D * cg / 256 + 10) * U                                  # relative error of the fp32 norm (wn_norm_kernel: D cg / 256 adds per lane)
        # chain of the per-tap dot: three-pass = cg k / 256 per thread + 256 / k partials, then 4 chains of D k / 4096 + 1024 / k partials;
        # single kernel = D cg / 256 per thread + the 8-step wave / workgroup reduction
        Ld = (cg * k / 256 + 256 / k + D * k / 4096 + 1024 / k + 8) if wn_path(D, G, k) != "single" else (D * cg / 256 + 12)
        e_dot = Ld * U * S + 2 * dn * dot.abs()
        sc = gg / nn_
        e_dv = sc * ((dn + 4 * U) * dW.abs() + v64.abs() * (e_dot + 3 * dn * dot.abs() + 4 * U * dot.abs()) / nn_ ** 2)
    check("wn dv += D%d G%d k%d (%s, %s)" % (D, G, k, wn_path(D, G, k), label), dv, dv0.double() + dv_grad, e_dv + 2 * U * (dv0.double().abs() + dv_grad.abs()))
    check("wn dg += (%s)" % label, dgk, dg0.double() + dg_grad, (e_dot + dn * dot.abs()) / nn_ + 2 * U * (dg0.double().abs() + dg_grad.abs()))


def test_weightnorm_backward_captures_into_a_graph_and_keeps_two_widths_apart():
    """the caller-owned workspace: the op captures into a torch.cuda.graph and the replay equals the eager call (the three-pass backward sums
    in a fixed order); two widths called alternately in one process each stay correct"""
    g = gen(11)
    D, G, k = 768, 16, 128
    cg = D // G
    v, gk, norms, Wf, Wb = wn_operands(D, G, k, g)
    dWf = randn((G, cg, k * cg), g)
    dv0, dg0 = randn((D, cg, k), g, 0.1), randn(k, g)
    ws = torch.empty(ops.w2v_weightnorm_ws_floats(D, k), dtype=f32, device=DEV)
    dv_e, dg_e = dv0.clone(), dg0.clone()
    ops.w2v_weightnorm_bwd(dWf, v, gk, norms, dv_e, dg_e, ws, D, G, k)
    dv_g, dg_g = dv0.clone(), dg0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                     # warm-up off the capture, as torch.cuda.graph asks
        ops.w2v_weightnorm_bwd(dWf, v, gk, norms, dv_g, dg_g, ws, D, G, k)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.w2v_weightnorm_bwd(dWf, v, gk, norms, dv_g, dg_g, ws, D, G, k)
    dv_g.copy_(dv0)
    dg_g.copy_(dg0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dv_g, dv_e) and torch.equal(dg_g, dg_e)
    # alternate two widths, each with its own workspace
    small = (128, 4, 16)
    v2, gk2, norms2, _, _ = wn_operands(*small, g)
    dWf2 = randn((small[1], small[0] // small[1], small[2] * small[0] // small[1]), g)
    ws2 = torch.empty(ops.w2v_weightnorm_ws_floats(small[0], small[2]), dtype=f32, device=DEV)
    for rep in range(2):
        for (DD, GG, kk), (vv, gg_, nn_, dd, ww) in [((D, G, k), (v, gk, norms, dWf, ws)), (small, (v2, gk2, norms2, dWf2, ws2))]:
            ccg = DD // GG
            dvx, dgx = torch.zeros(DD, ccg, kk, device=DEV), torch.zeros(kk, device=DEV)
            ops.w2v_weightnorm_bwd(dd, vv, gg_, nn_, dvx, dgx, ww, DD, GG, kk)
            v64, g64, w = wn_ref(vv, gg_)
            dW = dd.double().reshape(GG, ccg, kk, ccg).permute(0, 1, 3, 2).reshape(DD, ccg, kk)
            w.backward(dW)
            wn_check("alternating %d" % rep, DD, GG, kk, vv, gg_, nn_, dW, dvx, dgx, torch.zeros_like(dvx), torch.zeros_like(dgx),
                     v64.grad, g64.grad.reshape(kk))


def pos_geometry(D, G, k, B, T):
    P, Pp = rup(T + 1, 8), rup(T + k, 8)
    return P, Pp, B * Pp + k + 8


@pytest.mark.parametrize("D,G,k", [(128, 4, 16), (128, 4, 15), (768, 16, 128), (768, 16, 16), (768, 8, 15), (768, 8, 128)])
def test_positional_conv_three_products(D, G, k):
    """forward (gemm_nt_grouped_f32 on the n64 table for cg <= 64, else the 128 table), weight gradient with the bias (gemm_tn_grouped_f32),
    input gradient (tap-reversed Wb), each against F.conv1d(groups = G, padding = k // 2) under float64 autograd -- the last frame dropped for
    even k (oracle/w2v2_ref.py).  cg = 32 / 48 on the n64 table, 96 on the 128 table; k * cg is a multiple of the GEMM's 32-element k-step
    (W2vConfig; an odd k = 15 needs cg % 32 == 0)"""
    g = gen(D + G + k)
    B, T = 3, 53
    cg = D // G
    P, Pp, rows_total = pos_geometry(D, G, k, B, T)
    Kc = k * cg
    v, gk, norms, Wf, Wb = wn_operands(D, G, k, g)
    hv = randn((B, T, D), g)
    hidden = pitched(hv, P, SL)
    Xg = torch.zeros(G, rows_total, cg, dtype=bf16, device=DEV)
    ops.w2v_pos_stage(hidden, Xg, B, T, P, Pp, D, G, k // 2, rows_total)
    conv = torch.full((B * Pp + 8, D), SENT, dtype=f32, device=DEV)
    n64 = cg <= 64
    desc = ops.make_group_desc_ld([(ops._pa(Xg, gi * rows_total * cg), cg, ops._pa(Wf, gi * cg * Kc), Kc, ops._pa(conv, gi * cg), D, B * Pp, cg, Kc)
                                   for gi in range(G)], DEV, bn=64 if n64 else 128)
    d_, npb, ntiles, flops, nbytes = desc
    ops.gemm_nt_grouped_f32(d_, npb, ntiles, alpha=1.0, beta=0.0, flops=flops, nbytes=nbytes, n64=n64)
    # float64 reference on the operands the products read: bf16 hidden, the bf16 filter Wf
    x64 = hv.to(bf16).double().transpose(1, 2).requires_grad_(True)                           # [B, D, T]
    w64 = Wf.double().reshape(G, cg, k, cg).permute(0, 1, 3, 2).reshape(D, cg, k).requires_grad_(True)
    b64 = torch.zeros(D, dtype=f64, device=DEV, requires_grad=True)
    pc = F.conv1d(x64, w64, b64, padding=k // 2, groups=G)
    pc_abs = F.conv1d(x64.detach().abs(), w64.detach().abs(), padding=k // 2, groups=G)
    if k % 2 == 0:
        pc, pc_abs = pc[..., :-1], pc_abs[..., :-1]
    assert pc.shape[-1] == T
    L = Kc / 16 + 4                                                   # fp32 MFMA accumulation over k * cg products
    check("posconv fwd D%d G%d k%d (%s)" % (D, G, k, "n64" if n64 else "128"), frames_of(conv, B, Pp, T), pc.detach().transpose(1, 2),
          L * U * pc_abs.transpose(1, 2))
    # backward: dconv (fp32 rows, pitch P) -> staged with the backward pad -> dW (+ bias) and dX
    dcv = randn((B, T, D), g)
    dconv = pitched(dcv, P, 0)
    dYg = torch.zeros(G, rows_total, cg, dtype=bf16, device=DEV)
    padl = k - 1 - k // 2
    ops.w2v_pos_stage(dconv, dYg, B, T, P, Pp, D, G, padl, rows_total)
    dWf = torch.full((G, cg, Kc), SENT, dtype=f32, device=DEV)
    gb0 = randn(D, g)
    gb = gb0.clone()
    d_, npb, ntiles, flops, nbytes = ops.make_group_tn_desc_ld(
        [(ops._pa(dYg, (gi * rows_total + padl) * cg), cg, ops._pa(Xg, gi * rows_total * cg), cg, ops._pa(dWf, gi * cg * Kc), Kc,
          ops._pa(gb, gi * cg), cg, Kc, B * Pp) for gi in range(G)], DEV)
    ops.gemm_tn_grouped_f32(d_, npb, ntiles, alpha=1.0, beta=0.0, flops=flops, nbytes=nbytes)
    dxpos = torch.full((B * Pp + 8, D), SENT, dtype=f32, device=DEV)
    d_, npb, ntiles, flops, nbytes = ops.make_group_desc_ld(
        [(ops._pa(dYg, gi * rows_total * cg), cg, ops._pa(Wb, gi * cg * Kc), Kc, ops._pa(dxpos, gi * cg), D, B * Pp, cg, Kc) for gi in range(G)],
        DEV, bn=64 if n64 else 128)
    ops.gemm_nt_grouped_f32(d_, npb, ntiles, alpha=1.0, beta=0.0, flops=flops, nbytes=nbytes, n64=n64)
    dy64 = dcv.to(bf16).double().transpose(1, 2)                                              # the staged bf16 gradient
    pc.backward(dy64)
    wa = w64.detach().abs()
    with torch.no_grad():
        # sum |terms|: dW over B * T frames, dX over k * cg taps
        dW_abs = torch.nn.grad.conv1d_weight(x64.detach().abs(), w64.shape, F.pad(dy64.abs(), (0, 1)) if k % 2 == 0 else dy64.abs(),
                                             padding=k // 2, groups=G)
        dX_abs = torch.nn.grad.conv1d_input(x64.shape, wa, F.pad(dy64.abs(), (0, 1)) if k % 2 == 0 else dy64.abs(), padding=k // 2, groups=G)
    Lw = B * Pp / 16 + 4
    check("posconv dW", dWf.reshape(G, cg, k, cg).permute(0, 1, 3, 2).reshape(D, cg, k), w64.grad, Lw * U * dW_abs)
    bias_ref = b64.grad
    check("posconv dbias +=", gb, gb0.double() + bias_ref, Lw * U * dy64.abs().sum((0, 2)) + 2 * U * gb0.double().abs())
    check("posconv dX", frames_of(dxpos, B, Pp, T), x64.grad.transpose(1, 2), L * U * dX_abs.transpose(1, 2))


@pytest.mark.parametrize("D", [128, 384, 768])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_pos_finish_forward_and_backward(D, p):
    """encoder input: y = x + GELU(conv + b); x0 = dropout(LayerNorm(y)); the keep mask of oracle.w2v2_ref.pitched_keep(seed, SITE_EMB, ...)"""
    g = gen(D + int(p * 10))
    B, T, k, eps, seed = 3, 41, 128, 1e-5, 0x1234_5678_9ABC
    P, Pp = rup(T + 1, 8), rup(T + k, 8)
    M = B * P
    xv, cv = randn((B, T, D), g), randn((B, T, D), g)
    x, conv = pitched(xv, P, 0), pitched(cv, Pp, 8)
    cb, gamma, beta = randn(D, g, 0.3), (1.0 + 0.3 * torch.randn(D, generator=g)).float().to(DEV), randn(D, g, 0.3)
    drop = ops.Drop(seed, wave2vec.SITE_EMB, p) if p > 0 else None
    x0 = torch.full((M, D), SENT, dtype=f32, device=DEV)
    x0b = torch.full((M, D), SENT, dtype=bf16, device=DEV)
    ys = torch.full((M, D), SENT, dtype=f32, device=DEV)
    st = torch.full((2, M), SENT, dtype=f32, device=DEV)
    ops.w2v_pos_finish_fwd(x, conv, cb, gamma, beta, eps, x0, x0b, ys, st[0], st[1], B, T, P, Pp, D, drop)
    keep = torch.ones(B, T, D, dtype=f64, device=DEV)
    if p > 0:
        keep = torch.from_numpy(np.ascontiguousarray(WR.pitched_keep(seed, WR.SITE_EMB, (B, T, D), p, P))).to(DEV, f64) / (1.0 - p)
    x64, c64 = xv.double().requires_grad_(True), cv.double().requires_grad_(True)
    b64, g64, be64 = cb.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = c64 + b64
    y = x64 + F.gelu(z)
    ln = F.layer_norm(y, (D,), g64, be64, eps)
    out = ln * keep
    with torch.no_grad():
        gz = F.gelu(z)
        ey = U * (x64.abs() + 3 * gz.abs()) + 2e-7 * z.abs() + U * y.abs()                  # fp32 add of the A-S GELU
        mu, rs = y.mean(-1), (y.var(-1, unbiased=False) + eps).rsqrt()
        xh = (y - mu[..., None]) * rs[..., None]
        exh = ln_xhat_err(xh, rs[..., None], D) + rs[..., None] * (ey + ey.amax(-1, keepdim=True) * (1 + xh.abs()))
        e0 = keep * (exh * g64.abs()) + 2 * U * out.abs()
    check("posfin ysave D%d p%.1f" % (D, p), frames_of(ys, B, P, T), y.detach(), ey)
    check("posfin x0", frames_of(x0, B, P, T), out.detach(), e0)
    check_bf16("posfin x0 bf16", frames_of(x0b, B, P, T), out.detach(), e0)
    check("posfin mean", frames_of(st[0][:, None], B, P, T)[..., 0], mu, ey.amax(-1) + (D / 64 + 8) * U * y.abs().mean(-1))
    check("posfin rstd", frames_of(st[1][:, None], B, P, T)[..., 0], rs, rs * (4 * (D / 64 + 8) * U + 2 * rs * ey.amax(-1)))
    for buf in (x0, x0b, ys, st.t()):
        assert (filler_of(buf, B, P, T) == 0).all(), "filler frames of the encoder input are exact zeros"
    # backward: dx0 -> dy in place, dconv = dy * GELU'(conv + b), dgamma +=, dbeta +=
    dxv = randn((B, T, D), g)
    dx = pitched(dxv, P, 0)
    dconv = torch.full((M, D), SENT, dtype=f32, device=DEV)
    dg0, db0 = randn(D, g), randn(D, g)
    dgam, dbet = dg0.clone(), db0.clone()
    ops.w2v_pos_finish_bwd(dx, ys, conv, cb, st[0], st[1], gamma, dconv, dgam, dbet, B, T, P, Pp, D, drop)
    out.backward(dxv.double())
    with torch.no_grad():
        d = dxv.double() * keep
        dh = d * g64
        c1, c2 = dh.mean(-1, keepdim=True), (dh * xh).mean(-1, keepdim=True)
        mag = rs[..., None] * (dh.abs() + c1.abs() + (xh * c2).abs())
        dy_ref = x64.grad
        e_dy = mag * (2 * exh.amax(-1, keepdim=True) + 4 * (D / 64 + 8) * U) + 2 * U * dy_ref.abs()
        gd = gelu_grad64(z)
    check("posfin dy (in place)", frames_of(dx, B, P, T), dy_ref, e_dy)
    # dconv = dy * GELU'(conv + b): dy's bound through GELU', the A-S GELU' error, one fp32 rounding of conv + b (|GELU''| <= 0.4) and of the product
    check("posfin dconv", frames_of(dconv, B, P, T), c64.grad, e_dy * gd.abs() + dy_ref.abs() * (4e-7 + 0.5 * U * z.detach().abs() + 2 * U * gd.abs()))
    assert (filler_of(dx, B, P, T) == 0).all() and (filler_of(dconv, B, P, T) == 0).all()
    L = 32 + M / 32 + 2
    check("posfin dgamma +=", dgam, dg0.double() + g64.grad, L * U * (d * xh).abs().sum((0, 1)) + (d.abs() * exh).sum((0, 1)) + 2 * U * dg0.double().abs())
    check("posfin dbeta +=", dbet, db0.double() + be64.grad, L * U * d.abs().sum((0, 1)) + 2 * U * db0.double().abs())


# ---- in situ: the plans of a real backward at the benchmark's shape and at an odd one ---------------------------------------------------
@pytest.mark.parametrize("B,samples", [(8, 64000), (3, 16001)])
def test_front_end_plans_in_situ(B, samples):
    """wave2vecv2_base forward_features(save = True) + backward; then the conv-layer, feature-projection and positional-conv weight gradients are
    recomputed in float64 from the engine's own saved operands (ctx.f and the _bwd_front buffers) and compared in full: chunks, slabs, pads and
    pitches at the shapes where they actually split."""
    torch.manual_seed(0)
    model = wave2vec.wave2vecv2_base(num_classes=2, device=DEV, seed=3)
    model.eval()                                                      # no dropout / SpecAugment / LayerDrop: the plans are what is checked
    cfg = model.cfg
    C, D, G, k, nl = cfg.conv_dim[0], cfg.hidden, cfg.pos_groups, cfg.pos_k, len(cfg.conv_kernel)
    cg = D // G
    wave = torch.randn(B, samples, generator=gen(B), dtype=f32).to(DEV)
    logits, feat, ctx = model.forward_features(wave, None, save=True)
    model.zero_grad()                                                 # the front end accumulates into the gradient block
    dl = torch.randn(B, cfg.num_classes, generator=gen(5), dtype=f32).to(DEV)
    model.backward(ctx, dl)
    torch.cuda.synchronize()
    f = ctx.f
    t = model._bwd_front(B, f)
    T, P, Pp = f.T, f.P, f.Pp
    plan = wave2vec.conv_dw_chunks(C, cfg.conv_kernel, B, P)
    assert t.dW_parts[1:] == [len(c) for c in plan.chunks[1:]]
    if samples == 64000:
        assert len(plan.chunks[1]) > 1 and len(plan.chunks[3]) > 1 and plan.chunks[3][-1][1] < plan.CH
    for l in range(1, nl):
        kk, ss = cfg.conv_kernel[l], cfg.conv_stride[l]
        assert (filler_of(t.dpre[l], B, P[l], T[l]) == 0).all()
        ref, S_abs = conv_dw_ref(t.dpre[l], f.act[l - 1], B, P[l], P[l - 1], T[l], kk, ss, C)
        got = model.view(wave2vec.FE + "%d.conv.weight" % l, model.grad)
        L = plan.CH / 16 + 4 + len(plan.chunks[l]) + 1
        check("in situ B%d conv dW layer %d" % (B, l), got, ref, L * U * S_abs)
        del ref, S_abs
    # feature projection: token slices of 256 through slabs, then the slab reduction
    M = B * P[-1]
    gp, lb = t.gproj.double(), f.lnb.double()
    ref = gp.t() @ lb
    S_abs = gp.abs().t() @ lb.abs()
    nsl = -(-M // 256)
    L = 256 / 16 + 4 + nsl + 1
    check("in situ B%d proj dW" % B, model.view(wave2vec.M_ + "feature_projection.projection.weight", model.grad), ref, L * U * S_abs)
    check("in situ proj db", model.view(wave2vec.M_ + "feature_projection.projection.bias", model.grad), gp.sum(0), L * U * gp.abs().sum(0))
    # positional conv: dWf from the staged dYg (backward pad) and Xg, its bias, then v / g through the float64 weight-norm backward
    padl = k - 1 - k // 2
    R = B * Pp
    dYg, Xg = t.dYg.double(), f.Xg.double()
    dWf_ref = torch.empty(G, cg, k, cg, dtype=f64, device=DEV)
    dWf_abs = torch.empty_like(dWf_ref)
    for gi in range(G):
        a = dYg[gi, padl:padl + R]                                                             # [R, co]
        xs = Xg[gi].unfold(0, k, 1)[:R]                                                        # [R, ci, j]
        dWf_ref[gi] = torch.einsum("rc,rij->cji", a, xs)
        dWf_abs[gi] = torch.einsum("rc,rij->cji", a.abs(), xs.abs())
    Lw = R / 16 + 4
    check("in situ B%d posconv dWf" % B, t.dWf.reshape(G, cg, k, cg), dWf_ref, Lw * U * dWf_abs)
    gb = model.view(wave2vec.PC + "bias", model.grad)
    bias_ref = dYg[:, padl:padl + R].sum(1).reshape(D)
    check("in situ posconv dbias", gb, bias_ref, Lw * U * dYg[:, padl:padl + R].abs().sum(1).reshape(D))
    v = model.view(wave2vec.PC + "parametrizations.weight.original1")
    gk = model.view(wave2vec.PC + "parametrizations.weight.original0").reshape(k)
    v64, g64, w = wn_ref(v, gk)
    dW = t.dWf.double().reshape(G, cg, k, cg).permute(0, 1, 3, 2).reshape(D, cg, k)
    w.backward(dW)
    z_dv, z_dg = torch.zeros_like(v), torch.zeros_like(gk)
    wn_check("in situ B%d" % B, D, G, k, v, gk, model.pos_norms, dW, model.view(wave2vec.PC + "parametrizations.weight.original1", model.grad),
             model.view(wave2vec.PC + "parametrizations.weight.original0", model.grad).reshape(k), z_dv, z_dg, v64.grad, g64.grad.reshape(k))
