"""The cases of tests/test_{cpu,gpu}_wrn_cases.py: every kernel of csrc/wrn_conv.hip, csrc/wrn_ops.hip and csrc/wrn_bn.h element by element
against float64.  Nothing is stored: every input is rebuilt from its seed, every expected value is recomputed.

Why element by element: tests/test_gpu_wrn.py holds this family to whole-tensor norms (1e-5 .. 3e-6 on blocks, 4e-2 on network gradients), to
other HIP kernels that share the BatchNorm arithmetic "operation for operation", and to model-level bit-equality of two paths that share their
pass indexing.  A norm moves by 1 / sqrt(rows) when one row is wrong; an error both sides share cannot show at all.
tests/test_cpu_wrn_cases.py plants twelve such faults in the float32 restatement and shows verify() rejecting each.

Convolution (srhip_wrn_conv_bn_passes).  Inputs: fp32 x from a PCG64 stream; channel 0 is shifted far from zero (mean / std about 30: the
statistics path), channel 1 is constant (the variance clamp), channel 2 has gamma = beta = 0 (every element on the LeakyReLU kink), channel 3 has
gamma < 0; the border pixels of image 0 of every pass are spiked, so a tap that wraps into the neighbouring row or image moves an output by far
more than any bound.  The filter operand is built here in the tap-major bf16 layout with zero padding columns K .. Kpad (the kernel's contract).
Every tensor lives inside a larger allocation at a 16-byte-aligned non-zero offset (FRONT elements); the surroundings of what a launch reads are
NaN, the surroundings of what it writes hold PATTERN and must come back bit for bit; y starts as NaN; some copies of acc_out start with exactly
representable non-zero contents.

Bound of an output element (never a norm).  The activation a is built in float64 from x and the float64 statistics (mode 3: from the in_acc built
here).  r = C_R 2^-24 (|gamma| |x - mu| invstd + |beta|) + |gamma| invstd |fp32(mu) - mu| is the fp32 error radius of that arithmetic (the
kernels round the mean to fp32 once: that amount is known, the measured constant covers the four operations and the invstd); any bf16 value
that some number in [a - r, a + r] (mapped through the LeakyReLU, which is monotone) rounds to is admissible, w = the width of the admissible
set (0 for all but the elements near a rounding tie or the kink).  want = conv64(bf16_rne(a), W) + resid and
    tol = C_ACC 2^-24 conv(|a|, |W|) + conv(w, |W|) + 2^-23 |want| + 2^-24 |resid|.
At most 1 % of the activation elements of a case may have w > 0 and at least 80 % of its output elements carry no operand term (a cap on the
cases, asserted for every case on the CPU).  With r eight times its measurement an element has w > 0 at a rate near 1e-3, so an output that
sums K = 288 elements or more cannot meet the cap: those convolutions (every split-K template among them: KS > 1 needs K >= 256) read raw
input (mode 2, r = 0) or are the input-gradient form, which is mode 2 by definition.  For the same reason beta is small against gamma (beta
cancelling most of gamma xhat widens r relative to a) and, where the input goes through the BatchNorm, the spikes sit in one channel (they inflate that channel's batch variance); the
cases that read raw input spike every channel from 4 on.
Statistics: acc_out folded over its 16 copies, minus what was there, against the float64 sums of the y the launch STORED, within
C_SUM 2^-24 sum |y| (sum y^2); published mean within one rounding of float64; invstd and the running statistics restated as bn_finalize states
them (one fp64 fma for the variance, fp32 steps without contraction) bit for bit, differences of one ulp allowed and counted.

The other kernels, one class each below (inputs, run_hip, the float32 restatement, expect / verify with its bound written out): HeadLaunch
(srhip_wrn_head_passes), BnLaunch (bn_accumulate, bn_fold, bn_stats, bn_fwd, bn_act), BwdLaunch (bn_bwd_reduce / _apply / bn_bwd, one rank and two
simulated ranks), ImLaunch (im2col, im2col_bn, col2im), WeightLaunch (the three filter layouts and add_unpad: the same bits as a numpy statement),
FcLaunch, PoolLaunch (avgpool_fwd / _bwd, nchw_to_nhwc_bf16), SgdLaunch.

C_ACC, C_R, C_SUM, C_BWD, C_SGD are measured on float32 restatements against float64 (measure_*), times 8 -- the margin the GEMM and rewarder
tests give a float32 restatement.  They are never set from what a kernel produced: a kernel outside the bound is a finding.  The other bounds are
worst-case counts of fp32 roundings, written where they are used."""
import functools
import math
from fractions import Fraction

import numpy as np
import torch

from semireward_amd import ops

# measured by measure_c_acc / measure_c_r / measure_c_sum / measure_c_bwd / measure_c_sgd (tests/test_cpu_wrn_cases.py holds each constant between
# 4 and 16 times its fresh measurement)
C_ACC_MEASURED, C_R_MEASURED, C_SUM_MEASURED, C_BWD_MEASURED, C_SGD_MEASURED = 3.762, 4.501, 2.108, 2.567, 2.017
C_ACC, C_R, C_SUM, C_BWD, C_SGD = (8.0 * v for v in (C_ACC_MEASURED, C_R_MEASURED, C_SUM_MEASURED, C_BWD_MEASURED, C_SGD_MEASURED))

FRONT = 64                          # elements before the first and after the last of every tensor
PATTERN = 0x4B1D                    # every 16 bits around what a launch writes: finite as bf16, fp32 and fp64
EPS, SLOPE, MOMENTUM = np.float32(1e-3), np.float32(0.1), np.float32(0.001)
U24, U23 = 2.0 ** -24, 2.0 ** -23
COPIES = 16                         # BN_COPIES of csrc/wrn_bn.h
WS_COUNTER, WS_ACC = 512, 520       # csrc/wrn_bn.h: ws layout in doubles


def _rng(*key):
    return np.random.Generator(np.random.PCG64([int(k) for k in key]))


def bf16_rne(a):
    """float array -> the round-to-nearest-even bf16 values, as float64"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)
    return t.double().numpy()


def to_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


def bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def ulps32(a, b):
    """distance in units of the last place between two float32 arrays of one sign pattern (numpy)"""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


# ---- allocations with poisoned surroundings -----------------------------------------------------------------------------------------------
class Arena:
    """Tensors of one launch on ``device``: read(name, t) places t between NaN, write(name, t) between PATTERN (t = the contents before the launch)."""

    def __init__(self, device):
        self.device, self.w, self.v = device, {}, {}

    def _mk(self, name, t, nan):
        t = torch.as_tensor(t)
        n = t.numel()
        buf = torch.empty(n + 2 * FRONT, dtype=t.dtype, device=self.device)
        if nan:
            buf.fill_(float("nan"))
        else:
            buf.view(torch.int16).fill_(PATTERN)
        view = buf[FRONT:FRONT + n].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 0
        self.v[name] = view
        return buf, view

    def read(self, name, t):
        return self._mk(name, t, True)[1]

    def write(self, name, t):
        buf, view = self._mk(name, t, False)
        self.w[name] = (buf, view.numel())
        return view

    def __getitem__(self, name):
        return self.v[name]

    def surroundings_touched(self):
        bad = []
        for name, (buf, n) in self.w.items():
            b = buf.view(torch.int16)
            e = buf.element_size() // 2
            for part in (b[:FRONT * e], b[(FRONT + n) * e:]):
                if not bool((part == PATTERN).all()):
                    bad.append(name)
        return sorted(set(bad))


def nan_like(shape, dtype=torch.float32):
    return torch.full(tuple(shape), float("nan"), dtype=dtype)


def worst(name, got, want, tol):
    """every element of got within tol of want (float64 numpy) and finite -> max |got - want| / tol; AssertionError naming the worst element"""
    got, want, tol = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(tol, dtype=np.float64)
    tol = np.broadcast_to(tol, want.shape)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = np.abs(got - want)
    ok = err <= tol                                           # (NaN compares false)
    if not ok.all():
        over = np.where(np.isfinite(err), err - tol, np.inf)
        i = np.unravel_index(int(np.argmax(over)), over.shape)
        raise AssertionError("%s: worst element %s: got %.9g want %.9g |diff| %.3e tol %.3e (%d of %d outside)" % (
            name, tuple(int(j) for j in i), got[i], want[i], err[i], tol[i], int((~ok).sum()), got.size))
    nz = tol > 0
    return float((err[nz] / tol[nz]).max()) if nz.any() else 0.0


# ---- float64 references ------------------------------------------------------------------------------------------------------------------------
def out_hw(H, W, k, s):
    pad = k >> 1
    return (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1


def im2col_ref(a, k, s):
    """a [B, H, W, C] -> col [B * Ho * Wo, k * k * C], tap-major K axis ((i * k + j) * C + c), zeros outside the image"""
    B, H, W, C = a.shape
    pad = k >> 1
    Ho, Wo = out_hw(H, W, k, s)
    ap = np.zeros((B, H + 2 * pad, W + 2 * pad, C), dtype=a.dtype)
    ap[:, pad:pad + H, pad:pad + W] = a
    col = np.empty((B, Ho, Wo, k * k, C), dtype=a.dtype)
    for i in range(k):
        for j in range(k):
            col[:, :, :, i * k + j] = ap[:, i:i + s * (Ho - 1) + 1:s, j:j + s * (Wo - 1) + 1:s]
    return col.reshape(B * Ho * Wo, k * k * C)


def col2im_ref(d, B, H, W, C, k, s):
    """the adjoint of im2col_ref: d [B * Ho * Wo, k * k * C] -> [B, H, W, C]"""
    pad = k >> 1
    Ho, Wo = out_hw(H, W, k, s)
    d = d.reshape(B, Ho, Wo, k * k, C)
    ap = np.zeros((B, H + 2 * pad, W + 2 * pad, C), dtype=d.dtype)
    for i in range(k):
        for j in range(k):
            ap[:, i:i + s * (Ho - 1) + 1:s, j:j + s * (Wo - 1) + 1:s] += d[:, :, :, i * k + j]
    return ap[:, pad:pad + H, pad:pad + W].copy()


def conv_ref(a, Wt, k, s):
    """a [B, H, W, Cin] float64, Wt [Cout, k * k * Cin] tap-major -> [B * Ho * Wo, Cout]"""
    return im2col_ref(a, k, s) @ Wt.T


def tap_major(Wf):
    """W [Cout, C, k, k] -> [Cout, k * k * C] in col's K order (conv_weight_prep's layout without the padding)"""
    Cout, C, k, _ = Wf.shape
    return np.ascontiguousarray(Wf.transpose(0, 2, 3, 1).reshape(Cout, k * k * C))


def prep_ref(Wf, Kpad):
    """numpy statement of conv_weight_prep: (Wb bf16 [Cout, Kpad], WbT bf16 [Kpad, Cout]) as torch tensors"""
    Cout = Wf.shape[0]
    t = tap_major(Wf)
    Wb = np.zeros((Cout, Kpad), dtype=np.float32)
    Wb[:, :t.shape[1]] = t
    Wb = to_bf16(Wb)
    return Wb, Wb.t().contiguous()


def flip_ref(Wf, Kpad):
    """numpy statement of conv_weight_flip_grouped: W [Cout, Cin, 3, 3] -> W' bf16 [Cin, Kpad], W'[ci][(8 - t) * Cout + co] = W[co][ci][t]"""
    Cout, Cin = Wf.shape[:2]
    t = Wf.reshape(Cout, Cin, 9)[:, :, ::-1]                       # [co, ci, 8 - t]
    out = np.zeros((Cin, Kpad), dtype=np.float32)
    out[:, :9 * Cout] = t.transpose(1, 2, 0).reshape(Cin, 9 * Cout)
    return to_bf16(out)


def unpad_ref(src, Cout, C, kk, Kpad):
    """numpy statement of add_unpad's gather: dWpad [Cout, Kpad] (tap-major) -> [Cout, C, kk]"""
    return np.ascontiguousarray(src[:, :kk * C].reshape(Cout, kk, C).transpose(0, 2, 1))


def fold_copies(acc):
    """[..., COPIES, n] doubles -> [..., n]: added in the kernels' order"""
    t = np.zeros(acc.shape[:-2] + acc.shape[-1:], dtype=np.float64)
    for q in range(COPIES):
        t = t + acc[..., q, :]
    return t


def _fma64(a, b, c):
    """round(a * b + c) with one rounding, elementwise on float64 arrays"""
    out = np.empty(a.shape, dtype=np.float64)
    for i in np.ndindex(a.shape):
        out[i] = float(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return out


def finalize_ref(s1, s2, rows, eps, running=None, momentum=MOMENTUM):
    """bn_finalize of csrc/wrn_bn.h in numpy: (mean, invstd, running_mean, running_var) float32 from the folded fp64 sums; the variance is one
    fp64 fma, every fp32 step is rounded on its own."""
    m = s1 / float(rows)
    v = _fma64(-m, m, s2 / float(rows))
    vc = np.where(v > 0.0, v, 0.0)
    mu, var = m.astype(np.float32), vc.astype(np.float32)
    isd = (np.float32(1.0) / np.sqrt((var + np.float32(eps)).astype(np.float32))).astype(np.float32)
    if running is None:
        return mu, isd, None, None
    unb = (vc * (float(rows) / float(rows - 1 if rows > 1 else 1))).astype(np.float32)
    one_m = np.float32(np.float32(1.0) - np.float32(momentum))
    rm = ((one_m * running[0]).astype(np.float32) + (np.float32(momentum) * mu).astype(np.float32)).astype(np.float32)
    rv = ((one_m * running[1]).astype(np.float32) + (np.float32(momentum) * unb).astype(np.float32)).astype(np.float32)
    return mu, isd, rm, rv


def lrelu(y, slope=SLOPE):
    return np.where(y > 0, y, float(slope) * y)


def act_ref(x, mu, isd, gamma, beta, raw=False):
    """The activation in float64 and its admissible bf16 set: dict(a, abf, lo, hi, w, r, yv).  mu / isd / gamma / beta float64 per channel."""
    x = x.astype(np.float64)
    if raw:
        abf = bf16_rne(x)
        z = np.zeros_like(x)
        return dict(a=x, abf=abf, lo=abf, hi=abf, w=z, r=z, yv=x)
    yv = gamma * ((x - mu) * isd) + beta
    dmu = np.abs(mu.astype(np.float32).astype(np.float64) - mu)            # the kernels round the mean to fp32 once: a known amount, no constant
    r = C_R * U24 * (np.abs(gamma) * np.abs(x - mu) * isd + np.abs(beta)) + np.abs(gamma) * isd * dmu
    a = lrelu(yv)
    alo, ahi = lrelu(yv - r), lrelu(yv + r)
    alo = np.where(r > 0, alo - U24 * np.abs(alo), alo)           # (the product with the slope is one more rounding)
    ahi = np.where(r > 0, ahi + U24 * np.abs(ahi), ahi)
    lo, hi = bf16_rne(alo), bf16_rne(ahi)
    return dict(a=a, abf=bf16_rne(a), lo=lo, hi=hi, w=hi - lo, r=r, yv=yv)


def act32(x, mu, isd, gamma, beta, slope=SLOPE, fma=False):
    """bn_apply_kernel's arithmetic in float32 (numpy rounds every operation; fma: the last product and sum contracted)"""
    t = ((x - mu).astype(np.float32) * isd).astype(np.float32)
    if fma:
        yv = (gamma.astype(np.float64) * t.astype(np.float64) + beta.astype(np.float64)).astype(np.float32)
    else:
        yv = ((gamma * t).astype(np.float32) + beta).astype(np.float32)
    return np.where(yv > 0, yv, (np.float32(slope) * yv).astype(np.float32)).astype(np.float32), yv


def planted_x(rng, shape, whole=False):
    """fp32 [..., images, H, W, C] with the planted channels and the spiked border of image 0.  whole: every channel from 4 on is spiked (the
    inputs read raw, mode 2); otherwise channel 4 alone: the spikes inflate the batch variance of their channel, where beta then cancels most
    of the activation and widens r relative to it"""
    x = rng.standard_normal(shape, dtype=np.float32)
    x[..., 0] += np.float32(30.0)
    x[..., 1] = np.float32(0.75)
    if shape[-1] > 4 and len(shape) >= 4:
        img = x[..., 0, :, :, 4:] if whole else x[..., 0, :, :, 4:5]
        sp = np.float32(48.0) * np.sign(img)
        img[..., 0, :, :] = sp[..., 0, :, :]
        img[..., -1, :, :] = sp[..., -1, :, :]
        img[..., :, 0, :] = sp[..., :, 0, :]
        img[..., :, -1, :] = sp[..., :, -1, :]
    return x


def planted_affine(rng, C):
    gamma = rng.uniform(0.75, 1.25, C).astype(np.float32)
    beta = (0.05 * rng.standard_normal(C)).astype(np.float32)
    if C > 3:
        gamma[2] = 0.0
        beta[2] = 0.0
        gamma[3] = -gamma[3]
    return gamma, beta


def split_copies(rng, s):
    """[..., n] doubles -> [..., COPIES, n] whose fold_copies is close to s (the fold of what is returned is what the launch reads)"""
    wts = rng.uniform(0.2, 1.0, (COPIES,) + (1,) * 0)
    wts = wts / wts.sum()
    return np.stack([s * wts[q] for q in range(COPIES)], axis=-2)


# ---- convolution cases -------------------------------------------------------------------------------------------------------------------------
DIRECT, TILE = "wrn_conv_kernel<%d, %d>", "wrn_conv_tile_kernel<%d, %d>"


def _conv(cid, shape, kernel, mode, rounds=1, resid=False, acc=None, publish=False, running=False, ranks=1, flip=False, seed=0):
    """acc: None | 'zero' | 'add' (some copies start non-zero).  flip: the fused input-gradient form (mode 2, the filter of
    conv_weight_flip_grouped; shape is the LAUNCH's: Cin = the forward layer's Cout)."""
    assert not (publish and mode != 3) and not (running and not publish) and not (flip and (mode != 2 or shape[5] != 3 or shape[6] != 1))
    assert shape[7] == 1 or mode in (2, 3)
    return dict(id=cid, shape=shape, kernel=kernel, mode=mode, rounds=rounds, resid=resid, acc=acc, publish=publish, running=running, ranks=ranks,
                flip=flip, seed=seed)


CONV_CASES = (
    # ---- the direct kernel: all nine templates
    _conv("d11-ragged35", (1, 5, 7, 8, 16, 3, 1, 1), DIRECT % (1, 1), 0, resid=True, acc="zero", seed=1),
    _conv("d11-1x1s2", (3, 5, 7, 8, 16, 1, 2, 1), DIRECT % (1, 1), 1, acc="add", seed=2),
    _conv("d21", (2, 6, 6, 16, 32, 3, 1, 1), DIRECT % (2, 1), 3, resid=True, acc="add", publish=True, running=True, seed=3),
    _conv("d42-18px", (2, 6, 6, 32, 64, 3, 2, 1), DIRECT % (4, 2), 2, acc="zero", seed=4),
    _conv("d24-flip", (5, 9, 9, 64, 32, 3, 1, 1), DIRECT % (2, 4), 2, flip=True, seed=5),
    _conv("d44-gy4-9px", (1, 3, 3, 128, 256, 3, 1, 1), DIRECT % (4, 4), 2, resid=True, acc="add", seed=6),
    _conv("d44-s2-oddH", (2, 17, 17, 128, 128, 3, 2, 1), DIRECT % (4, 4), 2, acc="zero", seed=7),
    _conv("d11-rounds2-64p", (2, 24, 24, 16, 16, 3, 1, 64), DIRECT % (1, 1), 3, rounds=2, resid=True, acc="add", publish=True, running=True, seed=8),
    _conv("d41-64p-cin8", (2, 10, 10, 8, 64, 3, 1, 64), DIRECT % (4, 1), 3, acc="zero", publish=True, ranks=2, seed=9),
    _conv("d12-flip", (2, 6, 6, 32, 16, 3, 1, 1), DIRECT % (1, 2), 2, flip=True, resid=True, seed=10),
    _conv("d14-flip", (2, 6, 6, 64, 16, 3, 1, 1), DIRECT % (1, 4), 2, flip=True, seed=11),
    _conv("d22", (2, 6, 6, 32, 32, 3, 1, 1), DIRECT % (2, 2), 2, acc="add", seed=12),
    # the BatchNorm prologue on channels 32 .. 127 of the direct kernel (1 x 1: K = Cin keeps the operand term within its cap)
    _conv("d41-1x1-cin128-bn", (2, 6, 6, 128, 64, 1, 1, 1), DIRECT % (4, 1), 3, resid=True, acc="add", publish=True, running=True, seed=26),
    _conv("d11-1x1s2-cin64-m1", (3, 5, 7, 64, 16, 1, 2, 1), DIRECT % (1, 1), 1, acc="zero", seed=27),
    # ---- the tile kernel: all six templates
    _conv("t21-8x8-odd", (3, 8, 8, 16, 32, 3, 1, 1), TILE % (2, 1), 0, resid=True, acc="add", seed=213),     # (seed 13 left
    # 75 % of these 192 x 32 outputs without an operand term: the cap is a condition on the case, so the case draws other inputs)
    _conv("t22-8x8-pair", (2, 8, 8, 16, 32, 3, 1, 1), TILE % (2, 2), 1, acc="zero", seed=14),
    _conv("t41-s2-into8", (3, 16, 16, 64, 128, 3, 2, 1), TILE % (4, 1), 2, resid=True, acc="add", seed=15),
    _conv("t41-1x1s2-lds61200", (2, 16, 16, 128, 128, 1, 2, 1), TILE % (4, 1), 3, acc="zero", publish=True, running=True, seed=16),
    _conv("t42-8x8-cin128", (4, 8, 8, 128, 128, 3, 1, 1), TILE % (4, 2), 2, acc="zero", seed=17),
    _conv("t22-tw16-16x48", (1, 16, 48, 16, 32, 3, 1, 1), TILE % (2, 2), 3, resid=True, acc="add", publish=True, ranks=2, seed=18),
    _conv("t42-tw32-s2-64x64", (1, 64, 64, 16, 64, 3, 2, 1), TILE % (4, 2), 3, acc="zero", publish=True, seed=19),
    _conv("t22-flip-tw16", (2, 16, 16, 64, 32, 3, 1, 1), TILE % (2, 2), 2, flip=True, seed=20),
    _conv("t24-64p", (4, 32, 32, 16, 32, 3, 1, 64), TILE % (2, 4), 3, resid=True, acc="add", publish=True, running=True, seed=21),
    _conv("t24-1x1-64p", (4, 32, 32, 16, 32, 1, 1, 64), TILE % (2, 4), 2, acc="zero", seed=22),
    _conv("t44-32p", (8, 32, 32, 16, 64, 3, 1, 32), TILE % (4, 4), 3, acc="add", publish=True, ranks=2, seed=23),
    # ---- shapes the tile kernel's rules hand back to the direct kernel
    _conv("fall-lds-over-64k", (2, 16, 16, 128, 128, 3, 2, 1), DIRECT % (4, 4), 2, resid=True, seed=24),
    _conv("fall-wo8-ho16", (2, 16, 8, 16, 32, 3, 1, 1), DIRECT % (2, 1), 3, acc="zero", publish=True, seed=25),
)
FALL_BACK = ("fall-lds-over-64k", "fall-wo8-ho16")
LARGE = ("t24-64p", "t24-1x1-64p", "t44-32p")


def conv_by_id(cid):
    return next(c for c in CONV_CASES if c["id"] == cid)


def conv_dims(c):
    B, H, W, Cin, Cout, k, s, P = c["shape"]
    Ho, Wo = out_hw(H, W, k, s)
    K = k * k * Cin
    return dict(B=B, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, P=P, Ho=Ho, Wo=Wo, K=K, Kp=(K + 31) // 32 * 32, npix=B * Ho * Wo,
                rows_in=B * H * W * c["ranks"])


@functools.lru_cache(maxsize=4)
def conv_inputs(cid):
    """Everything a convolution case reads, as numpy arrays (float32 unless noted): x [P, B, H, W, Cin], Wb (torch bf16 [Cout, Kp]), resid,
    gamma, beta, stats (mode 0: mean, invstd; 1: running mean, running var), in_acc [P, COPIES, 2 Cin] float64, acc0 (acc_out before the launch),
    running (mean, var before the launch); flip: Wfwd, the forward layer's fp32 filter [Cin, Cout, 3, 3]."""
    c = conv_by_id(cid)
    d = conv_dims(c)
    rng = _rng(c["seed"], 0xC0)
    P, B, H, W, Cin, Cout, k = d["P"], d["B"], d["H"], d["W"], d["Cin"], d["Cout"], d["k"]
    I = dict(x=planted_x(rng, (P, B, H, W, Cin), whole=c["mode"] == 2))
    if c["flip"]:
        I["Wfwd"] = (rng.standard_normal((Cin, Cout, 3, 3)) / math.sqrt(9 * Cin)).astype(np.float32)      # forward layer: Cout -> Cin channels
        I["Wb"] = flip_ref(I["Wfwd"], d["Kp"])
    else:
        Wf = (rng.standard_normal((Cout, Cin, k, k)) / math.sqrt(d["K"])).astype(np.float32)
        I["Wb"] = prep_ref(Wf, d["Kp"])[0]
    if c["resid"]:
        I["resid"] = rng.standard_normal((P, d["npix"], Cout), dtype=np.float32)
        I["resid"][..., 0] += np.float32(30.0)
    I["gamma"], I["beta"] = planted_affine(rng, Cin)
    x64 = I["x"].astype(np.float64).reshape(P, -1, Cin)
    s1, s2 = x64.sum(1), (x64 * x64).sum(1)
    if c["mode"] in (0, 1):
        m = s1[0] / x64.shape[1]
        v = np.maximum(s2[0] / x64.shape[1] - m * m, 0.0)
        if c["mode"] == 0:
            I["stats"] = (m.astype(np.float32), (1.0 / np.sqrt(v + float(EPS))).astype(np.float32))
        else:
            I["stats"] = ((m + 0.05 * rng.standard_normal(Cin)).astype(np.float32), (1.1 * v + 0.01).astype(np.float32))
    if c["mode"] == 3:
        I["in_acc"] = split_copies(rng, np.concatenate([s1, s2], axis=1) * float(c["ranks"]))         # the sums of `ranks` times the rows
        I["running"] = ((0.1 * rng.standard_normal(Cin)).astype(np.float32), rng.uniform(0.5, 1.5, Cin).astype(np.float32))
    if c["acc"]:
        acc0 = np.zeros((P, COPIES, 2 * Cout))
        if c["acc"] == "add":
            acc0[:, 1::3] = rng.integers(-8, 9, (P, len(range(1, COPIES, 3)), 2 * Cout)) * 0.5           # exactly representable, non-zero
        I["acc0"] = acc0
    return I


def conv_stats64(c, I):
    """per-pass float64 (mu, invstd) of the input BatchNorm as the launch defines them, [P, Cin] each (mode 2: None)"""
    d = conv_dims(c)
    if c["mode"] == 2:
        return None
    if c["mode"] == 0:
        return I["stats"][0].astype(np.float64)[None], I["stats"][1].astype(np.float64)[None]
    if c["mode"] == 1:
        return I["stats"][0].astype(np.float64)[None], 1.0 / np.sqrt(I["stats"][1].astype(np.float64) + float(EPS))[None]
    t = fold_copies(I["in_acc"])
    m = t[:, :d["Cin"]] / d["rows_in"]
    v = np.maximum(t[:, d["Cin"]:] / d["rows_in"] - m * m, 0.0)
    return m, 1.0 / np.sqrt(v + float(EPS))


def conv_stats32(c, I):
    """the same in the kernels' float32: (mu, invstd) [P, Cin]"""
    d = conv_dims(c)
    if c["mode"] == 0:
        return I["stats"][0][None], I["stats"][1][None]
    if c["mode"] == 1:
        return I["stats"][0][None], (np.float32(1.0) / np.sqrt(I["stats"][1] + EPS))[None].astype(np.float32)
    t = fold_copies(I["in_acc"])
    m = t[:, :d["Cin"]] / d["rows_in"]
    v = np.maximum(t[:, d["Cin"]:] / d["rows_in"] - m * m, 0.0)
    return m.astype(np.float32), (np.float32(1.0) / np.sqrt(v.astype(np.float32) + EPS)).astype(np.float32)


def conv_filter64(c, I):
    """the tap-major float64 filter [Cout, K] of the launch as a forward convolution"""
    d = conv_dims(c)
    return I["Wb"].double().numpy()[:, :d["K"]]


@functools.lru_cache(maxsize=2)
def conv_expect(cid):
    """want / tol [P, npix, Cout] float64, clean (outputs without an operand term), frac_w (share of activation elements with w > 0), frac_clean (share of outputs without an operand
    term), and the expected published / running statistics of a publishing case."""
    c = conv_by_id(cid)
    d, I = conv_dims(c), conv_inputs(cid)
    P, Cout = d["P"], d["Cout"]
    st = conv_stats64(c, I)
    Wt = conv_filter64(c, I)
    Wa = np.abs(Wt)
    want, tol, clean = np.empty((P, d["npix"], Cout)), np.empty((P, d["npix"], Cout)), np.empty((P, d["npix"], Cout), dtype=bool)
    n_w = n_op = 0
    if c["flip"]:                                      # the float64 adjoint of the FORWARD convolution Cout -> Cin channels, not the flipped filter
        Wfwd = tap_major(bf16_rne(I["Wfwd"]))          # [Cin (forward Cout), 9 * Cout]
    for p in range(P):
        A = act_ref(I["x"][p], None, None, None, None, raw=True) if st is None else \
            act_ref(I["x"][p], st[0][min(p, len(st[0]) - 1)], st[1][min(p, len(st[1]) - 1)], I["gamma"].astype(np.float64), I["beta"].astype(np.float64))
        if c["flip"]:
            dy = A["abf"].reshape(-1, d["Cin"])
            wp = col2im_ref(dy @ Wfwd, d["B"], d["H"], d["W"], Cout, 3, 1).reshape(-1, Cout)
            S = col2im_ref(np.abs(dy) @ np.abs(Wfwd), d["B"], d["H"], d["W"], Cout, 3, 1).reshape(-1, Cout)
            O = np.zeros_like(S)
        else:
            wp = conv_ref(A["abf"], Wt, d["k"], d["s"])
            S = conv_ref(np.abs(A["abf"]), Wa, d["k"], d["s"])
            O = conv_ref(A["w"], Wa, d["k"], d["s"]) if st is not None else np.zeros_like(S)
        n_w += int((A["w"] > 0).sum())
        n_op += int((O > 0).sum())
        clean[p] = O == 0
        rs = I["resid"][p].astype(np.float64) if c["resid"] else 0.0
        want[p] = wp + rs
        tol[p] = C_ACC * U24 * S + O + U23 * np.abs(want[p]) + U24 * np.abs(rs)
    ex = dict(want=want, tol=tol, clean=clean, frac_w=n_w / I["x"].size, frac_clean=1.0 - n_op / want.size)
    if c["publish"]:
        t = fold_copies(I["in_acc"])
        Cin = d["Cin"]
        mu, isd, rm, rv = [], [], None, None
        for p in range(P):
            a, b, rm_p, rv_p = finalize_ref(t[p, :Cin], t[p, Cin:], d["rows_in"], EPS, I["running"] if (c["running"] and p == 0) else None)
            mu.append(a)
            isd.append(b)
            if p == 0 and c["running"]:
                rm, rv = rm_p, rv_p
        ex.update(pub_mean=np.stack(mu), pub_isd=np.stack(isd), mean64=t[:, :Cin] / d["rows_in"],
                  running=(rm, rv) if c["running"] else I["running"])        # (update_running off: the running statistics stay)
    return ex


class ConvLaunch:
    """Everything one convolution case reads and writes, on ``device`` ('cpu' for the float32 restatement)."""

    def __init__(self, c, device, Wb=None):
        self.c, self.d, self.I, self.device = c, conv_dims(c), conv_inputs(c["id"]), device
        d, I, A = self.d, self.I, Arena(device)
        self.A = A
        f = torch.from_numpy
        A.read("x", f(I["x"]))
        A.read("Wb", I["Wb"] if Wb is None else Wb)
        self.resid = A.read("resid", f(I["resid"])) if c["resid"] else None
        self.gamma = A.read("gamma", f(I["gamma"])) if c["mode"] != 2 else None
        self.beta = A.read("beta", f(I["beta"])) if c["mode"] != 2 else None
        self.stats = (A.read("s0", f(I["stats"][0])), A.read("s1", f(I["stats"][1]))) if c["mode"] in (0, 1) else None
        self.in_acc = A.read("in_acc", f(I["in_acc"])) if c["mode"] == 3 else None
        self.y = A.write("y", nan_like((d["P"] * d["npix"], d["Cout"])))
        self.acc_out = A.write("acc_out", f(I["acc0"])) if c["acc"] else None
        self.publish = (A.write("pub_mean", nan_like((d["P"], d["Cin"]))), A.write("pub_isd", nan_like((d["P"], d["Cin"])))) if c["publish"] else None
        self.running = (A.write("run_mean", f(I["running"][0])), A.write("run_var", f(I["running"][1]))) if c["publish"] else None

    def run_hip(self):
        c, d = self.c, self.d
        ops.wrn_conv_bn(self.A["x"], c["mode"], self.stats, self.in_acc, self.gamma, self.beta, float(EPS), float(SLOPE), self.A["Wb"], self.resid,
                        self.y, d["B"], d["H"], d["W"], d["Cin"], d["Cout"], d["k"], d["s"], d["Kp"], publish=self.publish, running=self.running,
                        momentum=float(MOMENTUM), update_running=c["running"], acc_out=self.acc_out, stat_ranks=c["ranks"], passes=d["P"])


def stats_of_stored(y, P):
    """float64 sums of the y a launch stored: (sum, sum of squares, sum |y|) [P, Cout]"""
    y = y.reshape(P, -1, y.shape[-1]).astype(np.float64)
    return y.sum(1), (y * y).sum(1), np.abs(y).sum(1)


def conv_verify(L, ex=None):
    """Holds the outputs of L to conv_expect: y per element, the statistics of what was stored, the published and running statistics, all
    surroundings.  Returns dict(y=, y_clean=, sum=, sq=, var=, var_far=, mean=, ulp1=): the largest |got - want| / tol of each, and the count of 1-ulp differences."""
    c, d = L.c, L.d
    ex = conv_expect(c["id"]) if ex is None else ex
    name = c["id"]
    P, Cout = d["P"], d["Cout"]
    y = L.y.cpu().numpy().reshape(P, d["npix"], Cout)
    H = dict(y=worst(name + " y", y, ex["want"], ex["tol"]), ulp1=0)
    # (an element whose operand term is not zero reads close to 1 whenever the kernel rounded an activation near a tie the other way: the
    # headroom of the accumulation itself is the one over the elements without an operand term)
    H["y_clean"] = float((np.abs(y - ex["want"])[ex["clean"]] / ex["tol"][ex["clean"]]).max())
    if c["acc"]:
        got = fold_copies(L.acc_out.cpu().numpy()) - fold_copies(L.I["acc0"])
        s1, s2, sa = stats_of_stored(y, P)
        H["sum"] = worst(name + " acc_out sums", got[:, :Cout], s1, C_SUM * U24 * sa)
        H["sq"] = worst(name + " acc_out squares", got[:, Cout:], s2, C_SUM * U24 * s2)
        # the mean and variance the next BatchNorm derives, against float64, bounds stated in E[y^2]: |dm| <= C_SUM 2^-24 E|y| and
        # |dv| <= C_SUM 2^-24 (E[y^2] + 2 |m| E|y|); channel 0 of a case with a residual is far from zero (mean / std about 30)
        n = float(d["npix"])
        m_g, m_w = got[:, :Cout] / n, s1 / n
        v_g, v_w = got[:, Cout:] / n - m_g * m_g, s2 / n - m_w * m_w
        vt = C_SUM * U24 * (s2 / n + 2.0 * np.abs(m_w) * sa / n)
        H["var"] = worst(name + " derived variance", v_g, v_w, vt)
        if c["resid"]:
            H["var_far"] = float((np.abs(v_g - v_w)[:, 0] / vt[:, 0]).max())
    if c["publish"]:
        H.update(stat_verify(name, L.publish[0].cpu().numpy(), L.publish[1].cpu().numpy(), L.running[0].cpu().numpy(), L.running[1].cpu().numpy(), ex,
                             moved=c["running"]))
    bad = L.A.surroundings_touched()
    assert not bad, "%s: surroundings overwritten: %s" % (name, bad)
    return H


def stat_verify(name, mean, isd, rm, rv, ex, moved=True):
    """published mean within one rounding of float64; invstd / running statistics equal to finalize_ref up to one ulp (counted); running
    statistics that the launch must not move (moved = False) keep their bits"""
    m64 = ex["mean64"].reshape(mean.shape)
    H = dict(mean=worst(name + " published mean", mean, m64, U24 * np.abs(m64) + 1e-45))
    n1 = 0
    for what, got, want in (("invstd", isd, ex["pub_isd"].reshape(isd.shape)), ("running_mean", rm, ex["running"][0]),
                            ("running_var", rv, ex["running"][1])):
        u = ulps32(np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32))
        assert np.isfinite(got).all() and u.max() <= (0 if (not moved and what != "invstd") else 1), "%s %s: %d ulp from the statement of bn_finalize at %s (got %r want %r)" % (
            name, what, u.max(), np.unravel_index(int(u.argmax()), u.shape), got.reshape(-1)[int(u.argmax())], want.reshape(-1)[int(u.argmax())])
        n1 += int((u == 1).sum())
    H["ulp1"] = n1
    return H


# ---- float32 restatement of the convolution ----------------------------------------------------------------------------------------------------
def accumulate32(col, Wb32, KS=1, reverse=False):
    """col [n, Kp] @ Wb32 [Cout, Kp]^T in float32 over 32-wide k steps: KS parts take every KS-th step each (first to last, or last to first) and
    are added to part 0 in order (the LDS sum of the split-K waves)."""
    nks = col.shape[1] // 32
    parts = []
    for part in range(KS):
        acc = np.zeros((col.shape[0], Wb32.shape[0]), dtype=np.float32)
        steps = list(range(part, nks, KS))
        for ks in (reversed(steps) if reverse else steps):
            acc += col[:, ks * 32:ks * 32 + 32] @ Wb32[:, ks * 32:ks * 32 + 32].T
        parts.append(acc)
    out = parts[0]
    for p in parts[1:]:
        out = (out + p).astype(np.float32)
    return out


def conv_KS(c):
    k = c["kernel"]
    return int(k[-2]) if k.startswith("wrn_conv_kernel") else 1


def walk_sums32(c, y, grid_x):
    """Per-channel sum and sum of squares of y [npix, Cout] float32 as the kernels take them: fp32 per lane over the 16-pixel tiles a lane walks
    (direct: the rounds of the grid-stride loop; tile: the PG groups of a wave, taken here in raster order), a 16-lane fp32 reduction, fp64 from
    there.  -> (s1, s2) float64 [Cout]"""
    n, Cout = y.shape
    nt = (n + 15) // 16
    yp = np.zeros((nt * 16, Cout), dtype=np.float32)
    yp[:n] = y
    if c["kernel"].startswith("wrn_conv_kernel"):
        per_round = grid_x * (4 // conv_KS(c))
        rounds = (nt + per_round - 1) // per_round
        t = np.zeros((rounds * per_round * 16, Cout), dtype=np.float32)
        t[:nt * 16] = yp
        t = t.reshape(rounds, per_round, 16, Cout)
    else:
        PG = int(c["kernel"][-2])
        t = yp.reshape(nt // PG, PG, 16, Cout).transpose(1, 0, 2, 3)
    s1 = np.zeros(t.shape[1:], dtype=np.float32)
    s2 = np.zeros(t.shape[1:], dtype=np.float32)
    for i in range(t.shape[0]):
        s1 = (s1 + t[i]).astype(np.float32)
        s2 = (s2 + (t[i] * t[i]).astype(np.float32)).astype(np.float32)
    for h in (8, 4, 2, 1):                                        # the 16 pixel lanes of a channel
        s1 = (s1[:, :h] + s1[:, h:2 * h]).astype(np.float32)
        s2 = (s2[:, :h] + s2[:, h:2 * h]).astype(np.float32)
    return s1.astype(np.float64).sum((0, 1)), s2.astype(np.float64).sum((0, 1))


def conv_act32(c, I, p, fma=False):
    """the bf16 activation of pass p as float32 [B, H, W, Cin], by the kernels' float32 arithmetic"""
    if c["mode"] == 2:
        return to_bf16(I["x"][p]).float().numpy()
    mu, isd = conv_stats32(c, I)
    a, _ = act32(I["x"][p], mu[min(p, len(mu) - 1)], isd[min(p, len(isd) - 1)], I["gamma"], I["beta"], fma=fma)
    return to_bf16(a).float().numpy()


def conv_restate(L, fault=None, reverse=False):
    """The launch in float32 on the CPU, written into L's arenas as a kernel would.  fault: one of the planted faults of
    tests/test_cpu_wrn_cases.py (None: the faithful restatement)."""
    c, d, I = L.c, L.d, L.I
    assert L.device == "cpu"
    P, Cout, k, s, Cin = d["P"], d["Cout"], d["k"], d["s"], d["Cin"]
    Wb32 = (I["Wb"] if fault != "flip_no_rotation" else flip_ref(I["Wfwd"].reshape(Cin, Cout, 9)[:, :, ::-1].reshape(Cin, Cout, 3, 3).copy(), d["Kp"])).float().numpy()
    grid_x = ops.wrn_conv_plan(*c["shape"]).grid_x
    y = L.y.view(P, d["npix"], Cout)
    acc_before = L.acc_out.clone() if L.acc_out is not None else None
    I_use = I
    if fault == "pass1_reads_pass0_acc":
        I_use = dict(I, in_acc=np.concatenate([I["in_acc"][:1], I["in_acc"][:1], I["in_acc"][2:]]))
    for p in range(P):
        a = conv_act32(c, I_use, p)
        col = np.zeros((d["npix"], d["Kp"]), dtype=np.float32)
        col[:, :d["K"]] = im2col_ref(a, k, s)
        if fault == "left_border_wraps" and p == 0 and k == 3:    # tap (., 0) of the pixels of column 0 reads the previous row's last pixel
            ap = a.reshape(-1, Cin)
            cv = col.reshape(d["B"], d["Ho"], d["Wo"], d["Kp"])
            for i in range(3):
                for yo in range(d["Ho"]):
                    yy = yo * s + i - 1
                    flat = (0 * d["H"] + yy) * d["W"] + (-1)
                    if 0 <= yy < d["H"] and flat >= 0:
                        cv[0, yo, 0, (i * 3) * Cin:(i * 3 + 1) * Cin] = ap[flat]
        if fault == "last_tap_missing_on_one_tile" and p == 0:
            t0 = 16 * ((d["npix"] // 16) // 2)
            col[t0:t0 + 16, (k * k - 1) * Cin:k * k * Cin] = 0.0
        out = accumulate32(col, Wb32, conv_KS(c), reverse)
        if c["resid"]:
            r = I["resid"][p].copy()
            if fault == "resid_skipped_on_ragged_tile" and p == P - 1:
                r[(d["npix"] // 16) * 16:] = 0.0
            out = (out + r).astype(np.float32)
        if fault == "lane_stores_to_neighbour_pixel" and p == 0:
            px = min(5, d["npix"] - 2)
            out[px + 1, 4:8] = out[px, 4:8]
        y[p].copy_(torch.from_numpy(out))
        if c["acc"]:
            s1, s2 = walk_sums32(c, out, grid_x)
            add = torch.from_numpy(np.concatenate([s1, s2]))
            if fault == "acc_out_overwritten":
                L.acc_out[p].zero_()
            L.acc_out[p, p % COPIES] += add
    if c["publish"]:
        t = fold_copies(I_use["in_acc"])
        run = [v.copy() for v in I["running"]]
        for p in range(P):
            moves = c["running"] and (p == 0 or (fault == "running_moved_by_pass1" and p == 1))
            mu, isd, rm, rv = finalize_ref(t[p, :Cin], t[p, Cin:], d["rows_in"], EPS, run if moves else None)
            L.publish[0][p].copy_(torch.from_numpy(mu))
            L.publish[1][p].copy_(torch.from_numpy(isd))
            if moves:
                run = [rm, rv]
        L.running[0].copy_(torch.from_numpy(run[0]))
        L.running[1].copy_(torch.from_numpy(run[1]))


# ---- what the constants are made of -------------------------------------------------------------------------------------------------------------
def conv_acc_ratio(c):
    """largest |float32 accumulation - float64| / (2^-24 conv(|a|, |W|)) over the passes of one case (at most 4 of them), either order"""
    d, I = conv_dims(c), conv_inputs(c["id"])
    Wb32 = I["Wb"].float().numpy()
    W64, worst_ = Wb32.astype(np.float64), 0.0
    for p in range(min(d["P"], 4)):
        col = np.zeros((d["npix"], d["Kp"]), dtype=np.float32)
        col[:, :d["K"]] = im2col_ref(conv_act32(c, I, p), d["k"], d["s"])
        c64 = col.astype(np.float64)
        want, S = c64 @ W64.T, np.abs(c64) @ np.abs(W64).T
        for rev in (False, True):
            got = accumulate32(col, Wb32, conv_KS(c), rev).astype(np.float64)
            nz = S > 0
            worst_ = max(worst_, float((np.abs(got - want)[nz] / (U24 * S[nz])).max()))
    return worst_


def measure_c_acc():
    return max(conv_acc_ratio(c) for c in CONV_CASES)


def conv_r_ratio(c):
    """largest (|float32 pre-activation - float64| - |gamma| invstd |fp32(mu) - mu|) / (2^-24 (|gamma| |x - mu| invstd + |beta|)), with and
    without the contraction"""
    if c["mode"] == 2:
        return 0.0
    d, I = conv_dims(c), conv_inputs(c["id"])
    m64, i64 = conv_stats64(c, I)
    m32, i32 = conv_stats32(c, I)
    g, b = I["gamma"].astype(np.float64), I["beta"].astype(np.float64)
    worst_ = 0.0
    for p in range(min(d["P"], 4)):
        q = min(p, len(m64) - 1)
        x = I["x"][p].astype(np.float64)
        yv = g * ((x - m64[q]) * i64[q]) + b
        mag = np.abs(g) * np.abs(x - m64[q]) * i64[q] + np.abs(b)
        known = np.abs(g) * i64[q] * np.abs(m32[q].astype(np.float64) - m64[q])
        for fma in (False, True):
            got = act32(I["x"][p], m32[q], i32[q], I["gamma"], I["beta"], fma=fma)[1].astype(np.float64)
            nz = mag > 0
            worst_ = max(worst_, float((np.maximum(np.abs(got - yv) - known, 0.0)[nz] / (U24 * mag[nz])).max()))
    return worst_


def measure_c_r():
    return max(conv_r_ratio(c) for c in CONV_CASES)


def conv_sum_ratio(c):
    """largest |walk_sums32 - float64 sums| / (2^-24 sum |y|) (and sum y^2) over the first passes of a case with statistics"""
    if not c["acc"]:
        return 0.0
    d = conv_dims(c)
    ex = conv_expect(c["id"])
    grid_x = ops.wrn_conv_plan(*c["shape"]).grid_x
    worst_ = 0.0
    for p in range(min(d["P"], 4)):
        y = ex["want"][p].astype(np.float32)
        s1, s2 = walk_sums32(c, y, grid_x)
        w1, w2, wa = stats_of_stored(y, 1)
        worst_ = max(worst_, float((np.abs(s1 - w1[0]) / (U24 * wa[0])).max()), float((np.abs(s2 - w2[0]) / (U24 * w2[0])).max()))
    return worst_


def measure_c_sum():
    return max(conv_sum_ratio(c) for c in CONV_CASES)


# ---- the network's tail: srhip_wrn_head_passes -----------------------------------------------------------------------------------------------
def _head(cid, B, HW2, C, K, mode, P=1, ranks=1, publish=False, running=False, seed=0):
    return dict(id=cid, B=B, HW2=HW2, C=C, K=K, mode=mode, P=P, ranks=ranks, publish=publish, running=running, seed=seed)


HEAD_CASES = (
    _head("h-c32-hw1-k1-m0", 3, 1, 32, 1, 0, seed=1),
    _head("h-c96-hw7-k10-m1", 2, 7, 96, 10, 1, seed=2),
    _head("h-c160-hw64-k33-m3", 2, 64, 160, 33, 3, publish=True, running=True, seed=3),
    _head("h-c256-hw65-k100-3p", 2, 65, 256, 100, 3, P=3, publish=True, running=True, seed=4),
    _head("h-c32-hw65-k33-2ranks", 2, 65, 32, 33, 3, ranks=2, publish=True, seed=5),
    _head("h-c256-hw64-k10-m0", 1, 64, 256, 10, 0, seed=6),
)


class HeadLaunch:
    def __init__(self, c, device):
        self.c, self.device = c, device
        rng = _rng(c["seed"], 0x4EAD)
        P, B, HW2, C, K = c["P"], c["B"], c["HW2"], c["C"], c["K"]
        I = dict(x=planted_x(rng, (P, B, 1, HW2, C)).reshape(P, B, HW2, C))
        I["gamma"], I["beta"] = planted_affine(rng, C)
        I["Wc"] = (rng.standard_normal((K, C)) / math.sqrt(C)).astype(np.float32)
        I["bc"] = (0.1 * rng.standard_normal(K)).astype(np.float32)
        x64 = I["x"].astype(np.float64).reshape(P, -1, C)
        s1, s2 = x64.sum(1), (x64 * x64).sum(1)
        self.rows = B * HW2 * c["ranks"]
        m = s1[0] / x64.shape[1]
        v = np.maximum(s2[0] / x64.shape[1] - m * m, 0.0)
        if c["mode"] == 0:
            I["stats"] = (m.astype(np.float32), (1.0 / np.sqrt(v + float(EPS))).astype(np.float32))
        elif c["mode"] == 1:
            I["stats"] = ((m + 0.05 * rng.standard_normal(C)).astype(np.float32), (1.1 * v + 0.01).astype(np.float32))
        else:
            I["in_acc"] = split_copies(rng, np.concatenate([s1, s2], axis=1) * float(c["ranks"]))
            I["running"] = ((0.1 * rng.standard_normal(C)).astype(np.float32), rng.uniform(0.5, 1.5, C).astype(np.float32))
        self.I = I
        A = self.A = Arena(device)
        f = torch.from_numpy
        for n in ("x", "gamma", "beta", "Wc", "bc"):
            A.read(n, f(I[n]))
        self.stats = (A.read("s0", f(I["stats"][0])), A.read("s1", f(I["stats"][1]))) if c["mode"] != 3 else None
        self.in_acc = A.read("in_acc", f(I["in_acc"])) if c["mode"] == 3 else None
        self.feat = A.write("feat", nan_like((P * B, C)))
        self.logits = A.write("logits", nan_like((P * B, K)))
        self.publish = (A.write("pub_mean", nan_like((P, C))), A.write("pub_isd", nan_like((P, C)))) if c["publish"] else None
        self.running = (A.write("run_mean", f(I["running"][0])), A.write("run_var", f(I["running"][1]))) if c["publish"] else None

    def run_hip(self):
        c, A = self.c, self.A
        ops.wrn_head(A["x"], c["mode"], self.stats, self.in_acc, A["gamma"], A["beta"], float(EPS), float(SLOPE), A["Wc"], A["bc"], self.feat,
                     self.logits, c["B"], c["HW2"], c["C"], c["K"], publish=self.publish, running=self.running, momentum=float(MOMENTUM),
                     update_running=c["running"], stat_ranks=c["ranks"], passes=c["P"])

    def _stats(self, f32):
        c, I, C = self.c, self.I, self.c["C"]
        if c["mode"] == 0:
            mu, isd = I["stats"][0][None], I["stats"][1][None]
            return (mu, isd) if f32 else (mu.astype(np.float64), isd.astype(np.float64))
        if c["mode"] == 1:
            if f32:
                return I["stats"][0][None], (np.float32(1.0) / np.sqrt(I["stats"][1] + EPS)).astype(np.float32)[None]
            return I["stats"][0].astype(np.float64)[None], (1.0 / np.sqrt(I["stats"][1].astype(np.float64) + float(EPS)))[None]
        t = fold_copies(I["in_acc"])
        m = t[:, :C] / self.rows
        v = np.maximum(t[:, C:] / self.rows - m * m, 0.0)
        if f32:
            return m.astype(np.float32), (np.float32(1.0) / np.sqrt(v.astype(np.float32) + EPS)).astype(np.float32)
        return m, 1.0 / np.sqrt(v + float(EPS))

    def expect(self):
        """feat: the float64 mean of the float64 activation; its bound = the mean of r (the LeakyReLU is 1-Lipschitz) + (HW2 + 10) fp32 roundings of
        the mean of |a| (a product with the slope, at most HW2 additions per thread, at most 8 partial sums, one division).  logits: float64 of the
        float64 feat; bound = sum_c tol_feat |Wc| + (ceil(C / 64) + 8) 2^-24 (sum |feat Wc| + |bc|): a lane's <= 4 products and additions, the
        6 steps of the wave sum, the bias."""
        c, I = self.c, self.I
        P, B, HW2, C, K = c["P"], c["B"], c["HW2"], c["C"], c["K"]
        mu, isd = self._stats(False)
        g, b = I["gamma"].astype(np.float64), I["beta"].astype(np.float64)
        W, bc = I["Wc"].astype(np.float64), I["bc"].astype(np.float64)
        feat, ftol = np.empty((P, B, C)), np.empty((P, B, C))
        for p in range(P):
            q = min(p, len(mu) - 1)
            A = act_ref(I["x"][p], mu[q], isd[q], g, b)
            feat[p] = A["a"].mean(1)
            ftol[p] = A["r"].mean(1) + (HW2 + 10) * U24 * np.abs(A["a"]).mean(1)
        feat, ftol = feat.reshape(P * B, C), ftol.reshape(P * B, C)
        ex = dict(feat=feat, ftol=ftol, logits=feat @ W.T + bc,
                  ltol=ftol @ np.abs(W).T + ((C + 63) // 64 + 8) * U24 * (np.abs(feat) @ np.abs(W).T + np.abs(bc)))
        if c["publish"]:
            t = fold_copies(I["in_acc"])
            mus, isds, run = [], [], I["running"]
            for p in range(P):
                a, b_, rm, rv = finalize_ref(t[p, :C], t[p, C:], self.rows, EPS, I["running"] if (c["running"] and p == 0) else None)
                mus.append(a)
                isds.append(b_)
                if p == 0 and c["running"]:
                    run = (rm, rv)
            ex.update(pub_mean=np.stack(mus), pub_isd=np.stack(isds), mean64=t[:, :C] / self.rows, running=run)
        return ex

    def restate(self):
        c, I = self.c, self.I
        mu, isd = self._stats(True)
        for p in range(c["P"]):
            q = min(p, len(mu) - 1)
            a, _ = act32(I["x"][p], mu[q], isd[q], I["gamma"], I["beta"])
            s = np.zeros((c["B"], c["C"]), dtype=np.float32)
            for i in range(c["HW2"]):
                s = (s + a[:, i]).astype(np.float32)
            ft = (s / np.float32(c["HW2"])).astype(np.float32)
            lg = ((ft @ I["Wc"].T).astype(np.float32) + I["bc"]).astype(np.float32)
            self.feat[p * c["B"]:(p + 1) * c["B"]].copy_(torch.from_numpy(ft))
            self.logits[p * c["B"]:(p + 1) * c["B"]].copy_(torch.from_numpy(lg))
        if c["publish"]:
            ex = self.expect()
            self.publish[0].copy_(torch.from_numpy(ex["pub_mean"]))
            self.publish[1].copy_(torch.from_numpy(ex["pub_isd"]))
            self.running[0].copy_(torch.from_numpy(ex["running"][0]))
            self.running[1].copy_(torch.from_numpy(ex["running"][1]))

    def verify(self):
        ex, name = self.expect(), self.c["id"]
        H = dict(feat=worst(name + " feat", self.feat.cpu().numpy(), ex["feat"], ex["ftol"]),
                 logits=worst(name + " logits", self.logits.cpu().numpy(), ex["logits"], ex["ltol"]), ulp1=0)
        if self.c["publish"]:
            H.update(stat_verify(name, *(t.cpu().numpy() for t in self.publish + self.running), ex, moved=self.c["running"]))
        bad = self.A.surroundings_touched()
        assert not bad, "%s: surroundings overwritten: %s" % (name, bad)
        return H


# ---- BatchNorm forward: bn_accumulate, bn_fold, bn_stats, bn_fwd, bn_act ----------------------------------------------------------------------
def bn_pass_rows(C):
    """rows one pass of a bn_reduce_kernel workgroup covers: 256 threads, C / V of them along a row (V = 4 channels per thread when C % 4 == 0)"""
    return 256 // (C // (4 if C % 4 == 0 else 1))


BN_CASES = tuple(dict(id="bn-c%d-r%d" % (C, rows), C=C, rows=rows, seed=17 * C + i)
                 for C in (2, 4, 16, 256)
                 for i, rows in enumerate((1, bn_pass_rows(C) - 1, bn_pass_rows(C), bn_pass_rows(C) + 1, 70001)))
# A workgroup of bn_reduce_kernel takes rows_per_block = (rows / 512 rounded up to whole passes, at most 1024) rows, four passes per trip of
# its row loop: C = 256 at 70 001 rows (136 rows per workgroup, 16 per trip) is the case with more than one trip -- nine, the last ragged.
# At that size (BN_BIG elements and more) the float64 activation is checked in chunks of rows and only on the training bn_fwd: the four
# other activation launches are elementwise in bn_apply_kernel / bn_act_kernel, whose code no row count changes.
BN_BIG, BN_CHUNK = 4_000_000, 8192
WS_DOUBLES = WS_ACC + COPIES * 512


def bn_x(rng, rows, C):
    x = rng.standard_normal((rows, C), dtype=np.float32)
    x[:, 0] += np.float32(30.0)
    x[:, 1] = np.float32(0.75)
    return x


def check_act(name, act_bf16, act_f32, A):
    """the admissible-set rule on a bf16 activation (equality wherever w = 0) and the fp32 one within r + one rounding; -> share of w > 0"""
    if act_bf16 is not None:
        got = act_bf16.double().cpu().numpy().reshape(A["a"].shape)
        ok = (got >= A["lo"]) & (got <= A["hi"])
        if not ok.all():
            i = np.unravel_index(int(np.argmin(ok)), ok.shape)
            raise AssertionError("%s: bf16 activation at %s: got %.9g, admissible [%.9g, %.9g] (float64 %.9g, %d outside)" % (
                name, i, got[i], A["lo"][i], A["hi"][i], A["a"][i], int((~ok).sum())))
    if act_f32 is not None:
        worst(name + " fp32 activation", act_f32.cpu().numpy().reshape(A["a"].shape), A["a"], A["r"] + U24 * np.abs(A["a"]))
    return float((A["w"] > 0).mean())


class BnLaunch:
    """One (rows, C) of the BatchNorm forward kernels.  Every launch has outputs of its own."""

    def __init__(self, c, device):
        self.c, self.device = c, device
        rows, C = c["rows"], c["C"]
        rng = _rng(c["seed"], 0xB4)
        I = dict(x=bn_x(rng, rows, C))
        I["gamma"], I["beta"] = planted_affine(rng, C)
        I["run"] = ((0.1 * rng.standard_normal(C)).astype(np.float32), rng.uniform(0.5, 1.5, C).astype(np.float32))
        acc0 = np.zeros((COPIES, 2 * C))
        acc0[2::5] = rng.integers(-8, 9, (len(range(2, COPIES, 5)), 2 * C)) * 0.5
        I["acc0"] = acc0
        self.I = I
        A = self.A = Arena(device)
        f = torch.from_numpy
        for n in ("x", "gamma", "beta"):
            A.read(n, f(I[n]))
        A.write("acc", f(acc0))
        self.big = rows * C >= BN_BIG
        for n in ("fold", "stats", "stats2", "fwd", "fwd2"):
            A.write(n + "_mean", nan_like((C,)))
            A.write(n + "_isd", nan_like((C,)))
        for n in ("fold", "stats", "fwd"):
            A.write(n + "_rm", f(I["run"][0]))
            A.write(n + "_rv", f(I["run"][1]))
        A.write("totals", nan_like((2 * C,), torch.float64))
        A.write("ws", torch.zeros(WS_DOUBLES, dtype=torch.float64))
        A.write("ws_fwd", torch.zeros(WS_DOUBLES, dtype=torch.float64))
        self.acts = ("fwd",) if self.big else ("fwd", "eval") + (("act0", "act1", "act2") if C % 4 == 0 else ())
        for n in self.acts:
            A.write(n + "_bf16", nan_like((rows, C), torch.bfloat16))
            A.write(n + "_f32", nan_like((rows, C)))
        if not self.big:
            A.write("fwd2_bf16", nan_like((rows, C), torch.bfloat16))

    def run_hip(self):
        A, rows, C, e, s, m = self.A, self.c["rows"], self.c["C"], float(EPS), float(SLOPE), float(MOMENTUM)
        ops.bn_accumulate(A["x"], A["acc"], rows, C)
        ops.bn_fold(A["acc"], rows, e, m, True, A["fold_rm"], A["fold_rv"], A["fold_mean"], A["fold_isd"], A["totals"], C)
        ops.bn_stats(A["x"], e, m, True, A["stats_rm"], A["stats_rv"], A["stats_mean"], A["stats_isd"], A["ws"], rows, C)
        self.ws_after_first = A["ws"].clone()
        ops.bn_stats(A["x"], e, m, False, None, None, A["stats2_mean"], A["stats2_isd"], A["ws"], rows, C)
        ops.bn_fwd(A["x"], A["gamma"], A["beta"], e, s, m, True, True, A["fwd_rm"], A["fwd_rv"], A["fwd_mean"], A["fwd_isd"], A["fwd_bf16"],
                   A["fwd_f32"], A["ws_fwd"], rows, C)
        # a second training launch on the workspace the first left (running statistics held): the same bits
        ops.bn_fwd(A["x"], A["gamma"], A["beta"], e, s, m, True, False, A["fwd_rm"], A["fwd_rv"], A["fwd2_mean"], A["fwd2_isd"],
                   None if self.big else A["fwd2_bf16"], None, A["ws_fwd"], rows, C)
        if self.big:
            return
        ops.bn_fwd(A["x"], A["gamma"], A["beta"], e, s, m, False, False, A["fwd_rm"], A["fwd_rv"], None, None, A["eval_bf16"], A["eval_f32"], None,
                   rows, C)
        if C % 4 == 0:
            ops.bn_act(A["x"], (A["fwd_mean"], A["fwd_isd"]), A["gamma"], A["beta"], e, s, 0, A["act0_bf16"], rows, C, act_f32=A["act0_f32"])
            ops.bn_act(A["x"], (A["fwd_rm"], A["fwd_rv"]), A["gamma"], A["beta"], e, s, 1, A["act1_bf16"], rows, C, act_f32=A["act1_f32"])
            ops.bn_act(A["x"], None, None, None, e, s, 2, A["act2_bf16"], rows, C, act_f32=A["act2_f32"])

    def restate(self):
        A, I, rows, C = self.A, self.I, self.c["rows"], self.c["C"]
        f = torch.from_numpy
        x64 = I["x"].astype(np.float64)
        tot = np.concatenate([x64.sum(0), (x64 * x64).sum(0)])
        A["acc"][3] += f(tot)
        t = fold_copies(A["acc"].numpy())
        A["totals"].copy_(f(t))
        for n, tt in (("fold", t), ("stats", tot), ("fwd", tot)):
            mu, isd, rm, rv = finalize_ref(tt[:C], tt[C:], rows, EPS, I["run"])
            for k, v in (("_mean", mu), ("_isd", isd), ("_rm", rm), ("_rv", rv)):
                A[n + k].copy_(f(v))
        A["stats2_mean"].copy_(A["stats_mean"])
        A["stats2_isd"].copy_(A["stats_isd"])
        A["ws"][:2 * C].copy_(f(tot))
        A["ws_fwd"][:2 * C].copy_(f(tot))
        self.ws_after_first = A["ws"].clone()
        g, b = I["gamma"], I["beta"]
        mu, isd, rm, rv = (A["fwd" + k].numpy() for k in ("_mean", "_isd", "_rm", "_rv"))
        isr = (np.float32(1.0) / np.sqrt(rv + EPS)).astype(np.float32)
        A["fwd2_mean"].copy_(A["fwd_mean"])
        A["fwd2_isd"].copy_(A["fwd_isd"])
        outs = [("fwd", act32(I["x"], mu, isd, g, b)[0])]
        if not self.big:
            A["fwd2_bf16"].copy_(to_bf16(outs[0][1]))
            outs.append(("eval", act32(I["x"], rm, isr, g, b)[0]))
            if C % 4 == 0:
                outs += [("act0", outs[0][1]), ("act1", outs[1][1]), ("act2", I["x"])]
        for n, a in outs:
            A[n + "_bf16"].copy_(to_bf16(a))
            A[n + "_f32"].copy_(f(np.ascontiguousarray(a)))

    def verify(self):
        A, I, rows, C, name = self.A, self.I, self.c["rows"], self.c["C"], self.c["id"]
        x64 = I["x"].astype(np.float64)
        s1, s2, sa = x64.sum(0), (x64 * x64).sum(0), np.abs(x64).sum(0)
        want = np.concatenate([s1, s2])
        # fp64 sums of fp32 values (products of two fp32 values are exact in fp64): recursive summation, at most rows + 32 additions
        stol = (rows + 32) * 2.0 ** -53 * np.concatenate([sa, s2]) + 2.0 ** -48 * np.abs(I["acc0"]).sum(0)
        H = dict(ulp1=0)
        acc = A["acc"].cpu().numpy()
        H["accumulate"] = worst(name + " bn_accumulate", fold_copies(acc) - fold_copies(I["acc0"]), want, stol)
        H["totals"] = worst(name + " bn_fold totals", A["totals"].cpu().numpy(), fold_copies(acc), 2.0 ** -50 * np.abs(acc).sum(0))
        for ws, first in ((A["ws"], self.ws_after_first), (A["ws_fwd"], None)):
            for w in ((ws, first) if first is not None else (ws,)):
                w = w.cpu().numpy()
                H["ws"] = max(H.get("ws", 0.0), worst(name + " ws totals", w[:2 * C], want, stol))
                assert not w[2 * C:].view(np.int64).any(), "%s: the arrival counter or an accumulator copy is not zero after the launch" % name
        # (the fp64 totals of two launches may differ in the last bits of a double -- the order of the atomic additions, csrc/wrn_bn.h -- 29 bits
        # below the float the statistics are rounded to: both launches' totals are held to the bound above, the fp32 statistics to the same bits)
        for n in ("_mean", "_isd"):
            assert torch.equal(bits(A["stats2" + n]), bits(A["stats" + n])), "%s: a second bn_stats launch gave other bits (%s)" % (name, n)
        for n in ("_mean", "_isd") + (() if self.big else ("_bf16",)):
            assert torch.equal(bits(A["fwd2" + n]), bits(A["fwd" + n])), "%s: a second bn_fwd launch gave other bits (%s)" % (name, n)
        for n, tt in (("fold", fold_copies(acc)), ("stats", A["ws"].cpu().numpy()[:2 * C]), ("fwd", A["ws_fwd"].cpu().numpy()[:2 * C])):
            mu, isd, rm, rv = finalize_ref(tt[:C], tt[C:], rows, EPS, I["run"])
            ex = dict(mean64=tt[:C] / rows, pub_isd=isd, running=(rm, rv))
            h = stat_verify(name + " " + n, *(A[n + k].cpu().numpy() for k in ("_mean", "_isd", "_rm", "_rv")), ex)
            H["ulp1"] += h["ulp1"]
            H["mean"] = max(H.get("mean", 0.0), h["mean"])
        g, b = I["gamma"].astype(np.float64), I["beta"].astype(np.float64)
        mu, isd, rm, rv = (A["fwd" + k].cpu().numpy().astype(np.float64) for k in ("_mean", "_isd", "_rm", "_rv"))
        isr = 1.0 / np.sqrt(rv + float(EPS))
        stats = dict(fwd=(mu, isd), act0=(mu, isd), eval=(rm, isr), act1=(rm, isr), act2=None)
        n_w = dict.fromkeys(self.acts, 0.0)
        for r0 in range(0, rows, BN_CHUNK):
            sl, ref = slice(r0, r0 + BN_CHUNK), {}
            for n in self.acts:
                st = stats[n]
                if id(st) not in ref:
                    ref[id(st)] = act_ref(I["x"][sl], None, None, None, None, raw=True) if st is None else act_ref(I["x"][sl], st[0], st[1], g, b)
                R = ref[id(st)]
                n_w[n] += check_act("%s %s rows %d.." % (name, n, r0), A[n + "_bf16"][sl], A[n + "_f32"][sl], R) * R["a"].size
        H["frac_w"] = max(n_w.values()) / (rows * C)
        bad = A.surroundings_touched()
        assert not bad, "%s: surroundings overwritten: %s" % (name, bad)
        return H


# ---- BatchNorm backward: bn_bwd_reduce, bn_bwd_apply, bn_bwd ---------------------------------------------------------------------------------
BWD_CASES = (
    dict(id="bwd-c16-r300", C=16, rows=300, resid=True, ranks=1, seed=1),
    dict(id="bwd-c2-r130", C=2, rows=130, resid=False, ranks=1, seed=2),
    dict(id="bwd-c256-r1000", C=256, rows=1000, resid=True, ranks=1, seed=3),
    dict(id="bwd-c16-2ranks", C=16, rows=150, resid=True, ranks=2, seed=4),
    dict(id="bwd-c4-2ranks-noresid", C=4, rows=257, resid=False, ranks=2, seed=5),
    # 40 rows per workgroup, 16 per trip of bn_reduce_kernel's row loop: three trips, the last with two of its four rows in flight valid
    dict(id="bwd-c256-r20001-3trips", C=256, rows=20001, resid=False, ranks=1, seed=6),
)


def bwd_ref(x, dact, mu, isd, g, b, resid, slope=float(SLOPE), kink_one=False):
    """float64 backward of LeakyReLU(BatchNorm(x)) over all rows (mu / isd: the saved statistics as float64): dict(dx, s1, s2, xh, d, yv)"""
    xh = (x - mu) * isd
    yv = g * xh + b
    d = dact * np.where((yv >= 0) if kink_one else (yv > 0), 1.0, slope)
    s1, s2 = d.sum(0), (d * xh).sum(0)
    n = float(x.shape[0])
    dx = g * isd * (d - s1 / n - xh * (s2 / n))
    return dict(dx=dx + (resid if resid is not None else 0.0), s1=s1, s2=s2, xh=xh, d=d, yv=yv)


def bwd32(x, dact, mu, isd, g, b, resid, tot, n_total, slope=SLOPE):
    """bn_bwd_apply_kernel / bn_reduce_kernel<true> in float32 (numpy rounds every operation): (dx, s1, s2 (float64 sums of fp32 terms))"""
    xh = ((x - mu).astype(np.float32) * isd).astype(np.float32)
    yv = ((g * xh).astype(np.float32) + b).astype(np.float32)
    dy = (dact * np.where(yv > 0, np.float32(1.0), np.float32(slope))).astype(np.float32)
    s1, s2 = dy.astype(np.float64).sum(0), (dy.astype(np.float64) * xh.astype(np.float64)).sum(0)
    if tot is None:
        return None, s1, s2
    C = x.shape[1]
    m1, m2 = (tot[:C] / n_total).astype(np.float32), (tot[C:] / n_total).astype(np.float32)
    v = ((g * isd).astype(np.float32) * ((dy - m1).astype(np.float32) - (xh * m2).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return (v if resid is None else (resid + v).astype(np.float32)), s1, s2


class BwdLaunch:
    """ranks = 2: two halves of `rows` rows each on one device: reduce each, add the totals, apply each with local_totals = its own sums and
    rows_total = 2 rows; the result must be the float64 backward of the full-batch BatchNorm.  ranks = 1 also runs srhip_bn_bwd."""

    def __init__(self, c, device):
        self.c, self.device = c, device
        C, rows, R = c["C"], c["rows"], c["ranks"]
        rng = _rng(c["seed"], 0xBD)
        n = rows * R
        I = dict(x=bn_x(rng, n, C), dact=rng.standard_normal((n, C), dtype=np.float32))
        I["gamma"], I["beta"] = planted_affine(rng, C)
        if C <= 3:                                           # (no room for the planted channels of planted_affine: the kink channel is channel 1)
            I["gamma"][1] = 0.0
            I["beta"][1] = 0.0
        if c["resid"]:
            I["resid"] = rng.standard_normal((n, C), dtype=np.float32)
        x64 = I["x"].astype(np.float64)
        m = x64.mean(0)
        v = np.maximum((x64 * x64).mean(0) - m * m, 0.0)
        I["mean"], I["isd"] = m.astype(np.float32), (1.0 / np.sqrt(v + float(EPS))).astype(np.float32)
        I["dg0"], I["db0"] = rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
        self.I = I
        A = self.A = Arena(device)
        f = torch.from_numpy
        for k in ("gamma", "beta", "mean", "isd"):
            A.read(k, f(I[k]))
        for r in range(R):
            sl = slice(r * rows, (r + 1) * rows)
            A.read("x%d" % r, f(I["x"][sl]))
            A.read("dact%d" % r, f(I["dact"][sl]))
            if c["resid"]:
                A.read("resid%d" % r, f(I["resid"][sl]))
            A.write("ws%d" % r, torch.zeros(WS_DOUBLES, dtype=torch.float64))
            A.write("dx%d" % r, nan_like((rows, C)))
            A.write("dxb%d" % r, nan_like((rows, C), torch.bfloat16))
            A.write("dg%d" % r, f(I["dg0"]))
            A.write("db%d" % r, f(I["db0"]))
        A.write("totals", nan_like((2 * C,), torch.float64))
        if R == 1:
            A.write("ws_one", torch.zeros(WS_DOUBLES, dtype=torch.float64))
            A.write("dx_one", nan_like((rows, C)))
            A.write("dg_one", f(I["dg0"]))
            A.write("db_one", f(I["db0"]))

    def _resid(self, r):
        return self.A["resid%d" % r] if self.c["resid"] else None

    def run_hip(self):
        A, C, rows, R, s = self.A, self.c["C"], self.c["rows"], self.c["ranks"], float(SLOPE)
        st = (A["mean"], A["isd"], A["gamma"], A["beta"])
        for r in range(R):
            ops.bn_bwd_reduce(A["dact%d" % r], A["x%d" % r], *st, s, A["ws%d" % r], rows, C)
        A["totals"].copy_(sum(A["ws%d" % r][:2 * C] for r in range(R)))
        for r in range(R):
            ops.bn_bwd_apply(A["dact%d" % r], A["x%d" % r], *st, s, self._resid(r), A["dx%d" % r], A["dg%d" % r], A["db%d" % r], A["totals"],
                             A["ws%d" % r] if R > 1 else None, R * rows, rows, C, dx_bf16=A["dxb%d" % r])
        if R == 1:
            ops.bn_bwd(A["dact0"], A["x0"], *st, s, self._resid(0), A["dx_one"], A["dg_one"], A["db_one"], A["ws_one"], rows, C)

    def restate(self, fault=None):
        A, I, C, rows, R = self.A, self.I, self.c["C"], self.c["rows"], self.c["ranks"]
        f = torch.from_numpy
        slope = SLOPE
        st = (I["mean"], I["isd"], I["gamma"], I["beta"])

        def terms(sl):
            if fault == "kink_derivative_one":             # yv >= 0 takes the derivative 1
                xh = ((I["x"][sl] - st[0]).astype(np.float32) * st[1]).astype(np.float32)
                yv = ((st[2] * xh).astype(np.float32) + st[3]).astype(np.float32)
                dy = (I["dact"][sl] * np.where(yv >= 0, np.float32(1.0), slope)).astype(np.float32)
                return dy.astype(np.float64).sum(0), (dy.astype(np.float64) * xh.astype(np.float64)).sum(0)
            return bwd32(I["x"][sl], I["dact"][sl], *st, None, None, None)[1:]
        loc = []
        for r in range(R):
            s1, s2 = terms(slice(r * rows, (r + 1) * rows))
            loc.append(np.concatenate([s1, s2]))
            A["ws%d" % r][:2 * C].copy_(f(loc[r]))
        tot = sum(loc)
        A["totals"].copy_(f(tot))
        n_total = rows if fault == "rows_instead_of_rows_total" else R * rows
        for r in range(R):
            sl = slice(r * rows, (r + 1) * rows)
            dx = bwd32(I["x"][sl], I["dact"][sl], *st, I["resid"][sl] if self.c["resid"] else None, tot, n_total)[0]
            A["dx%d" % r].copy_(f(dx))
            A["dxb%d" % r].copy_(to_bf16(dx))
            A["db%d" % r].copy_(f((I["db0"] + loc[r][:C].astype(np.float32)).astype(np.float32)))
            A["dg%d" % r].copy_(f((I["dg0"] + loc[r][C:].astype(np.float32)).astype(np.float32)))
        if R == 1:
            A["ws_one"][:2 * C].copy_(f(tot))
            A["dx_one"].copy_(A["dx0"])
            A["dg_one"].copy_(A["dg0"])
            A["db_one"].copy_(A["db0"])

    def expect(self):
        """Bounds.  mag = |x - mu| invstd is what xhat's two roundings are relative to.  A sum's terms are fp32 values added in fp64:
        tol_s1 = C_BWD 2^-24 sum |d|, tol_s2 = C_BWD 2^-24 sum |d| mag; dx: C_BWD 2^-24 (|gamma| invstd (|d| + |s1| / n + mag |s2| / n) + |dx|) +
        2^-24 |resid| + |gamma| invstd (tol_s1 + mag tol_s2) / n.  An element whose float64 pre-activation is within r of zero may take either
        derivative: (1 - slope) |dact| is added to its own bound and to the sums' (the kink channel has r = 0: its derivative is the slope)."""
        I, C, rows, R = self.I, self.c["C"], self.c["rows"], self.c["ranks"]
        g, b = I["gamma"].astype(np.float64), I["beta"].astype(np.float64)
        mu, isd = I["mean"].astype(np.float64), I["isd"].astype(np.float64)
        x, dact = I["x"].astype(np.float64), I["dact"].astype(np.float64)
        resid = I["resid"].astype(np.float64) if self.c["resid"] else None
        F = bwd_ref(x, dact, mu, isd, g, b, resid)
        n = float(R * rows)
        mag = np.abs(x - mu) * isd
        r = C_R * U24 * (np.abs(g) * mag + np.abs(b))
        amb = (np.abs(F["yv"]) <= r) & (r > 0)
        flip = np.where(amb, (1.0 - float(SLOPE)) * np.abs(dact), 0.0)
        ad = np.abs(F["d"])
        ts1 = lambda sl: C_BWD * U24 * ad[sl].sum(0) + flip[sl].sum(0)
        ts2 = lambda sl: C_BWD * U24 * (ad[sl] * mag[sl]).sum(0) + (flip[sl] * mag[sl]).sum(0)
        al = slice(None)
        dxt = C_BWD * U24 * (np.abs(g) * isd * (ad + np.abs(F["s1"]) / n + mag * np.abs(F["s2"]) / n) + np.abs(F["dx"])) \
            + (U24 * np.abs(resid) if resid is not None else 0.0) + np.abs(g) * isd * (flip + (ts1(al) + mag * ts2(al)) / n)
        loc = []
        for q in range(R):
            sl = slice(q * rows, (q + 1) * rows)
            loc.append(dict(s1=F["d"][sl].sum(0), s2=(F["d"][sl] * F["xh"][sl]).sum(0), t1=ts1(sl), t2=ts2(sl)))
        return dict(F=F, dx=F["dx"], dxt=dxt, loc=loc, frac_amb=float(amb.mean()), ts1=ts1(al), ts2=ts2(al))

    def verify(self):
        A, I, C, rows, R, name = self.A, self.I, self.c["C"], self.c["rows"], self.c["ranks"], self.c["id"]
        ex = self.expect()
        H = {}
        tot = A["totals"].cpu().numpy()
        H["sums"] = max(worst(name + " total sum d", tot[:C], ex["F"]["s1"], ex["ts1"]), worst(name + " total sum d xhat", tot[C:], ex["F"]["s2"], ex["ts2"]))
        outs = [(r, "dx%d" % r, "dg%d" % r, "db%d" % r, "ws%d" % r) for r in range(R)] + ([(0, "dx_one", "dg_one", "db_one", "ws_one")] if R == 1 else [])
        for r, dxn, dgn, dbn, wsn in outs:
            sl, L = slice(r * rows, (r + 1) * rows), ex["loc"][r]
            H["dx"] = max(H.get("dx", 0.0), worst("%s %s" % (name, dxn), A[dxn].cpu().numpy(), ex["dx"][sl], ex["dxt"][sl]))
            # d(gamma), d(beta) += (float)local sum: the sum's bound, one rounding of it, one of the addition
            for what, got, s, t, init in (("dbeta", A[dbn], L["s1"], L["t1"], I["db0"]), ("dgamma", A[dgn], L["s2"], L["t2"], I["dg0"])):
                want = init.astype(np.float64) + s
                H["dparam"] = max(H.get("dparam", 0.0), worst("%s %s %s" % (name, dgn, what), got.cpu().numpy(), want, t + U24 * np.abs(s) + U24 * np.abs(want)))
            w = A[wsn].cpu().numpy()
            H["sums"] = max(H["sums"], worst(name + " " + wsn, w[:2 * C], np.concatenate([L["s1"], L["s2"]]), np.concatenate([L["t1"], L["t2"]])))
            assert not w[2 * C:].view(np.int64).any(), "%s: the arrival counter or an accumulator copy is not zero after the launch" % name
        for r in range(R):
            assert torch.equal(bits(A["dxb%d" % r]), bits(A["dx%d" % r].to(torch.bfloat16))), "%s: dx_bf16 is not the round-to-nearest bf16 of the stored dx" % name
        if R == 1:          # srhip_bn_bwd is a second reduce + apply on a workspace of its own: the same bits (the fp64 sums of two launches may
            for a, b_ in (("dx_one", "dx0"), ("dg_one", "dg0"), ("db_one", "db0")):      # differ in the last bits of a double, below the fp32 values)
                assert torch.equal(bits(A[a]), bits(A[b_])), "%s: the second launch (srhip_bn_bwd) gave other bits in %s" % (name, a)
        H["frac_amb"] = ex["frac_amb"]
        bad = A.surroundings_touched()
        assert not bad, "%s: surroundings overwritten: %s" % (name, bad)
        return H


def measure_c_bwd():
    """largest |float32 restatement - float64| / (2^-24 magnitude) of dx and of the two sums over BWD_CASES (ambiguous elements excluded)"""
    worst_ = 0.0
    for c in BWD_CASES:
        L = BwdLaunch(c, "cpu")
        I, C, n = L.I, c["C"], c["rows"] * c["ranks"]
        ex = L.expect()
        F = ex["F"]
        g, isd, mu = I["gamma"].astype(np.float64), I["isd"].astype(np.float64), I["mean"].astype(np.float64)
        mag = np.abs(I["x"].astype(np.float64) - mu) * isd
        r = C_R * U24 * (np.abs(g) * mag + np.abs(I["beta"].astype(np.float64)))
        amb = (np.abs(F["yv"]) <= r) & (r > 0)
        _, s1, s2 = bwd32(I["x"], I["dact"], I["mean"], I["isd"], I["gamma"], I["beta"], None, None, None)
        ad = np.where(amb, 0.0, np.abs(F["d"]))
        if not amb.any():
            worst_ = max(worst_, float((np.abs(s1 - F["s1"]) / (U24 * ad.sum(0))).max()), float((np.abs(s2 - F["s2"]) / (U24 * (ad * mag).sum(0) + 1e-300)).max()))
        dx = bwd32(I["x"], I["dact"], I["mean"], I["isd"], I["gamma"], I["beta"], I.get("resid"), np.concatenate([F["s1"], F["s2"]]), float(n))[0]
        m = np.abs(g) * isd * (np.abs(F["d"]) + np.abs(F["s1"]) / n + mag * np.abs(F["s2"]) / n) + np.abs(F["dx"])
        ok = ~amb & (m > 0)
        worst_ = max(worst_, float((np.abs(dx - F["dx"])[ok] / (U24 * m[ok])).max()))
    return worst_


# ---- im2col, im2col_bn, col2im ---------------------------------------------------------------------------------------------------------------------
IM_CASES = (                              # B, H, W, C, k, stride
    dict(id="im-5x7-c8-k3", shape=(2, 5, 7, 8, 3, 1)),
    dict(id="im-7x7-c16-k3-s2", shape=(2, 7, 7, 16, 3, 2)),
    dict(id="im-6x6-c8-1x1-s2", shape=(2, 6, 6, 8, 1, 2)),
    dict(id="im-5x5-c3-scalar", shape=(2, 5, 5, 3, 3, 1)),
)
C_COL = 10.0                              # col2im: at most 9 terms and the contents under accumulate = 10 operands, 9 additions (+ 1 of margin)


class ImLaunch:
    def __init__(self, c, device):
        self.c, self.device = c, device
        B, H, W, C, k, s = c["shape"]
        Ho, Wo = out_hw(H, W, k, s)
        K = k * k * C
        self.Kp, self.rows = (K + 31) // 32 * 32, B * Ho * Wo
        rng = _rng(sum(c["shape"]), 0x12C)
        I = dict(x=planted_x(rng, (B, H, W, C)) if C > 4 else rng.standard_normal((B, H, W, C), dtype=np.float32))
        I["gamma"], I["beta"] = planted_affine(rng, C)
        x64 = I["x"].astype(np.float64).reshape(-1, C)
        m = x64.mean(0)
        I["mean"], I["isd"] = m.astype(np.float32), (1.0 / np.sqrt(np.maximum((x64 * x64).mean(0) - m * m, 0) + float(EPS))).astype(np.float32)
        dcol = rng.standard_normal((self.rows, self.Kp), dtype=np.float32)
        dcol[:, K:] = np.nan                                   # col2im never reads the padding columns
        I["dcol"] = dcol
        I["dact0"] = rng.standard_normal((B, H, W, C), dtype=np.float32)
        self.I = I
        A = self.A = Arena(device)
        f = torch.from_numpy
        for n in ("x", "gamma", "beta", "mean", "isd", "dcol"):
            A.read(n, f(I[n]))
        A.read("act", to_bf16(I["x"]))
        A.write("col", nan_like((self.rows, self.Kp), torch.bfloat16))
        self.bn = C % 8 == 0
        if self.bn:
            A.write("col_bn0", nan_like((self.rows, self.Kp), torch.bfloat16))
            A.write("col_bn2", nan_like((self.rows, self.Kp), torch.bfloat16))
        A.write("dact", nan_like((B, H, W, C)))
        A.write("dact_acc", f(I["dact0"]))

    def run_hip(self):
        A, (B, H, W, C, k, s), Kp = self.A, self.c["shape"], self.Kp
        ops.im2col(A["act"], A["col"], B, H, W, C, k, s, Kp)
        if self.bn:
            ops.im2col_bn(A["x"], (A["mean"], A["isd"]), A["gamma"], A["beta"], float(SLOPE), 0, A["col_bn0"], B, H, W, C, k, s, Kp)
            ops.im2col_bn(A["x"], None, None, None, float(SLOPE), 2, A["col_bn2"], B, H, W, C, k, s, Kp)
        ops.col2im(A["dcol"], A["dact"], B, H, W, C, k, s, Kp, accumulate=False)
        ops.col2im(A["dcol"], A["dact_acc"], B, H, W, C, k, s, Kp, accumulate=True)

    def restate(self, fault=None):
        A, I, (B, H, W, C, k, s), Kp = self.A, self.I, self.c["shape"], self.Kp
        K = k * k * C

        def pad(col):
            out = np.zeros((self.rows, Kp), dtype=np.float32)
            out[:, :K] = col
            return to_bf16(out)
        A["col"].copy_(pad(im2col_ref(to_bf16(I["x"]).float().numpy(), k, s)))
        if self.bn:
            A["col_bn0"].copy_(pad(im2col_ref(act32(I["x"], I["mean"], I["isd"], I["gamma"], I["beta"])[0], k, s)))
            A["col_bn2"].copy_(pad(im2col_ref(I["x"], k, s)))
        d = I["dcol"][:, :K]
        if fault == "ignores_ty_mod_stride":                   # every tap is taken from output pixel ty / stride, divisible or not
            Ho, Wo = out_hw(H, W, k, s)
            pd = k >> 1
            out = np.zeros((B, H, W, C), dtype=np.float32)
            dv = d.reshape(B, Ho, Wo, k * k, C)
            for y in range(H):
                for x in range(W):
                    for i in range(k):
                        for j in range(k):
                            ty, tx = y + pd - i, x + pd - j
                            if ty < 0 or tx < 0 or tx % s or ty // s >= Ho or tx // s >= Wo:
                                continue
                            out[:, y, x] += dv[:, ty // s, tx // s, i * k + j]
        else:
            out = col2im_ref(d, B, H, W, C, k, s)
        A["dact"].copy_(torch.from_numpy(out))
        A["dact_acc"].copy_(torch.from_numpy((I["dact0"] + out).astype(np.float32)))

    def verify(self):
        A, I, (B, H, W, C, k, s), Kp, name = self.A, self.I, self.c["shape"], self.Kp, self.c["id"]
        K = k * k * C
        H_ = {}
        want = torch.zeros((self.rows, Kp), dtype=torch.bfloat16)
        want[:, :K] = to_bf16(im2col_ref(to_bf16(I["x"]).float().numpy(), k, s))
        assert torch.equal(bits(A["col"].cpu()), bits(want)), name + ": im2col is not a copy of its input with zero padding"
        if self.bn:
            R0 = act_ref(I["x"], I["mean"].astype(np.float64), I["isd"].astype(np.float64), I["gamma"].astype(np.float64), I["beta"].astype(np.float64))
            R2 = act_ref(I["x"], None, None, None, None, raw=True)
            for n, R in (("col_bn0", R0), ("col_bn2", R2)):
                got = A[n].double().cpu().numpy()
                assert not got[:, K:].any() and not np.signbit(got[:, K:]).any(), "%s %s: padding columns are not zeros" % (name, n)
                lo, hi = im2col_ref(R["lo"], k, s), im2col_ref(R["hi"], k, s)
                ok = (got[:, :K] >= lo) & (got[:, :K] <= hi)
                assert ok.all(), "%s %s: %d elements outside the admissible set, first at %s" % (name, n, int((~ok).sum()), np.argwhere(~ok)[0])
            H_["frac_w"] = float((R0["w"] > 0).mean())
        d64 = np.nan_to_num(I["dcol"][:, :K].astype(np.float64))
        want, S = col2im_ref(d64, B, H, W, C, k, s), col2im_ref(np.abs(d64), B, H, W, C, k, s)
        H_["col2im"] = worst(name + " col2im", A["dact"].cpu().numpy(), want, C_COL * U24 * S)
        d0 = I["dact0"].astype(np.float64)
        H_["col2im_acc"] = worst(name + " col2im accumulate", A["dact_acc"].cpu().numpy(), d0 + want, np.where(S > 0, C_COL * U24 * (S + np.abs(d0)), 0.0))
        bad = A.surroundings_touched()
        assert not bad, "%s: surroundings overwritten: %s" % (name, bad)
        return H_


# ---- filter layouts: conv_weight_prep(_grouped), conv_weight_flip_grouped, add_unpad(_grouped) ---------------------------------------------------
WEIGHT_TABLES = (                          # entries (Cout, C, k); Kpad = K rounded up to 32
    dict(id="w-three", entries=((5, 3, 3), (16, 8, 1), (32, 16, 3))),           # entry 1 starts at 160, entry 2 at 672: no multiple of 256
    dict(id="w-single", entries=((7, 6, 3),)),
)
FLIP_TABLES = (                            # entries (Cout, Cin) of 3 x 3 layers, Cin != Cout
    dict(id="flip-three", entries=((16, 3), (32, 16), (8, 24))),                # W' has Cin * Kpad elements: entry 1 starts at 480
    dict(id="flip-single", entries=((16, 32),)),
)


class WeightLaunch:
    """One table: the grouped launches, and every entry again through the single launches."""

    def __init__(self, c, device, flip=False):
        self.c, self.device, self.flip = c, device, flip
        rng = _rng(len(c["entries"]), 0xF17 + flip)
        A = self.A = Arena(device)
        self.E = []
        for i, e in enumerate(c["entries"]):
            Cout, C, k = (e[0], e[1], 3) if flip else e
            if flip:
                Kp = (9 * Cout + 31) // 32 * 32
                Wf = rng.permuted(np.tile(np.arange(1, 10, dtype=np.float32), (Cout, C, 1)), axis=2).reshape(Cout, C, 3, 3)   # nine distinct taps
                Wf = (Wf * rng.uniform(0.5, 1.5, (Cout, C, 1, 1))).astype(np.float32)
                A.read("W%d" % i, torch.from_numpy(Wf))
                A.write("flip%d" % i, nan_like((C, Kp), torch.bfloat16))
            else:
                K = k * k * C
                Kp = (K + 31) // 32 * 32
                Wf = rng.standard_normal((Cout, C, k, k)).astype(np.float32)
                src = rng.standard_normal((Cout, Kp)).astype(np.float32)
                src[:, K:] = np.nan                                                   # add_unpad never reads the padding columns
                dW0 = rng.standard_normal((Cout, C, k, k)).astype(np.float32)
                A.read("W%d" % i, torch.from_numpy(Wf))
                A.read("src%d" % i, torch.from_numpy(src))
                for tag in ("g", "s"):
                    A.write("Wb%s%d" % (tag, i), nan_like((Cout, Kp), torch.bfloat16))
                    A.write("WbT%s%d" % (tag, i), nan_like((Kp, Cout), torch.bfloat16))
                    A.write("dW%s%d" % (tag, i), torch.from_numpy(dW0))
                self.E.append(dict(Cout=Cout, C=C, k=k, Kp=Kp, Wf=Wf, src=src, dW0=dW0))
                continue
            self.E.append(dict(Cout=Cout, C=C, k=3, Kp=Kp, Wf=Wf))

    def run_hip(self):
        A, E = self.A, self.E
        if self.flip:
            desc, n, total = ops.make_conv_desc([(A["W%d" % i], A["flip%d" % i], None, e["Cout"], e["C"], 3, e["Kp"]) for i, e in enumerate(E)],
                                                self.device, lambda Cout, C, kk, Kpad: C * Kpad)
            ops.conv_weight_flip_grouped(desc, n, total)
            return
        desc, n, total = ops.make_conv_desc([(A["W%d" % i], A["Wbg%d" % i], A["WbTg%d" % i], e["Cout"], e["C"], e["k"], e["Kp"]) for i, e in enumerate(E)],
                                            self.device, lambda Cout, C, kk, Kpad: Cout * Kpad)
        ops.conv_weight_prep_grouped(desc, n, total)
        desc, n, total = ops.make_conv_desc([(A["src%d" % i], A["dWg%d" % i], None, e["Cout"], e["C"], e["k"], e["Kp"]) for i, e in enumerate(E)],
                                            self.device, lambda Cout, C, kk, Kpad: Cout * C * kk)
        ops.add_unpad_grouped(desc, n, total)
        for i, e in enumerate(E):
            ops.conv_weight_prep(A["W%d" % i], A["Wbs%d" % i], A["WbTs%d" % i], e["Cout"], e["C"], e["k"], e["Kp"])
            ops.add_unpad(A["src%d" % i], A["dWs%d" % i], e["Cout"], e["C"], e["k"], e["Kp"])

    def restate(self):
        A = self.A
        for i, e in enumerate(self.E):
            if self.flip:
                A["flip%d" % i].copy_(flip_ref(e["Wf"], e["Kp"]))
                continue
            Wb, WbT = prep_ref(e["Wf"], e["Kp"])
            add = unpad_ref(np.nan_to_num(e["src"]), e["Cout"], e["C"], e["k"] ** 2, e["Kp"]).reshape(e["dW0"].shape)
            for tag in ("g", "s"):
                A["Wb%s%d" % (tag, i)].copy_(Wb)
                A["WbT%s%d" % (tag, i)].copy_(WbT)
                A["dW%s%d" % (tag, i)].copy_(torch.from_numpy((e["dW0"] + add).astype(np.float32)))

    def verify(self):
        A, name = self.A, self.c["id"]
        for i, e in enumerate(self.E):
            if self.flip:
                assert torch.equal(bits(A["flip%d" % i].cpu()), bits(flip_ref(e["Wf"], e["Kp"]))), "%s entry %d: flipped filter" % (name, i)
                continue
            Wb, WbT = prep_ref(e["Wf"], e["Kp"])
            add = unpad_ref(np.nan_to_num(e["src"]), e["Cout"], e["C"], e["k"] ** 2, e["Kp"]).reshape(e["dW0"].shape)
            dW = torch.from_numpy((e["dW0"] + add).astype(np.float32))                # one fp32 addition: the same bits
            for tag in ("g", "s"):
                assert torch.equal(bits(A["Wb%s%d" % (tag, i)].cpu()), bits(Wb)), "%s entry %d (%s): Wb" % (name, i, tag)
                assert torch.equal(bits(A["WbT%s%d" % (tag, i)].cpu()), bits(WbT)), "%s entry %d (%s): WbT" % (name, i, tag)
                assert torch.equal(bits(A["dW%s%d" % (tag, i)].cpu()), bits(dW)), "%s entry %d (%s): add_unpad" % (name, i, tag)
        bad = A.surroundings_touched()
        assert not bad, "%s: surroundings overwritten: %s" % (name, bad)
        return {}


# ---- classifier, pooling, input layout ------------------------------------------------------------------------------------------------------------
FC_CASES = tuple(dict(id="fc-f%d-k%d" % (F, K), B=B, F=F, K=K) for B, F, K in ((3, 64, 1), (2, 130, 3), (5, 768, 5), (3, 130, 100), (2, 64, 5)))


class FcLaunch:
    """fc_fwd / fc_bwd (+ avgpool over HW2 = 7 pixels of F channels, B * 7 * F is a multiple of 64 only for some cases: the others must be refused)."""

    def __init__(self, c, device):
        self.c, self.device = c, device
        B, F, K = c["B"], c["F"], c["K"]
        rng = _rng(B, F, K, 0xFC)
        I = dict(feat=rng.standard_normal((B, F), dtype=np.float32), Wc=(rng.standard_normal((K, F)) / math.sqrt(F)).astype(np.float32),
                 bc=rng.standard_normal(K).astype(np.float32), dl=rng.standard_normal((B, K), dtype=np.float32),
                 dW0=rng.standard_normal((K, F), dtype=np.float32), db0=rng.standard_normal(K).astype(np.float32))
        self.I = I
        A = self.A = Arena(device)
        for n in ("feat", "Wc", "bc", "dl"):
            A.read(n, torch.from_numpy(I[n]))
        A.write("logits", nan_like((B, K)))
        A.write("dfeat", nan_like((B, F)))
        A.write("dWc", torch.from_numpy(I["dW0"]))
        A.write("dbc", torch.from_numpy(I["db0"]))

    def run_hip(self):
        A, c = self.A, self.c
        ops.fc_fwd(A["feat"], A["Wc"], A["bc"], A["logits"], c["B"], c["F"], c["K"])
        ops.fc_bwd(A["dl"], A["feat"], A["Wc"], A["dfeat"], A["dWc"], A["dbc"], c["B"], c["F"], c["K"])

    def restate(self):
        A, I = self.A, self.I
        f = torch.from_numpy
        A["logits"].copy_(f(((I["feat"] @ I["Wc"].T).astype(np.float32) + I["bc"]).astype(np.float32)))
        A["dfeat"].copy_(f((I["dl"] @ I["Wc"]).astype(np.float32)))
        A["dWc"].copy_(f((I["dW0"] + (I["dl"].T @ I["feat"]).astype(np.float32)).astype(np.float32)))
        A["dbc"].copy_(f((I["db0"] + I["dl"].sum(0, dtype=np.float32)).astype(np.float32)))

    def verify(self):
        """Worst-case counts of fp32 roundings, each at most 2^-24 of the sum of the absolute terms: logits ceil(F / 64) products and additions
        per lane + 6 steps of the wave sum + the bias; dfeat K products and additions + 3 partial sums; dWc / dbc B products and additions + the
        contents they are added to."""
        A, I, c, name = self.A, self.I, self.c, self.c["id"]
        B, F, K = c["B"], c["F"], c["K"]
        ft, W, bc, dl = (I[n].astype(np.float64) for n in ("feat", "Wc", "bc", "dl"))
        H = dict(fc_fwd=worst(name + " logits", A["logits"].cpu().numpy(), ft @ W.T + bc,
                              (2 * ((F + 63) // 64) + 8) * U24 * (np.abs(ft) @ np.abs(W).T + np.abs(bc))))
        H["fc_bwd_x"] = worst(name + " dfeat", A["dfeat"].cpu().numpy(), dl @ W, (2 * K + 4) * U24 * (np.abs(dl) @ np.abs(W)))
        H["fc_bwd_w"] = max(
            worst(name + " dWc", A["dWc"].cpu().numpy(), I["dW0"] + dl.T @ ft, (2 * B + 2) * U24 * (np.abs(I["dW0"]) + np.abs(dl).T @ np.abs(ft))),
            worst(name + " dbc", A["dbc"].cpu().numpy(), I["db0"] + dl.sum(0), (B + 2) * U24 * (np.abs(I["db0"]) + np.abs(dl).sum(0))))
        bad = A.surroundings_touched()
        assert not bad, "%s: surroundings overwritten: %s" % (name, bad)
        return H


POOL_CASES = (dict(id="pool-b2-hw64-c32", B=2, HW2=64, C=32), dict(id="pool-b4-hw7-c16", B=4, HW2=7, C=16), dict(id="pool-b3-hw7-c5-refused", B=3, HW2=7, C=5))


class PoolLaunch:
    """avgpool_fwd, avgpool_bwd (refused when B * HW2 * C is no multiple of 64: the output pattern stays), nchw_to_nhwc_bf16 with 3 channels."""

    def __init__(self, c, device):
        self.c, self.device = c, device
        B, HW2, C = c["B"], c["HW2"], c["C"]
        rng = _rng(B, HW2, C, 0xA9)
        self.I = dict(act=rng.standard_normal((B, HW2, C), dtype=np.float32), dfeat=rng.standard_normal((B, C), dtype=np.float32),
                      img=rng.standard_normal((B, 3, HW2, 5), dtype=np.float32))
        A = self.A = Arena(device)
        for n in ("act", "dfeat", "img"):
            A.read(n, torch.from_numpy(self.I[n]))
        A.write("feat", nan_like((B, C)))
        A.write("dact", nan_like((B, HW2, C)))
        A.write("nhwc", nan_like((B, HW2, 5, 3), torch.bfloat16))
        self.refused = (B * HW2 * C) % 64 != 0

    def run_hip(self):
        A, c = self.A, self.c
        ops.avgpool_fwd(A["act"], A["feat"], c["B"], c["HW2"], c["C"])
        try:
            ops.avgpool_bwd(A["dfeat"], A["dact"], c["B"], c["HW2"], c["C"])
            self.raised = False
        except RuntimeError:
            self.raised = True
        ops.nchw_to_nhwc_bf16(A["img"], A["nhwc"], c["B"], 3, c["HW2"], 5)

    def restate(self):
        A, I, c = self.A, self.I, self.c
        s = np.zeros((c["B"], c["C"]), dtype=np.float32)
        for p in range(c["HW2"]):
            s = (s + I["act"][:, p]).astype(np.float32)
        A["feat"].copy_(torch.from_numpy((s / np.float32(c["HW2"])).astype(np.float32)))
        self.raised = self.refused
        if not self.refused:
            A["dact"].copy_(torch.from_numpy(np.broadcast_to((I["dfeat"] / np.float32(c["HW2"])).astype(np.float32)[:, None], I["act"].shape).copy()))
        A["nhwc"].copy_(to_bf16(I["img"].transpose(0, 2, 3, 1)))

    def verify(self):
        A, I, c, name = self.A, self.I, self.c, self.c["id"]
        a = I["act"].astype(np.float64)
        H = dict(avgpool_fwd=worst(name + " feat", A["feat"].cpu().numpy(), a.mean(1), (c["HW2"] + 1) * U24 * np.abs(a).mean(1)))     # HW2 additions, one division
        assert self.raised == self.refused, name + ": avgpool_bwd refuses exactly the sizes that are no multiple of 64"
        if self.refused:
            assert bool(torch.isnan(A["dact"]).all()), name + ": a refused avgpool_bwd wrote"
        else:
            want = np.broadcast_to((I["dfeat"] / np.float32(c["HW2"])).astype(np.float32)[:, None], I["act"].shape)                    # one division: the same bits
            assert np.array_equal(A["dact"].cpu().numpy().view(np.int32), np.ascontiguousarray(want).view(np.int32)), name + ": avgpool_bwd"
        assert torch.equal(bits(A["nhwc"].cpu()), bits(to_bf16(I["img"].transpose(0, 2, 3, 1)))), name + ": nchw_to_nhwc_bf16"
        bad = A.surroundings_touched()
        assert not bad, "%s: surroundings overwritten: %s" % (name, bad)
        return H


# ---- srhip_sgd_flat ---------------------------------------------------------------------------------------------------------------------------------
SGD_ENDS = (256, 511, 1025)               # chunk ends at, one below and one above a multiple of 256; n = 1025 is no multiple of 256
SGD_WD = (5e-4, 0.0, 5e-4)
SGD_CASES = tuple(dict(id="sgd-%s%s%s%s" % ("first" if fs else "later", "-clip" if cl else "", "-ema" if em else "", "-keepgrad" if not zg else ""),
                       first=fs, clip=cl, ema=em, zero=zg)
                  for fs, cl, em, zg in ((True, False, False, True), (False, True, True, True), (False, False, True, False), (True, True, False, False),
                                         (False, False, False, True)))
SGD_LR, SGD_MOM, SGD_SCALE, SGD_EMA = np.float32(0.03), np.float32(0.9), np.float32(0.5), 0.999


class SgdLaunch:
    def __init__(self, c, device):
        self.c, self.device = c, device
        n = SGD_ENDS[-1]
        rng = _rng(c["first"], c["clip"], c["ema"], c["zero"], 0x56D)
        I = dict(p=rng.standard_normal(n, dtype=np.float32), g=rng.standard_normal(n, dtype=np.float32), buf=rng.standard_normal(n, dtype=np.float32),
                 ema=rng.standard_normal(n, dtype=np.float32), clip=np.array([0.37, 2.5], dtype=np.float32))
        tab = np.zeros(3, dtype=[("end", "<i8"), ("wd", "<f4"), ("pad", "<f4")])
        tab["end"], tab["wd"] = SGD_ENDS, SGD_WD
        self.I, self.n = I, n
        A = self.A = Arena(device)
        self.table = torch.from_numpy(tab.view(np.uint8).copy()).to(device)
        A.read("clip", torch.from_numpy(I["clip"]))
        for k in ("p", "g", "buf", "ema"):
            A.write(k, torch.from_numpy(I[k]))

    def run_hip(self):
        A, c = self.A, self.c
        ops.sgd_flat(A["p"], A["g"], A["buf"], A["ema"] if c["ema"] else None, self.table, 3, self.n, float(SGD_LR), float(SGD_MOM),
                     grad_scale=float(SGD_SCALE), ema_m=SGD_EMA if c["ema"] else 0.0, first_step=c["first"], zero_grad=c["zero"],
                     clip_coef=A["clip"] if c["clip"] else None)

    def wd(self, fault=None):
        w = np.zeros(self.n, dtype=np.float32)
        lo = 0
        for e, v in zip(SGD_ENDS, SGD_WD):
            w[lo:e] = v
            lo = e
        if fault == "wd_on_flag0_first_element":
            w[SGD_ENDS[0]] = SGD_WD[0]
        return w

    def ema_statement(self, p_stored):
        """misc.py:154 as two fp32 products and their fp32 sum, on the p the launch stored"""
        m, one_m = np.float32(SGD_EMA), np.float32(1.0 - SGD_EMA)
        return ((one_m * p_stored).astype(np.float32) + (m * self.I["ema"]).astype(np.float32)).astype(np.float32)

    def restate(self, fault=None):
        A, I, c = self.A, self.I, self.c
        wd = self.wd(fault)
        sc = np.float32(SGD_SCALE * I["clip"][0]) if c["clip"] else SGD_SCALE
        d = (I["g"] * sc).astype(np.float32)
        d = np.where(wd != 0, (d + (wd * I["p"]).astype(np.float32)).astype(np.float32), d)
        b = d if c["first"] else ((SGD_MOM * I["buf"]).astype(np.float32) + d).astype(np.float32)
        p = (I["p"] - (SGD_LR * (d + (SGD_MOM * b).astype(np.float32)).astype(np.float32)).astype(np.float32)).astype(np.float32)
        f = torch.from_numpy
        A["p"].copy_(f(p))
        A["buf"].copy_(f(b))
        if c["ema"]:
            A["ema"].copy_(f(self.ema_statement(p)))
        if c["zero"]:
            A["g"].zero_()

    def expect(self):
        I, c = self.I, self.c
        p, g, buf = (I[k].astype(np.float64) for k in ("p", "g", "buf"))
        wd = self.wd().astype(np.float64)
        sc = float(SGD_SCALE) * (float(I["clip"][0]) if c["clip"] else 1.0)
        d = g * sc + wd * p
        D = np.abs(g * sc) + np.abs(wd * p)
        b = d if c["first"] else float(SGD_MOM) * buf + d
        Bm = D if c["first"] else float(SGD_MOM) * np.abs(buf) + D
        pn = p - float(SGD_LR) * (d + float(SGD_MOM) * b)
        return dict(p=pn, buf=b, ptol=C_SGD * U24 * (np.abs(p) + float(SGD_LR) * (D + float(SGD_MOM) * Bm)), btol=C_SGD * U24 * Bm)

    def verify(self):
        A, I, c, name = self.A, self.I, self.c, self.c["id"]
        ex = self.expect()
        ps = A["p"].cpu().numpy()
        H = dict(p=worst(name + " p", ps, ex["p"], ex["ptol"]), buf=worst(name + " buf", A["buf"].cpu().numpy(), ex["buf"], ex["btol"]))
        want_ema = self.ema_statement(ps) if c["ema"] else I["ema"]
        assert np.array_equal(A["ema"].cpu().numpy().view(np.int32), want_ema.view(np.int32)), name + ": the EMA is not the two-products-and-a-sum statement"
        want_g = np.zeros_like(I["g"]) if c["zero"] else I["g"]
        assert np.array_equal(A["g"].cpu().numpy().view(np.int32), want_g.view(np.int32)), name + ": g after the launch"
        bad = A.surroundings_touched()
        assert not bad, "%s: surroundings overwritten: %s" % (name, bad)
        return H


def measure_c_sgd():
    """largest |float32 restatement - float64| / (2^-24 magnitude) of p and buf over SGD_CASES"""
    worst_ = 0.0
    for c in SGD_CASES:
        L = SgdLaunch(c, "cpu")
        L.restate()
        ex = L.expect()
        worst_ = max(worst_, float((np.abs(L.A["p"].numpy() - ex["p"]) / (ex["ptol"] / C_SGD)).max()),
                     float((np.abs(L.A["buf"].numpy() - ex["buf"]) / (ex["btol"] / C_SGD)).max()))
    return worst_
