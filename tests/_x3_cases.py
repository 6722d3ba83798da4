"""The cases of tests/test_{cpu,gpu}_x3_cases.py: every split-bf16 ("bf16x3") kernel of csrc/x3.hip
(gemm_x3_kernel NT with the three epilogues of srhip_gemm_nt_x3, NT GELU_PRE and NN F32 / ACC / DGELU of srhip_gemm_x3, the grouped TN weight-gradient kernel with its
dbias column sums, attn_fwd_x3 with and without lse, both roles of attn_bwd_x3) and the fp32-output LayerNorm the x3 chain runs twice per block,
element by element against float64.  Nothing is stored: every input is rebuilt from its seed, every expected value is recomputed.  Importing
this module launches nothing and does not touch CUDA.

Why element by element: the whole-tensor rel-L2 thresholds of test_gpu_read_rows_precision.py / test_gpu_grad_rows_precision.py (1e-5 .. 5e-5)
move by 1 / sqrt(rows) of a row's own relative error; a lo plane dropped in one k-step of one 16-row fragment (2^-9 instead of 2^-17 there) is
invisible in them.  tests/test_cpu_x3_cases.py plants eighteen such faults, states what the norms read at the old tests' own shapes
(NORM_BLIND lists the ones they let pass) and shows verify() rejecting every one.

Arenas.  Every operand and output lies inside a larger allocation at a 16-byte-aligned non-zero offset (FRONT floats) with a real pitch
(lda = K + 4, ldw = K + 8, ldb = N + 4, ldc = N + 4 or N + 3, ldaux = N + 4 / N + 8).  Operand padding (front, pitch columns, ROWS_AFTER rows
after the last) is NaN; output padding holds PATTERN32 and must come back bit for bit; an overwriting output starts as NaN inside its block,
an accumulating one (RESID, ACC, the TN product, dbias) starts non-zero.  Every launch is made twice and must give the same bits.

Single products (both operands visible).  The test splits the operands itself, hi = bf16_rne(x), lo = bf16_rne(x - hi), r = x - hi - lo, and
holds the kernel to two statements, both per element:
  (1) what it is specified to compute: want3 = ah.bh + ah.bl + al.bh in float64, |got - want3| <= C_X3 2^-24 S3 (+ the epilogue's terms),
      S3 = |ah||bh| + |ah||bl| + |al||bh| (+ |bias|, + |C0| where it accumulates).  bf16 x bf16 products are exact in fp32, only the
      accumulation rounds; this bound is ~2^-7 of the x3 error itself, so a cross term missing at one k position of one element fails it.
  (2) what it is for: |got - a.b| <= bound (1) + E, E = |al||bl| + |ra||b| + |a||rb|, exact, no constant.
Epilogues: RESID multiplies product, bias and bound by |s| and adds 2^-23 |want| (rows of scale 0 equal the residual by value); GELU_F32 has no
visible pre-activation: L = 1.13 times the product's bound plus gelu_fn_tol = C_FN 2^-24 (|v / 2| (1 + |erf| + |t| erf'(t)) + |want|), the
first-order terms of the fp32 operations of 0.5 v (1 + erff(t)), t = v / sqrt 2 (C_FN measured on the float32 restatement over a grid of
fp32 arguments, like DGELU_ABS), plus FN_ULP ulps of erff;
GELU_PRE: aux_out is held to (1) and (2), C to the float64 GELU of the aux_out the kernel wrote (gelu_fn_tol alone); DGELU: |GELU'(aux)|
times the product's bound plus dgelu_abs(aux) |v|, the derivative formula's error being absolute in GELU' (it crosses 0) -- DGELU_ABS is
measured on the float32 restatement of dgelu_erf over a grid of fp32 arguments in -10 .. 10, the device functions add FN_ULP ulps of erf and
of exp.  dbias: plain fp32 column sums, C_X3 2^-24 (sum |A| + |dbias0|).

Chained kernels (attention).  Probabilities and dS are split inside the kernel from values the test cannot see; the bound is the first-order
propagation of tests/_attn_cases.py with every "half a bf16 ulp" replaced by the x3 residue of that value:
  a score / dP entry (operands visible)   es = scale E_qk (no constant) + fp32 term tau_qk = scale S3_qk + |S_qk| + |max or lse| + 1
  an operand made in the kernel           relative 2^-16 (|lo error| <= 2^-8 . 2^-8) plus its lo.lo term, |lo| <= half_ulp_bf16(value)
  through the exponential                 P_qk (es_qk + sum_j P_qj es_qj)  (an error of the row maximum cancels in the normalisation)
  lse                                     sum_j P_qj es_qj + fp32 / logf terms;   delta: C_ATT_B 2^-24 sum |dO out|
  dS = P (dP - delta)                     P (rel_qk |dP - delta| + e(dP) + e(delta)), then dQ, dK, dV as in the T_qk / E_qk structure there.
Each bound is (x3 terms, no constant) + C 2^-24 x (fp32 term) + (the device functions' assumed ulps, applied where they act: expf moves a
probability by 2 FN_ULP 2^-24 relative -- once in the numerator and once in the row sum of the forward, 4 FN_ULP 2^-24 P |v|; once in the
recomputed P of the backward, 2 FN_ULP 2^-24 on P |dO| and on |dS| |K| or |Q|; logf moves lse by FN_ULP 2^-23 |log l| on top of the row sum's
2 FN_ULP 2^-24).

Constants.  C_X3, C_ATT_F, C_ATT_B and DGELU_ABS are measured (measure_*) on float32 restatements against float64 -- the kernels' fp32
operations over 32-wide k-chunks in the kernels' order and in reverse, in units of the fp32 term -- and committed at 8 times the measurement,
the margin _gemm_cases.py gives a restatement (the MFMA's order inside a chunk is not the restatement's).  tests/test_cpu_x3_cases.py
re-measures each and holds the committed value between 4 and 16 times it.  None is set from what a kernel produced: a kernel outside the bound
is a finding.  FN_ULP = 4: no .md, .rst, .txt or .html file of the ROCm installation names expf, logf or erff with an accuracy, so 4 ulp each is AN
ASSUMPTION NOBODY MEASURED.  It enters only as the separate terms named above (16 x 2^-24 of sum P |v| in the forward, 8 x 2^-24 in the
backward, and the function terms of gelu_fn_tol / dgelu_abs), never as part of a measured constant.

How much room the float32 restatement must leave.  Every statement that carries a measured constant is met by the restatement with a ratio
of 1/4 or less (tests/test_cpu_x3_cases.py).  Statement (2) cannot be held to that: E carries no constant and is attained -- at K = 1, or
wherever the residues of a short product share a sign, |al bl + ra b + a rb| IS E, and the largest ratio over the 16129 elements of the
127 x 127 x 64 product is 0.36 -- so a restatement (and a correct kernel) may come arbitrarily close to 1 there.  The restatement is held to
1/4 on (1) and to 1 on (2).  The attention bounds mix both kinds of term and the test cannot see the intermediate values that would separate
them, so there the 'f32' restatement (the kernels' fp32 operations without the split) is held to 1/4 of the fp32 terms alone, and the x3
restatement to 1.5 times ATT_X3_RESTATED, the largest share of the whole bound it takes over the cases (forward, backward: mostly the
exact residue terms); the CPU test re-measures that share and fails when it has moved by a tenth, so a bound that drifts is noticed.  TINY is the absolute floor for results the
hardware may flush below 2^-126."""
import functools
import math

import numpy as np
import torch

import _enc_cases as EC
from _attn_cases import half_ulp_bf16
from semireward_amd import ops

F = np.float32
U24 = 2.0 ** -24
# measured by measure_c_x3() / measure_attn_constants() / measure_dgelu_abs(); tests/test_cpu_x3_cases.py holds each between 4 and 16 times
C_X3_MEASURED, C_ATT_F_MEASURED, C_ATT_B_MEASURED, DGELU_ABS_MEASURED = 5.879, 0.891, 3.656, 1.341e-7
C_X3, C_ATT_F, C_ATT_B, DGELU_ABS = 8.0 * C_X3_MEASURED, 8.0 * C_ATT_F_MEASURED, 8.0 * C_ATT_B_MEASURED, 8.0 * DGELU_ABS_MEASURED
ATT_X3_RESTATED = (0.426, 0.310)    # measure_attn_x3_restated(): largest |x3 restatement - float64| / whole bound, forward and backward
FN_ULP = 4.0                        # assumed (see the docstring): device expf / logf / erff
C_FN_MEASURED = 0.936                # measure_c_fn()
C_FN = 8.0 * C_FN_MEASURED
GELU_L = 1.13
TINY = 1e-32                        # a probability flushed below 2^-126, times 2^9 keys, times |dP - delta| |operand| <= 2^9: 3e-33
FRONT, ROWS_AFTER = 4, 2            # floats before the block (16 bytes), rows after the last
PATTERN32 = 0x4B1D4B1D              # 1.03e7 as fp32
RPS = 37                            # rows_per_sample of the row_scale forms: sample boundaries inside every 16-row fragment
SCALES = (1.5, 0.0, 1.0)
SC, HD = 0.125, 64


EXP_REL = 2.0 * FN_ULP * U24          # relative error of one device expf


# ---- number formats ------------------------------------------------------------------------------------------------------------------------
def bf(x):
    """bf16 round-to-nearest-even of a float32 array, as float32"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F)).to(torch.bfloat16).float().numpy()


def split(x):
    x = np.ascontiguousarray(x, dtype=F)
    hi = bf(x)
    with np.errstate(invalid="ignore"):                  # (inf - inf of a planted overflow)
        return hi, bf((x - hi).astype(F))


def parts(x):
    """(x, hi, lo, r = x - hi - lo) of float32 values, as float64"""
    hi, lo = split(x)
    x8 = np.asarray(x, dtype=F).astype(np.float64)
    return x8, hi.astype(np.float64), lo.astype(np.float64), x8 - hi.astype(np.float64) - lo.astype(np.float64)


def planes(x, mode):
    """the two operand planes of float32 x: 'x3' (hi, lo), 'f32' (x, 0: the fp32 operations alone), 'bf16' (hi, 0: the lo planes zeroed)"""
    x = np.ascontiguousarray(x, dtype=F)
    if mode == "x3":
        return split(x)
    return (x if mode == "f32" else bf(x)), np.zeros_like(x)


def x3_acc(ah, al, bh, bl, reverse=False):
    """sum over 32-wide k-chunks of ah.bl + al.bh + ah.bh (mfma_x3's order; reverse: last chunk first, terms in the other order) in float32:
    [rows of a, rows of b]"""
    acc = np.zeros((ah.shape[0], bh.shape[0]), dtype=F)
    ks = list(range(0, ah.shape[1], 32))
    for k in (ks[::-1] if reverse else ks):
        s = slice(k, k + 32)
        terms = [ah[:, s] @ bl[:, s].T, al[:, s] @ bh[:, s].T, ah[:, s] @ bh[:, s].T]
        for t in (terms[::-1] if reverse else terms):
            acc = (acc + t).astype(F)
    return acc


def _erf(x):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def gelu64(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + _erf(x / math.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu32(v):
    """csrc gelu_erf in float32"""
    v = v.astype(F)
    return (F(0.5) * v * (F(1.0) + _erf((v * F(0.70710678118654752440)).astype(F)))).astype(F)


def gelu_tanh32(v):
    v = v.astype(F)
    return (F(0.5) * v * (F(1.0) + np.tanh(F(0.7978845608) * (v + F(0.044715) * v * v * v)))).astype(F)


def dgelu32(v):
    """csrc dgelu_erf in float32"""
    v = v.astype(F)
    return (F(0.5) * (F(1.0) + _erf((v * F(0.70710678118654752440)).astype(F))) + v * F(0.39894228040143267794) * np.exp(F(-0.5) * v * v)).astype(F)


def gelu_fn_tol(v):
    """error of 0.5 v (1 + erff(v / sqrt 2)) evaluated in fp32 on the exact fp32 argument v (float64 array)"""
    t = v / math.sqrt(2.0)
    e = _erf(t)
    d = 2.0 / math.sqrt(math.pi) * np.exp(-t * t)
    return C_FN * U24 * (np.abs(0.5 * v) * (1.0 + np.abs(e) + np.abs(t) * d) + np.abs(gelu64(v))) + np.abs(0.5 * v) * FN_ULP * 2.0 * U24 * np.abs(e) + TINY


def measure_c_fn():
    """largest |float32 gelu_erf - float64 GELU| in units of 2^-24 x the first-order terms, over the grid of measure_dgelu_abs"""
    x = _grid()
    v = x.astype(np.float64)
    t = v / math.sqrt(2.0)
    base = np.abs(0.5 * v) * (1.0 + np.abs(_erf(t)) + np.abs(t) * 2.0 / math.sqrt(math.pi) * np.exp(-t * t)) + np.abs(gelu64(v))
    nz = base > 0
    return float((np.maximum(np.abs(gelu32(x).astype(np.float64) - gelu64(v))[nz] - TINY, 0.0) / (U24 * base[nz])).max())


def dgelu_abs(x):
    """absolute error of the device GELU' at pre-activation x"""
    return DGELU_ABS + FN_ULP * 2.0 * U24 * (0.5 * np.abs(_erf(x / math.sqrt(2.0))) + np.abs(x) * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi))


def _grid():
    return np.concatenate([np.arange(-10.0, 10.0, 2.0 ** -12), np.linspace(-2.0 ** -4, 2.0 ** -4, 1 << 16)]).astype(F)


def measure_dgelu_abs():
    """largest |float32 dgelu_erf - float64 GELU'| over a grid of fp32 arguments in -10 .. 10 (every 2^-12 and the 2^16 values around 0)"""
    x = _grid()
    return float(np.abs(dgelu32(x).astype(np.float64) - gelu_grad64(x.astype(np.float64))).max())


def _rng(*key):
    return np.random.Generator(np.random.PCG64([int(k) & 0xFFFFFFFF for k in key]))


# ---- arenas ------------------------------------------------------------------------------------------------------------------------------
class Arena:
    """A [rows, width] fp32 block of pitch ld inside a larger allocation.  Operands: block = fill, padding NaN.  Outputs: padding PATTERN32,
    block = fill (an accumulating output) or NaN."""

    def __init__(self, device, rows, width, ld, fill=None, output=False):
        assert ld >= width
        n = FRONT + (rows + ROWS_AFTER) * ld
        if output:
            buf = torch.full((n,), PATTERN32, dtype=torch.int32).view(torch.float32).clone()
        else:
            buf = torch.full((n,), float("nan"), dtype=torch.float32)
        view = torch.as_strided(buf, (rows, width), (ld, 1), FRONT)
        if fill is not None:
            view.copy_(torch.from_numpy(np.ascontiguousarray(fill, dtype=F)).reshape(rows, width))
        else:
            view.fill_(float("nan"))
        self.rows, self.width, self.ld, self.output = rows, width, ld, output
        self.buf = buf.to(device)
        self.view = torch.as_strided(self.buf, (rows, width), (ld, 1), FRONT)
        self.init = self.buf.clone()
        self.ptr = self.buf[FRONT:]                        # contiguous: what the launch is handed
        assert self.ptr.data_ptr() % 16 == 0 and self.ptr.data_ptr() != self.buf.data_ptr()

    def reset(self):
        self.buf.copy_(self.init)

    def put(self, a):
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=F)).reshape(self.rows, self.width))

    def get(self):
        return self.view.cpu().numpy().astype(np.float64)

    def bits(self):
        return self.buf.cpu().view(torch.int32).numpy().copy()

    def pad_touched(self):
        """offsets (from the first valid element) of padding that no longer holds what it held before the launch"""
        now, was = self.buf.clone(), self.init
        torch.as_strided(now, (self.rows, self.width), (self.ld, 1), FRONT).copy_(torch.as_strided(was, (self.rows, self.width), (self.ld, 1), FRONT))
        d = (now.view(torch.int32) != was.view(torch.int32)).nonzero().reshape(-1)[:4].tolist()
        return [i - FRONT for i in d]


def vec(device, a, output=False):
    return Arena(device, 1, len(a), len(a), fill=a, output=output)


# ---- checking ----------------------------------------------------------------------------------------------------------------------------
def within(cid, name, got, want, tol):
    """every element of got within tol of want (NaN is outside); returns max |got - want| / tol, raises naming the worst element"""
    got, want, tol = (np.asarray(x, dtype=np.float64) for x in (got, want, tol))
    assert got.shape == want.shape == tol.shape, (cid, name, got.shape, want.shape, tol.shape)
    err = np.abs(got - want)
    bad = ~(err <= tol)
    if bad.any():
        score = np.where(bad, np.where(np.isfinite(err), err / np.maximum(tol, 1e-300), np.inf), -1.0)
        idx = tuple(int(i) for i in np.unravel_index(int(np.argmax(score)), got.shape))
        frag = " (16-row fragment %d, row %d of it; column tile %d)" % (idx[-2] // 16, idx[-2] % 16, idx[-1] // 128) if got.ndim >= 2 else ""
        raise AssertionError("%s: %s%s got %r want %r |diff| %.3e tol %.3e (%d of %d outside)%s" % (
            cid, name, list(idx), float(got[idx]), float(want[idx]), float(err[idx]), float(tol[idx]), int(bad.sum()), bad.size, frag))
    nz = tol > 0
    return float((err[nz] / tol[nz]).max()) if nz.any() else 0.0


def same_twice(cid, arenas, run):
    """run() twice from the same initial contents: the same bits"""
    run()
    first = [a.bits() for a in arenas]
    for a in arenas:
        a.reset()
    run()
    for a, b in zip(arenas, first):
        assert np.array_equal(a.bits(), b), "%s: two launches of the same operands differ" % cid


# ---- single products: cases ----------------------------------------------------------------------------------------------------------------
def _g(api, epi, M, N, K, *, bias=True, rs=False, ldc_pad=4, spread=False, rps=RPS):
    cid = "%s-%s-%dx%dx%d%s%s%s" % (api, epi, M, N, K, "" if bias else "-nobias", "-rs" if rs else "", "-spread" if spread else "")
    return dict(id=cid, api=api, epi=epi, M=M, N=N, K=K, bias=bias, rs=rs, rps=rps, ldc_pad=ldc_pad, spread=spread, seed=M * 7 + N * 3 + K)


NT_SHAPES = ((1, 1, 32), (127, 127, 64), (128, 128, 96), (129, 132, 32), (300, 132, 64), (129, 1, 96), (1, 128, 64), (300, 127, 96), (129, 132, 3072))
PRE_SHAPES = ((1, 1, 32), (127, 127, 64), (128, 128, 96), (129, 132, 96), (300, 128, 64), (129, 1, 32), (129, 132, 3072))
NN_SHAPES = ((1, 4, 32), (129, 124, 96), (300, 128, 32), (129, 132, 1536), (300, 132, 96))
GEMM_CASES = tuple(
    [_g("nt3", e, *s, **kw) for s in NT_SHAPES for e, kw in (("f32", {}), ("f32", dict(bias=False, ldc_pad=3)), ("gelu", {}), ("resid", {}),
                                                              ("resid", dict(rs=True)), ("resid", dict(rs=True, bias=False, ldc_pad=3)))]
    + [_g("nt3", e, 129, 132, 96, spread=True, **kw) for e, kw in (("f32", {}), ("resid", dict(rs=True)))]
    + [_g("nt", "gelu_pre", *s, bias=b) for s in PRE_SHAPES for b in (True, False)]
    + [_g("nn", e, *s, bias=False) for s in NN_SHAPES for e in ("f32", "acc", "dgelu")])
GEMM_BY_ID = {c["id"]: c for c in GEMM_CASES}
assert len(GEMM_BY_ID) == len(GEMM_CASES)
KERNEL = {"nt3": "gemm_x3_kernel<NT>", "nt": "gemm_x3_kernel<NT>", "nn": "gemm_x3_kernel<NN>"}


@functools.lru_cache(maxsize=4)
def operands(M, N, K, seed, spread):
    """a [M, K], b [N, K] float32 (C = a b^T): column 3 of a and row 5 of b shifted; spread: every element times 2^e, e in -20 .. 20"""
    rng = _rng(seed, M, N, K, 1)
    a = rng.standard_normal((M, K)).astype(F)
    b = (0.1 * rng.standard_normal((N, K))).astype(F)
    a[:, 3] += F(1.0)
    b[min(5, N - 1)] += F(0.25)
    if spread:
        a = np.ldexp(a, rng.integers(-20, 21, size=a.shape)).astype(F)
        b = np.ldexp(b, rng.integers(-20, 21, size=b.shape)).astype(F)
    return a, b


def product_ref(a, b):
    """float64: want3 (what the kernel is specified to compute), S3, true = a b^T, E (what the three-term product leaves out)"""
    a8, ah, al, ra = parts(a)
    b8, bh, bl, rb = parts(b)
    ab = np.abs
    return dict(want3=ah @ bh.T + ah @ bl.T + al @ bh.T, S3=ab(ah) @ ab(bh).T + ab(ah) @ ab(bl).T + ab(al) @ ab(bh).T, true=a8 @ b8.T,
                E=ab(al) @ ab(bl).T + ab(ra) @ ab(b8).T + ab(a8) @ ab(rb).T)


@functools.lru_cache(maxsize=4)
def _case_product(M, N, K, seed, spread):
    return product_ref(*operands(M, N, K, seed, spread))


def case_extras(c):
    """bias [N], C0 [M, N] (no -0), aux [M, N] in -6 .. 6 with zeros, row scales [ceil(M / rows_per_sample)]"""
    M, N = c["M"], c["N"]
    rng = _rng(c["seed"], M, N, 2)
    bias = rng.standard_normal(N).astype(F)
    c0 = (1.5 * rng.standard_normal((M, N)) + 0.2).astype(F)
    aux = rng.uniform(-6.0, 6.0, (M, N)).astype(F)
    aux[::3, ::5] = F(0.0)
    ns = (M + c["rps"] - 1) // c["rps"]
    sc = np.array([SCALES[i % 3] for i in range(ns)], dtype=F)
    if c["spread"]:
        c0 = (c0 * F(2.0 ** 10)).astype(F)
    return bias, c0, aux, sc


class GemmLaunch:
    """Everything one single-product launch reads and writes, on ``device`` ('cpu': the float32 restatement writes the outputs)."""

    def __init__(self, c, device):
        self.c, self.device = c, device
        M, N, K = c["M"], c["N"], c["K"]
        self.a, self.b = operands(M, N, K, c["seed"], c["spread"])
        bias, c0, aux, sc = case_extras(c)
        self.bias = bias if c["bias"] else None
        self.c0 = c0 if c["epi"] in ("resid", "acc") else None
        self.aux = aux if c["epi"] == "dgelu" else None
        self.sc = sc if c["rs"] else None
        self.lda, self.ldc = K + 4, N + c["ldc_pad"]
        self.A = Arena(device, M, K, self.lda, self.a)
        if c["api"] == "nn":
            self.ldb = N + 4
            self.B = Arena(device, K, N, self.ldb, self.b.T)
        else:
            self.ldb = K + 8
            self.B = Arena(device, N, K, self.ldb, self.b)
        self.C = Arena(device, M, N, self.ldc, self.c0, output=True)
        self.outs = [self.C]
        self.Bias = vec(device, self.bias) if self.bias is not None else None
        self.Sc = vec(device, self.sc) if self.sc is not None else None
        self.Aux = self.AuxOut = None
        if self.aux is not None:
            self.ldaux = N + 8
            self.Aux = Arena(device, M, N, self.ldaux, self.aux)
        if c["epi"] == "gelu_pre":
            self.ldaux = N + 4
            self.AuxOut = Arena(device, M, N, self.ldaux, None, output=True)
            self.outs.append(self.AuxOut)

    def row_scales(self):
        return None if self.sc is None else np.repeat(self.sc, self.c["rps"])[:self.c["M"]]

    def run_hip(self):
        c, p = self.c, (lambda x: None if x is None else x.ptr)
        M, N, K = c["M"], c["N"], c["K"]
        if c["api"] == "nt3":
            epi = {"f32": ops.X3_EPI_F32, "gelu": ops.X3_EPI_GELU_F32, "resid": ops.X3_EPI_RESID_F32}[c["epi"]]
            ops.gemm_nt_x3(epi, self.A.ptr, self.B.ptr, self.C.ptr, M, N, K, lda=self.lda, ldw=self.ldb, ldc=self.ldc, bias=p(self.Bias),
                           row_scale=p(self.Sc), rows_per_sample=c["rps"] if self.sc is not None else 0)
        elif c["api"] == "nt":
            ops.gemm_x3(ops.X3B_NT, ops.X3B_EPI_GELU_PRE, self.A.ptr, self.B.ptr, self.C.ptr, M, N, K, lda=self.lda, ldb=self.ldb, ldc=self.ldc,
                        bias=p(self.Bias), aux_out=self.AuxOut.ptr, ldaux=self.ldaux)
        else:
            epi = {"f32": ops.X3B_EPI_F32, "acc": ops.X3B_EPI_ACC, "dgelu": ops.X3B_EPI_DGELU}[c["epi"]]
            ops.gemm_x3(ops.X3B_NN, epi, self.A.ptr, self.B.ptr, self.C.ptr, M, N, K, lda=self.lda, ldb=self.ldb, ldc=self.ldc, aux=p(self.Aux),
                        ldaux=self.ldaux if self.Aux is not None else 0)
        torch.cuda.synchronize()

    # -- the float32 restatement, with the planted faults of tests/test_cpu_x3_cases.py --
    def restate(self, mode="x3", reverse=False, fault=None):
        c = self.c
        M, N, K = c["M"], c["N"], c["K"]
        ah, al = planes(self.a, mode)
        bh, bl = planes(self.b, mode)
        if fault == "al_zero_one_kstep":                   # one 32-wide k-step of the last 16-row fragment
            r0, k0 = (M - 1) // 16 * 16, K - 32
            al = al.copy()
            al[r0:r0 + 16, k0:k0 + 32] = 0.0
        if fault == "split2_second_lo":                    # lo of the second element of a pair against the first element's hi
            r = M // 2
            al = al.copy()
            al[r, 5] = bf(np.array([self.a[r, 5] - ah[r, 4]], dtype=F))[0]
        acc = x3_acc(ah, al, bh, bl, reverse)
        if fault == "last_row_from_M-2":
            acc[M - 1] = acc[M - 2]
        bias = np.zeros(N, dtype=F) if self.bias is None else self.bias
        bn = np.broadcast_to(bias, (M, N)).copy()
        if fault == "bias_dropped_last_col":
            bn[:, N - 1] = 0.0
        v = (acc + bn).astype(F)
        e = c["epi"]
        if e == "f32":
            out = v
        elif e == "gelu":
            out = gelu32(v)
            if fault == "tanh_gelu_one_row":
                out[M // 2] = gelu_tanh32(v[M // 2])
        elif e == "resid":
            s = self.row_scales()
            if s is None:
                s = np.ones(M, dtype=F)
            if fault == "row_scale_index_off":             # the first row of every sample takes the previous sample's scale
                s = s.copy()
                first = np.arange(c["rps"], M, c["rps"])
                s[first] = s[first - 1]
            if fault == "resid_bias_unscaled":
                out = ((self.c0 + (s[:, None] * acc).astype(F)).astype(F) + bn).astype(F)
            else:
                out = (self.c0 + (s[:, None] * v).astype(F)).astype(F)
            if fault == "scale0_changed_resid":            # a dropped row whose residual came back one ulp off
                r = int(np.nonzero(s == 0)[0][0])
                out[r] = np.nextafter(self.c0[r], F(np.inf))
        elif e == "acc":
            out = (self.c0 + v).astype(F)
        elif e == "dgelu":
            aux = self.aux
            if fault == "aux_dense_pitch":                 # aux read at pitch N where it has pitch ldaux
                flat = self.Aux.buf.cpu().numpy()[FRONT:]
                aux = flat[(np.arange(M)[:, None] * N + np.arange(N)[None, :])]
            with np.errstate(invalid="ignore"):
                out = (v * dgelu32(aux)).astype(F)
        else:
            self.AuxOut.put(v)
            out = gelu32(v)
        self.C.put(out)

    def expect(self):
        """[(name, arena, want, tol)] in float64, and the exact statements [(arena, row mask, values)]"""
        c = self.c
        R = _case_product(c["M"], c["N"], c["K"], c["seed"], c["spread"])
        b8 = 0.0 if self.bias is None else self.bias.astype(np.float64)
        w3, wt, S, E = R["want3"] + b8, R["true"] + b8, R["S3"] + np.abs(b8), R["E"]
        t1 = C_X3 * U24 * S
        e, ent, exact = c["epi"], [], []
        if e == "f32":
            ent = [("C:spec", self.C, w3, t1), ("C:true", self.C, wt, t1 + E)]
        elif e == "gelu":
            ent = [("C:spec", self.C, gelu64(w3), GELU_L * t1 + gelu_fn_tol(w3)), ("C:true", self.C, gelu64(wt), GELU_L * (t1 + E) + gelu_fn_tol(wt))]
        elif e in ("resid", "acc"):
            c0 = self.c0.astype(np.float64)
            s = self.row_scales()
            s = np.ones((c["M"], 1)) if s is None else s.astype(np.float64)[:, None]
            own = C_X3 * U24 * np.abs(c0) if e == "acc" else 0.0      # RESID makes one add, c0 + s v: its rounding is the 2^-23 |want|
            for name, w, extra in (("C:spec", w3, 0.0), ("C:true", wt, E)):
                want = c0 + s * w
                ent.append((name, self.C, want, np.abs(s) * (t1 + extra) + own + 2.0 * U24 * np.abs(want)))
            if self.sc is not None:
                exact.append((self.C, s[:, 0] == 0, c0))
        elif e == "dgelu":
            x = self.aux.astype(np.float64)
            d, da = gelu_grad64(x), dgelu_abs(x)
            for name, w, extra in (("C:spec", w3, 0.0), ("C:true", wt, E)):
                want = w * d
                ent.append((name, self.C, want, np.abs(d) * (t1 + extra) + da * (np.abs(w) + t1 + extra) + 2.0 * U24 * np.abs(want) + TINY))
        else:
            ent = [("aux_out:spec", self.AuxOut, w3, t1), ("aux_out:true", self.AuxOut, wt, t1 + E)]
            with np.errstate(invalid="ignore"):
                pre = self.AuxOut.get()
                ent.append(("C:gelu(aux_out)", self.C, gelu64(pre), gelu_fn_tol(pre)))
        return ent, exact

    def verify(self):
        cid = self.c["id"]
        ent, exact = self.expect()
        self.ratios = {name: within(cid, name, ar.get(), want, tol) for name, ar, want, tol in ent}
        ratio = max(self.ratios.values())
        for ar, rows, vals in exact:
            got = ar.get()
            assert np.array_equal(got[rows], vals[rows]), "%s: a row of scale 0 must equal the residual" % cid
        for ar in self.outs:
            t = ar.pad_touched()
            assert not t, "%s: output padding overwritten at offsets %s" % (cid, t)
        return ratio


def measure_c_x3():
    """largest |float32 restatement - want3| / (2^-24 S3) over every product of GEMM_CASES and TN_LAUNCHES, either chunk order"""
    worst, seen = 0.0, set()
    prods = [operands(c["M"], c["N"], c["K"], c["seed"], c["spread"]) + ((c["M"], c["N"], c["K"], c["spread"]),) for c in GEMM_CASES]
    for ln in TN_LAUNCHES:
        for i, pr in enumerate(ln["problems"]):
            a, b, _, _ = tn_inputs(ln, i)
            prods.append((a.T, b.T, (ln["id"], i)))
    for a, b, key in prods:
        if key in seen:
            continue
        seen.add(key)
        R = product_ref(a, b)
        ah, al = split(a)
        bh, bl = split(b)
        for rev in (False, True):
            got = x3_acc(ah, al, bh, bl, rev).astype(np.float64)
            worst = max(worst, float((np.abs(got - R["want3"]) / (U24 * R["S3"])).max()))
    return worst


# ---- the grouped TN weight-gradient launch ------------------------------------------------------------------------------------------------
# (M, N, K tokens, dbias): C[M, N] += A[K, M]^T B[K, N], dbias[M] += colsum A.  pitched: a table built by hand with lda = M + 8, ldb = N + 8,
# ldc = N + 4 -- fields the kernel honours and make_group_tn_desc never sets.
TN_LAUNCHES = (
    dict(id="tn-dense", pitched=False, problems=((8, 8, 1, True), (120, 136, 2, False), (128, 128, 31, True), (136, 264, 33, True), (8, 8, 65, False),
                                                 (136, 264, 272, True))),
    dict(id="tn-pitched", pitched=True, problems=((120, 136, 33, True), (136, 264, 65, False), (8, 8, 272, True), (128, 128, 2, True), (136, 264, 31, True))),
)
TN_BY_ID = {ln["id"]: ln for ln in TN_LAUNCHES}


def tn_inputs(ln, i):
    M, N, K, _ = ln["problems"][i]
    rng = _rng(len(ln["id"]), i, M, N, K)
    A = rng.standard_normal((K, M)).astype(F)
    B = (0.1 * rng.standard_normal((K, N))).astype(F)
    A[:, 3] += F(1.0)
    B[:, min(5, N - 1)] += F(0.25)
    return A, B, (1.5 * rng.standard_normal((M, N)) + 0.2).astype(F), (rng.standard_normal(M) + 0.5).astype(F)


class TnLaunch:
    def __init__(self, ln, device):
        self.ln, self.device, self.P = ln, device, []
        for i, (M, N, K, db) in enumerate(ln["problems"]):
            A, B, c0, d0 = tn_inputs(ln, i)
            pad = ln["pitched"]
            lda, ldb, ldc = M + 8 * pad, N + 8 * pad, N + 4 * pad
            self.P.append(dict(M=M, N=N, K=K, A=A, B=B, c0=c0, d0=d0 if db else None, lda=lda, ldb=ldb, ldc=ldc, aA=Arena(device, K, M, lda, A),
                               aB=Arena(device, K, N, ldb, B), aC=Arena(device, M, N, ldc, c0, output=True),
                               aD=vec(device, d0, output=True) if db else None))
        self.outs = [p["aC"] for p in self.P] + [p["aD"] for p in self.P if p["aD"] is not None]

    def run_hip(self):
        if self.ln["pitched"]:
            arr, t = np.zeros(len(self.P), dtype=ops.GROUP_TN_DESC_DTYPE), 0
            for i, p in enumerate(self.P):
                arr[i] = (p["aA"].ptr.data_ptr(), p["aB"].ptr.data_ptr(), p["aC"].ptr.data_ptr(), p["aD"].ptr.data_ptr() if p["aD"] else 0, p["M"], p["N"],
                          p["K"], p["lda"], p["ldb"], p["ldc"], t, 0)
                t += -(-p["M"] // 128) * -(-p["N"] // 128)
            desc, n = torch.from_numpy(arr.view(np.uint8).copy()).to(self.device), len(self.P)
        else:
            desc, n, t, _, _ = ops.make_group_tn_x3_desc([(p["aA"].ptr, p["aB"].ptr, p["aC"].ptr, p["aD"].ptr if p["aD"] else None, p["M"], p["N"], p["K"])
                                                          for p in self.P], self.device)
        ops.gemm_tn_x3_grouped(desc, n, t)
        torch.cuda.synchronize()

    def restate(self, mode="x3", reverse=False, fault=None):
        for p in self.P:
            A, B, K, M, N = p["A"], p["B"], p["K"], p["M"], p["N"]
            if fault == "tn_last_odd_token_dropped" and K % 2:
                A = A.copy()
                A[K - 1] = 0.0
            ah, al = planes(A.T, mode)
            bh, bl = planes(B.T, mode)
            p["aC"].put((p["c0"] + x3_acc(ah, al, bh, bl, reverse)).astype(F))
            if p["aD"] is not None:
                Kp = -(-K // 32) * 32
                Ap = np.zeros((Kp, M), dtype=F)
                Ap[:K] = p["A"]
                ch = Ap.reshape(Kp // 32, 16, 2, M)
                if fault == "tn_dbias_missing_last_slice":
                    ch = ch[:-1] if len(ch) > 1 else ch * F(0.0)
                cs = np.zeros((16, M), dtype=F)
                for k in (range(len(ch))[::-1] if reverse else range(len(ch))):
                    cs = (cs + (ch[k, :, 0] + ch[k, :, 1]).astype(F)).astype(F)
                s = np.zeros(M, dtype=F)
                for r in (range(16)[::-1] if reverse else range(16)):
                    s = (s + cs[r]).astype(F)
                d = (p["d0"] + s).astype(F)
                if fault == "tn_dbias_every_column_tile":
                    for _ in range(-(-N // 128) - 1):
                        d = (d + s).astype(F)
                p["aD"].put(d)

    def verify(self):
        self.ratios = {"C:spec": 0.0, "C:true": 0.0, "dbias": 0.0}
        for i, p in enumerate(self.P):
            cid = "%s[%d: %dx%dx%d]" % (self.ln["id"], i, p["M"], p["N"], p["K"])
            R = product_ref(p["A"].T, p["B"].T)
            c0 = p["c0"].astype(np.float64)
            t1 = C_X3 * U24 * (R["S3"] + np.abs(c0))
            self.ratios["C:spec"] = max(self.ratios["C:spec"], within(cid, "C:spec", p["aC"].get(), c0 + R["want3"], t1))
            self.ratios["C:true"] = max(self.ratios["C:true"], within(cid, "C:true", p["aC"].get(), c0 + R["true"], t1 + R["E"]))
            if p["aD"] is not None:
                A8, d0 = p["A"].astype(np.float64), p["d0"].astype(np.float64)
                self.ratios["dbias"] = max(self.ratios["dbias"], within(cid, "dbias", p["aD"].get()[0], d0 + A8.sum(0),
                                                                        C_X3 * U24 * (np.abs(A8).sum(0) + np.abs(d0))))
        ratio = max(self.ratios.values())
        for ar in self.outs:
            t = ar.pad_touched()
            assert not t, "%s: output padding overwritten at offsets %s" % (self.ln["id"], t)
        return ratio


# ---- LayerNorm with fp32 output (srhip_layernorm_fwd_f32) ----------------------------------------------------------------------------------
LN_CASES = tuple(dict(id="ln-d%d-m%d-%s" % (D, M, "stats" if (di + mi) % 2 == 0 else "nostats"), D=D, M=M, stats=(di + mi) % 2 == 0, seed=10 * di + mi,
                      eps=1e-6) for di, D in enumerate((128, 384, 512, 768)) for mi, M in enumerate((1, 7, 8, 9, 17)))
LN_BY_ID = {c["id"]: c for c in LN_CASES}


class LnLaunch:
    """rows cycle through unit / mean 300 / spread 1e-3 / constant (tests/_enc_cases.py family_rows); the bound is _enc_cases.ln_fwd_ref's, with
    its conditioning term |mu| rstd and its constants C_LN and RSQRT_ULP"""

    def __init__(self, c, device):
        self.c, self.device = c, device
        M, D = c["M"], c["D"]
        rng = _rng(c["seed"], 0xF3)
        self.y, self.fam = EC.family_rows(rng, M, D, c["seed"])
        self.g, self.b = (1.0 + 0.1 * rng.standard_normal(D)).astype(F), (0.1 * rng.standard_normal(D)).astype(F)
        self.X, self.G, self.Bt = Arena(device, M, D, D, self.y), vec(device, self.g), vec(device, self.b)
        self.O = Arena(device, M, D, D, None, output=True)
        self.Mean, self.Rstd = (Arena(device, 1, M, M, None, output=True), Arena(device, 1, M, M, None, output=True)) if c["stats"] else (None, None)
        self.outs = [a for a in (self.O, self.Mean, self.Rstd) if a is not None]

    def run_hip(self):
        c = self.c
        ops.layernorm_fwd_f32(self.X.ptr, self.G.ptr, self.Bt.ptr, c["eps"], self.O.ptr, self.Mean.ptr if self.Mean else None,
                              self.Rstd.ptr if self.Rstd else None, c["M"], c["D"])
        torch.cuda.synchronize()

    def restate(self, order="tree"):
        o, mu, rs = EC.ln_fwd32(self.y, self.g, self.b, self.c["eps"], order)
        self.O.put(o)
        if self.Mean is not None:
            self.Mean.put(mu)
            self.Rstd.put(rs)

    def verify(self):
        cid = self.c["id"]
        y8 = self.y.astype(np.float64)
        R = EC.ln_fwd_ref(y8, np.zeros_like(y8), np.abs(y8), self.g.astype(np.float64), self.b.astype(np.float64), self.c["eps"])
        got = self.O.get()
        ratio = within(cid, "out", got, R["o"], EC.C_LN * R["base_o"] + R["extra_o"])
        if self.Mean is not None:
            ratio = max(ratio, within(cid, "mean", self.Mean.get()[0], R["mu"], EC.C_LN * R["base_mu"]),
                        within(cid, "rstd", self.Rstd.get()[0], R["rs"], EC.C_LN * R["base_rs"] + R["extra_rs"]))
        const = self.fam == 3
        assert np.array_equal(got[const].astype(F), np.tile(self.b, (int(const.sum()), 1))), "%s: a constant row's output is beta" % cid
        for ar in self.outs:
            t = ar.pad_touched()
            assert not t, "%s: output padding overwritten at offsets %s" % (cid, t)
        return ratio


# ---- attention -----------------------------------------------------------------------------------------------------------------------------
ATTN_NS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257, 512)
ATTN_CASES = tuple(dict(id="attn-N%d" % N, N=N, B=1 if N == 512 else 2, H=1 if N == 512 else 2, seed=9100 + N) for N in ATTN_NS)
ATTN_BY_ID = {c["id"]: c for c in ATTN_CASES}
DECISIVE, SPIKE_A, SPIKE_B = 0.25, 8.0, 28.0
# SPIKE_B: the raw score of the second spiked key is 784 = 98 after the scale, so a row maximum that misses it overflows expf.  (A softmax is
# invariant to the shift it subtracts: with the 12.0 of _attn_cases.py a maximum taken over too few keys would give the right answer.)


def attn_inputs(c):
    """q, k, v, do: float64 arrays [B, H, N, 64] of float32 values, built as tests/_attn_cases.py make_inputs builds them (every key decisive for
    some query; two spiked keys per head, the second in the last 16-key block, its raw score >= 40 above the rest) but NOT rounded to bf16: the
    lo planes carry information.  pi [B, H, N]; spikes [(b, h, qa, s1, qb, s2)]."""
    B, N, H = c["B"], c["N"], c["H"]
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    q, k = 0.5 * rng.standard_normal((B, H, N, HD)), 0.5 * rng.standard_normal((B, H, N, HD))
    v, do = rng.standard_normal((B, H, N, HD)), rng.standard_normal((B, H, N, HD))
    q[..., 62:], k[..., 62:] = 0.0, 0.0
    pi, spikes = np.zeros((B, H, N), dtype=np.int64), []
    x = (math.log(N) + 1.5) / SC
    for b in range(B):
        for h in range(H):
            perm = rng.permutation(N)
            pi[b, h] = perm
            sp = None
            if N >= 4:
                lo = (N - 1) // 16 * 16
                s2 = int(rng.integers(lo, N))
                s1 = int(rng.integers(0, min(N, 128)))
                if s1 == s2:
                    s1 = (s2 + 1) % N if s2 + 1 < N or lo > 0 else s2 - 1
                qa, qb = int(np.nonzero(perm == s1)[0][0]), int(np.nonzero(perm == s2)[0][0])
                k[b, h, s1, 63], k[b, h, s2, 62] = SPIKE_A, SPIKE_B
                sp = (b, h, qa, s1, qb, s2)
            kk = k[b, h, perm]
            q[b, h] += x * kk / (kk * kk).sum(-1, keepdims=True)
            if sp:
                q[b, h, qa, 63] = SPIKE_A
                q[b, h, qb, 63], q[b, h, qb, 62] = SPIKE_A, SPIKE_B
                spikes.append(sp)
    f = lambda t: t.astype(F).astype(np.float64)
    return dict(q=f(q), k=f(k), v=f(v), do=f(do), pi=pi, spikes=spikes)


def _pair_terms(x, y):
    """of the product x y^T of two visible fp32 operands: (E: what x3 leaves out, S3) in float64, unscaled"""
    x8, xh, xl, rx = parts(x)
    y8, yh, yl, ry = parts(y)
    a = np.abs
    return (a(xl) @ a(yl).T + a(rx) @ a(y8).T + a(x8) @ a(ry).T, a(xh) @ a(yh).T + a(xh) @ a(yl).T + a(xl) @ a(yh).T)


def head_fwd(q, k, v):
    a = np.abs
    S = SC * (q @ k.T)
    m = S.max(1)
    Eu = np.exp(S - m[:, None])
    Z = Eu.sum(1)
    P = Eu / Z[:, None]
    lse = m + np.log(Z)
    Es, S3s = _pair_terms(q, k)
    es, tau = SC * Es, SC * S3s + a(S) + a(m)[:, None] + 1.0
    rel_x3, rel_f = es + (P * es).sum(1, keepdims=True), tau + (P * tau).sum(1, keepdims=True) + 1.0
    v8, vh, vl, rv = parts(v)
    A = P @ a(v8)
    hu = half_ulp_bf16(Eu) / Z[:, None]
    out_x3 = (P * rel_x3) @ a(v8) + 2.0 ** -16 * A + P @ a(rv) + hu @ a(vl)
    out_f = (P * rel_f) @ a(v8)
    lse_x3, lse_f = (P * es).sum(1), (P * tau).sum(1) + a(lse) + 1.0
    out_fn, lse_fn = 2.0 * EXP_REL * A, EXP_REL + FN_ULP * 2.0 * U24 * np.log(Z)
    return dict(P=P, S=S, out=P @ v8, out_f32=out_f, out_fn=out_fn, out_tol=out_x3 + C_ATT_F * U24 * out_f + out_fn + TINY * (A > 0), lse=lse,
                lse_f32=lse_f, lse_fn=lse_fn, lse_tol=lse_x3 + C_ATT_F * U24 * lse_f + lse_fn)


def head_bwd(q, k, v, do, out_g, lse_g):
    """the kernels' backward formula in float64 on the given arrays, with the bound of every element"""
    a = np.abs
    S = SC * (q @ k.T)
    P = np.exp(S - lse_g[:, None])
    delta, aD = (do * out_g).sum(1), (a(do) * a(out_g)).sum(1)
    dP = do @ v.T
    Es, S3s = _pair_terms(q, k)
    Ep, S3p = _pair_terms(do, v)
    es, tau = SC * Es, SC * S3s + a(S) + a(lse_g)[:, None] + 1.0
    diff = dP - delta[:, None]
    dS = P * diff
    eds_x3 = P * (es * a(diff) + Ep)
    eds_f = P * (tau * a(diff) + S3p + aD[:, None] + a(dP) + a(delta)[:, None])
    r = dict(delta=delta, delta_f32=aD, delta_tol=C_ATT_B * U24 * aD)
    hS, hP = half_ulp_bf16(dS), half_ulp_bf16(P)
    for name, val, ex3, ef, hv, opnd in (("dq", dS, eds_x3, eds_f, hS, k), ("dk", dS.T, eds_x3.T, eds_f.T, hS.T, q),
                                        ("dv", P.T, (P * es).T, (P * tau).T, hP.T, do)):
        o8, oh, ol, ro = parts(opnd)
        sc = 1.0 if name == "dv" else SC
        r[name] = sc * (val @ o8)
        x3 = sc * (ex3 @ a(o8) + 2.0 ** -16 * (a(val) @ a(o8)) + a(val) @ a(ro) + hv @ a(ol))
        r[name + "_f32"] = sc * (ef @ a(o8) + a(val) @ a(o8))
        r[name + "_fn"] = EXP_REL * sc * (a(val) @ a(o8))
        r[name + "_tol"] = x3 + C_ATT_B * U24 * r[name + "_f32"] + r[name + "_fn"] + TINY * (r[name + "_f32"] > 0)
    return r


FWD_KEYS = ("out", "out_tol", "out_f32", "out_fn", "lse", "lse_tol", "lse_f32", "lse_fn")
BWD_KEYS = ("delta", "delta_tol", "delta_f32") + tuple(n + s for n in ("dq", "dk", "dv") for s in ("", "_tol", "_f32", "_fn"))


def _stack(c, fn, keys):
    res = [[fn(b, h) for h in range(c["H"])] for b in range(c["B"])]
    return {key: np.stack([np.stack([res[b][h][key] for h in range(c["H"])]) for b in range(c["B"])]) for key in keys}


@functools.lru_cache(maxsize=2)
def attn_reference(cid):
    """inputs and both references of a case (read-only); out_given / lse_given: the float64 forward rounded to fp32, what the backward is fed"""
    c = ATTN_BY_ID[cid]
    inp = attn_inputs(c)
    fwd = _stack(c, lambda b, h: head_fwd(inp["q"][b, h], inp["k"][b, h], inp["v"][b, h]), FWD_KEYS)
    fwd["out_given"], fwd["lse_given"] = fwd["out"].astype(F).astype(np.float64), fwd["lse"].astype(F).astype(np.float64)
    bwd = _stack(c, lambda b, h: head_bwd(inp["q"][b, h], inp["k"][b, h], inp["v"][b, h], inp["do"][b, h], fwd["out_given"][b, h],
                                          fwd["lse_given"][b, h]), BWD_KEYS)
    return dict(c=c, inp=inp, fwd=fwd, bwd=bwd)


def decisive_mass(c, inp):
    """smallest probability of the key a row was built to depend on; smallest margin of a spiked raw score over the row's other raw scores"""
    least, margin = 1.0, np.inf
    for b in range(c["B"]):
        for h in range(c["H"]):
            P = head_fwd(inp["q"][b, h], inp["k"][b, h], inp["v"][b, h])["P"]
            least = min(least, float(P[np.arange(c["N"]), inp["pi"][b, h]].min()))
    for b, h, qa, s1, qb, s2 in inp["spikes"]:
        raw = inp["q"][b, h] @ inp["k"][b, h].T
        for qq, s in ((qa, s1), (qb, s2)):
            margin = min(margin, float(raw[qq, s] - np.delete(raw[qq], s).max()))
    return least, margin


def _tol(ref, n, f32_only, c):
    """the bound of output n; f32_only: its fp32 term alone, without the device functions' ulps (what the 'f32' restatement, which makes no
    split and takes the host's exp and log, is held to)"""
    return c * U24 * ref[n + "_f32"] + TINY * (ref[n + "_f32"] > 0) if f32_only else ref[n + "_tol"]


def verify_fwd(cid, out, lse, ref, f32_only=False):
    """out [B, H, N, 64], lse [B, H, N] or None"""
    r = within(cid, "out", out, ref["out"], _tol(ref, "out", f32_only, C_ATT_F))
    return r if lse is None else max(r, within(cid, "lse", lse, ref["lse"], _tol(ref, "lse", f32_only, C_ATT_F)))


def verify_bwd(cid, got, ref, f32_only=False):
    return max([within(cid, n, got[n], ref[n], _tol(ref, n, f32_only, C_ATT_B)) for n in ("dq", "dk", "dv")]
               + [within(cid, "delta_ws", got["delta"], ref["delta"], ref["delta_tol"])])


def _sum32(x, reverse):
    """sum over the last axis in float32, first to last or last to first"""
    x = x[..., ::-1] if reverse else x
    return np.cumsum(x.astype(F), axis=-1, dtype=F)[..., -1]


def restate_fwd(q, k, v, mode="x3", reverse=False, fault=None):
    """one head of attn_fwd_x3_kernel in float32: out [N, 64], lse [N] (float64 arrays of the float32 values)"""
    N = q.shape[0]
    q, k, v = q.astype(F), k.astype(F), v.astype(F)
    s = x3_acc(*planes(k, mode), *planes(q, mode), reverse).T
    sc = (s * F(SC)).astype(F)
    mx = sc.max(1)
    if fault == "max_over_whole_blocks" and N % 16 and N > 16:
        mx = sc[:, :N // 16 * 16].max(1)
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.exp((sc - mx[:, None]).astype(F)).astype(F)
    vv = v
    if fault == "key_N_counted" and N % 32:                # queries of the last 16-row block see the clamped duplicate of key N - 1 as key N
        q0 = (N - 1) // 16 * 16
        extra = np.zeros((N, 1), dtype=F)
        extra[q0:, 0] = p[q0:, N - 1]
        p, vv = np.concatenate([p, extra], 1), np.concatenate([v, v[N - 1:]], 0)
    L = p.shape[1]
    steps = [slice(i, min(i + 32, L)) for i in range(0, L, 32)]
    l = np.zeros(N, dtype=F)
    for t in (steps[::-1] if reverse else steps):
        l = (l + _sum32(p[:, t], reverse)).astype(F)
    ph, pl = planes(p, mode)
    if fault == "p_plain_bf16_one_step":
        t = steps[-1]
        ph, pl = ph.copy(), pl.copy()
        ph[:, t], pl[:, t] = bf(p[:, t]), 0.0
    vh, vl = planes(vv.T, mode)
    with np.errstate(invalid="ignore", over="ignore"):
        o = x3_acc(vh, vl, ph, pl, reverse).T
        out = (o * (F(1.0) / l)[:, None]).astype(F)
        lse = (mx + np.log(l)).astype(F)
    if fault == "lse_without_max":
        lse[N // 2] = np.log(l[N // 2])
    return out.astype(np.float64), lse.astype(np.float64)


def restate_bwd(q, k, v, do, out_g, lse_g, mode="x3", reverse=False, fault=None):
    """one head of both attn_bwd_x3 kernels in float32: dq, dk, dv [N, 64], delta [N]"""
    N = q.shape[0]
    q, k, v, do, og, lg = (t.astype(F) for t in (q, k, v, do, out_g, lse_g))
    s = x3_acc(*planes(k, mode), *planes(q, mode), reverse).T
    dp = x3_acc(*planes(v, mode), *planes(do, mode), reverse).T
    prod = (do * og).astype(F)
    delta = _sum32(prod, reverse)
    if fault == "delta_one_lane_group":                    # one query: the 16 dims of lane group 0 only
        delta[N // 2] = _sum32(prod[N // 2, [d for d in range(64) if (d % 32) // 8 == 0]], reverse)
    p = np.exp(((s * F(SC)).astype(F) - lg[:, None]).astype(F)).astype(F)
    ds = (p * (dp - delta[:, None]).astype(F)).astype(F)
    dq = (x3_acc(*planes(k.T, mode), *planes(ds, mode), reverse).T * F(SC)).astype(F)
    dk = (x3_acc(*planes(q.T, mode), *planes(ds.T, mode), reverse).T * F(SC)).astype(F)
    dv = x3_acc(*planes(do.T, mode), *planes(p.T, mode), reverse).T
    if fault == "dk_unscaled_one_block":
        b0 = (N - 1) // 16 * 16
        dk[b0:b0 + 16] = (dk[b0:b0 + 16] / F(SC)).astype(F)
    return dict(dq=dq.astype(np.float64), dk=dk.astype(np.float64), dv=dv.astype(np.float64), delta=delta.astype(np.float64))


def restate_attn(cid, mode="x3", reverse=False, fault=None):
    """both restatements over every head of a case, shaped like the references"""
    ref = attn_reference(cid)
    c, inp, fwd = ref["c"], ref["inp"], ref["fwd"]
    B, H, N = c["B"], c["H"], c["N"]
    r = {n: np.zeros((B, H, N, HD)) for n in ("out", "dq", "dk", "dv")}
    r.update({n: np.zeros((B, H, N)) for n in ("lse", "delta")})
    for b in range(B):
        for h in range(H):
            a = (inp["q"][b, h], inp["k"][b, h], inp["v"][b, h])
            r["out"][b, h], r["lse"][b, h] = restate_fwd(*a, mode=mode, reverse=reverse, fault=fault)
            g = restate_bwd(*a, inp["do"][b, h], fwd["out_given"][b, h], fwd["lse_given"][b, h], mode=mode, reverse=reverse, fault=fault)
            for n in g:
                r[n][b, h] = g[n]
    return r


def _units(got, want, term):
    nz = term > 0
    return float((np.maximum(np.abs(got - want)[nz] - TINY, 0.0) / (U24 * term[nz])).max()) if nz.any() else 0.0


def measure_attn_constants():
    """largest error of the 'f32' restatements (the fp32 operations without the split) in units of 2^-24 x the fp32 term: (forward, backward)"""
    cf = cb = 0.0
    for c in ATTN_CASES:
        ref = attn_reference(c["id"])
        for rev in (False, True):
            r = restate_attn(c["id"], mode="f32", reverse=rev)
            cf = max(cf, _units(r["out"], ref["fwd"]["out"], ref["fwd"]["out_f32"]), _units(r["lse"], ref["fwd"]["lse"], ref["fwd"]["lse_f32"]))
            cb = max(cb, max(_units(r[n], ref["bwd"][n], ref["bwd"][n + "_f32"]) for n in ("dq", "dk", "dv", "delta")))
    return cf, cb


def measure_attn_x3_restated():
    """largest share of the whole bound the x3 restatement takes, either order: (forward, backward)"""
    rf = rb = 0.0
    for c in ATTN_CASES:
        ref = attn_reference(c["id"])
        for rev in (False, True):
            r = restate_attn(c["id"], reverse=rev)
            rf, rb = max(rf, verify_fwd(c["id"], r["out"], r["lse"], ref["fwd"])), max(rb, verify_bwd(c["id"], r, ref["bwd"]))
    return rf, rb


# -- launches (GPU tests only) --
def _pack(x):
    B, H, N, _ = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(B * N, H * HD)


def _unpack(x, B, N, H):
    return x.reshape(B, N, H, HD).transpose(0, 2, 1, 3)


class AttnLaunch:
    def __init__(self, cid, device):
        ref = attn_reference(cid)
        c, inp, fwd = ref["c"], ref["inp"], ref["fwd"]
        self.c, self.ref = c, ref
        B, N, H = c["B"], c["N"], c["H"]
        D = H * HD
        self.qkv = Arena(device, B * N, 3 * D, 3 * D, np.concatenate([_pack(inp["q"]), _pack(inp["k"]), _pack(inp["v"])], 1))
        self.o_in = Arena(device, B * N, D, D, _pack(fwd["out_given"]))
        self.do = Arena(device, B * N, D, D, _pack(inp["do"]))
        self.lse_in = Arena(device, B * H, N, N, fwd["lse_given"].reshape(B * H, N))
        self.out, self.out2 = Arena(device, B * N, D, D, None, output=True), Arena(device, B * N, D, D, None, output=True)
        self.lse = Arena(device, B * H, N, N, None, output=True)
        self.dqkv = Arena(device, B * N, 3 * D, 3 * D, None, output=True)
        self.delta = Arena(device, B * H, N, N, None, output=True)

    def run_fwd(self):
        c = self.c
        ops.attn_fwd_x3(self.qkv.ptr, self.out.ptr, c["B"], c["N"], c["H"], SC)
        ops.attn_fwd_x3_lse(self.qkv.ptr, self.out2.ptr, self.lse.ptr, c["B"], c["N"], c["H"], SC)
        torch.cuda.synchronize()

    def run_bwd(self):
        c = self.c
        ops.attn_bwd_x3(self.qkv.ptr, self.o_in.ptr, self.do.ptr, self.lse_in.ptr, self.dqkv.ptr, self.delta.ptr, c["B"], c["N"], c["H"], SC)
        torch.cuda.synchronize()

    def got_fwd(self):
        c = self.c
        return _unpack(self.out.get(), c["B"], c["N"], c["H"]), self.lse.get().reshape(c["B"], c["H"], c["N"])

    def got_bwd(self):
        c = self.c
        D, x = c["H"] * HD, self.dqkv.get()
        g = {n: _unpack(x[:, i * D:(i + 1) * D], c["B"], c["N"], c["H"]) for i, n in enumerate(("dq", "dk", "dv"))}
        g["delta"] = self.delta.get().reshape(c["B"], c["H"], c["N"])
        return g


# ---- the planted faults (tests/test_cpu_x3_cases.py) and what the whole-tensor norms make of them -------------------------------------------
# name -> (family, case id the fault is planted in)
FAULTS = {
    "al_zero_one_kstep": ("gemm", "nt3-f32-128x128x96"),
    "split2_second_lo": ("gemm", "nt3-f32-300x132x64"),
    "last_row_from_M-2": ("gemm", "nt3-f32-129x132x32"),
    "bias_dropped_last_col": ("gemm", "nt3-f32-300x132x64"),
    "tanh_gelu_one_row": ("gemm", "nt3-gelu-300x132x64"),
    "resid_bias_unscaled": ("gemm", "nt3-resid-300x132x64-rs"),
    "row_scale_index_off": ("gemm", "nt3-resid-300x132x64-rs"),
    "scale0_changed_resid": ("gemm", "nt3-resid-300x132x64-rs"),
    "tn_last_odd_token_dropped": ("tn", "tn-dense"),
    "tn_dbias_every_column_tile": ("tn", "tn-dense"),
    "tn_dbias_missing_last_slice": ("tn", "tn-dense"),
    "aux_dense_pitch": ("gemm", "nn-dgelu-129x124x96-nobias"),
    "key_N_counted": ("attn", "attn-N33"),
    "max_over_whole_blocks": ("attn", "attn-N33"),
    "lse_without_max": ("attn", "attn-N33"),
    "delta_one_lane_group": ("attn", "attn-N33"),
    "dk_unscaled_one_block": ("attn", "attn-N257"),
    "p_plain_bf16_one_step": ("attn", "attn-N257"),
}
# the faults whose whole-tensor rel-L2 stays under the thresholds of test_gpu_read_rows_precision.py / test_gpu_grad_rows_precision.py at those
# tests' own shapes and Gaussian inputs (tests/test_cpu_x3_cases.py::test_what_the_norm_thresholds_let_pass computes every figure)
NORM_BLIND = ("tanh_gelu_one_row", "aux_dense_pitch", "max_over_whole_blocks")
