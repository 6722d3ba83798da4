"""The cases of tests/test_{cpu,gpu}_gemm_cases.py: every tile kernel of csrc/gemm.hip (64 x 64 'small64', 128 x 128 'tile128' with and without
split-K, the two-wave-group 256 x 256 x 64 'pp256', the lockstep 256-row 'big256'), every epilogue form it accepts and every edge at which it
branches, element by element against float64.  Nothing is stored: every input is rebuilt from its seed, every expected value is recomputed.

Why element by element: a whole-tensor rel-L2 moves by 1 / sqrt(M) when one output row is wrong -- 3.8e-3 at M = 70001, beside the 4e-3 .. 5e-3
the dense tests allowed -- so a bias dropped on one row (2.4e-3) or a k-tile missing from one fragment (1.7e-3) passed at every shape, and a
ragged last row stored as zeros read 4.09e-3 on the bf16 output (in quadrature with 1.7e-3 of bf16 rounding: caught by 2 % of the bound, at
that M and no larger) and passed the 5e-3 of the GELU output.  tests/test_cpu_gemm_cases.py states these figures and shows verify() below
rejecting all three.

Inputs.  bf16 operands from a PCG64 stream; column 3 of A and row 5 of B are shifted (a transposed or permuted fragment shows).  bias, residual,
row_scale, pre-activations and LayerNorm statistics are seeded likewise.  Every operand and output lives inside a larger allocation at a
16-byte-aligned non-zero offset (FRONT elements) with a real pitch.  Operand padding (columns K .. lda, ROWS_AFTER rows past the last, the
front) is NaN: a kernel that reads a row or a k-tile too far poisons its result.  Output padding (columns N .. ldc, ROWS_AFTER rows after M, the
front) holds the bit pattern PATTERN and must come back bit for bit; where the epilogue overwrites (everything but the in-place residual and
beta != 0) the [M, N] block itself starts as NaN, so that 0 * C or a skipped store shows.

Bound of an element (never a norm).  S = |A| |B|^T + |bias| in float64, tol32 = C_ACC 2^-24 S:
  fp32 outputs    |got - want| <= tol32' + 2^-23 |want|, tol32' = C_ACC 2^-24 (|rs| s S + |resid|)  (rs: row scale, s = 1 / (1 - p): both multiply
                  the product and its error; 1 without them);  alpha / beta likewise: |alpha| S + |beta| |C0|
  LayerNorm owed  ... + 2^-22 (|xhat gamma| + |beta|) for the four fp32 operations of the normalisation
  bf16 outputs    |got - want| <= L tol32 + E + half_ulp_bf16(|want| + L tol32), half_ulp_bf16 exact (8 significant bits)
                  BF16 and the saved pre-activation: L = 1, E = 0;  GELU: L = 1.13 (max |GELU'|), E = 1e-6 (what test_gelu_forms_against_exact_erf
                  holds gelu_erf to);  DGELU: L = |GELU'(p)|, E = DGELU_ABS |v|, v = the float64 product the derivative multiplies (the
                  formula's error is absolute in GELU', which crosses 0: relative to v GELU'(p) it would be unbounded);  with dropout L and E
                  are multiplied by s
  exact           elements the mask drops are zero in bf16 outputs (-0 where a dropped DGELU element meets a negative GELU'); dropped elements and rows whose row_scale is 0 equal the residual bit for bit in
                  RESID_F32 without LayerNorm; all output padding equals what was there before the launch
C_ACC and DGELU_ABS are measured on float32 restatements against the float64 reference (measure_c_acc, measure_dgelu_abs: the accumulation over
32-wide k-chunks in the kernels' order and in reverse; the derivative formula of csrc/common.h over every finite bf16 pre-activation), times 8
-- the margin the rewarder tests give a float32 restatement; the MFMA's order inside a chunk is not the restatement's.  They are never set from
what a kernel produced: a kernel outside the bound is a finding.  tests/test_cpu_gemm_cases.py measures both afresh.

Shapes are the smallest that reach each kernel under gemm_plan's rules at GEMM_SMALL_ALONE (a 256-row kernel needs three rounds of 256 tiles
below K = 768: 39173 x 1152, 48901 x 1024), M odd and ragged against every tile height; see CASES for what each one varies."""
import functools
import math

import numpy as np
import torch

from oracle import bert_ref as BR
from semireward_amd import ops

# measured by measure_c_acc() / measure_dgelu_abs() (tests/test_cpu_gemm_cases.py holds each constant between 4 and 16 times its measurement):
#   largest |float32 restatement - float64| / (2^-24 S) over every product of CASES, either chunk order: C_ACC_MEASURED
#   largest |float32 gelu_erf_grad - float64 GELU'| over every finite bf16 argument:                      DGELU_ABS_MEASURED
C_ACC_MEASURED, DGELU_ABS_MEASURED = 2.887, 2.676e-7
C_ACC, DGELU_ABS = 8.0 * C_ACC_MEASURED, 8.0 * DGELU_ABS_MEASURED
GELU_L, GELU_E = 1.13, 1e-6
# what test_gelu_forms_against_exact_erf holds gelu_poly2 (the GELU inside srhip_mlp_fused_proj) to: |gelu_poly2(x) - GELU(x)| <= max(ABS, REL |x|)
GELU_POLY2_ABS, GELU_POLY2_REL = 7e-5, 5e-6

FRONT, ROWS_AFTER = 64, 64          # elements before the first, rows after the last (operands and outputs)
PATTERN = 0x4B1D                    # every 16 bits of the output padding: 9.96e6 as bf16, 1.03e7 as fp32 (0x4B1D4B1D), finite in both
RPS = 257                           # rows_per_sample of the row_scale forms: sample boundaries inside every tile height
DROP_P, DROP_SITE, DROP_SEED = 0.1, 5, (41 << 32) + 7
TILE = {"small64": 64, "tile128": 128, "pp256": 256, "big256": 256, "big128": 256, "big2wg": 256}
BF16_EPIS = (ops.EPI_BF16, ops.EPI_GELU_BF16, ops.EPI_DGELU_BF16)


# ---- epilogue forms ----------------------------------------------------------------------------------------------------------------------
def _form(name, epi, **kw):
    f = dict(name=name, epi=epi, api="nt", bias=True, resid=None, row_scale=False, drop=False, ln=False, aux_out=False, aux_pad=0,
             alpha=1.0, beta=0.0, op_pad=0, c_pad=0, overlap=0)
    f.update(kw)
    return f


_F = {f["name"]: f for f in (
    _form("bf16", ops.EPI_BF16),
    _form("gelu", ops.EPI_GELU_BF16),
    _form("gelu_aux", ops.EPI_GELU_BF16, aux_out=True),
    _form("gelu_aux_ld2", ops.EPI_GELU_BF16, aux_out=True, aux_pad=2),                     # ldaux % 4 != 0: the narrow store path
    _form("dgelu", ops.EPI_DGELU_BF16, bias=False),
    _form("gelu_drop", ops.EPI_GELU_BF16, api="dropout", aux_out=True, drop=True),         # srhip_gemm_nt_dropout: the MLP forward ...
    _form("dgelu_drop", ops.EPI_DGELU_BF16, api="dropout", bias=False, drop=True),         # ... and backward of BERT / Wav2Vec2
    _form("resid_inplace", ops.EPI_RESID_F32, resid="inplace"),
    _form("resid_aux", ops.EPI_RESID_F32, resid="aux"),
    _form("resid_rowscale", ops.EPI_RESID_F32, resid="inplace", row_scale=True),
    _form("resid_drop", ops.EPI_RESID_F32, api="resid_dropout", resid="aux", drop=True),
    _form("resid_ln", ops.EPI_RESID_F32, api="resid_ln", resid="inplace", ln=True),
    _form("resid_ln_drop", ops.EPI_RESID_F32, api="resid_ln", resid="inplace", ln=True, drop=True),
    _form("f32_a1_b0", ops.EPI_F32, bias=False),
    _form("f32_a.5_b1", ops.EPI_F32, bias=False, alpha=0.5, beta=1.0),
    _form("f32_a-1_b1", ops.EPI_F32, bias=False, alpha=-1.0, beta=1.0),
    _form("pitch8_bf16", ops.EPI_BF16, op_pad=8, c_pad=8),                                 # lda, ldb = K + 8; ldc = N + 8 keeps the wide path
    _form("pitch4_bf16", ops.EPI_BF16, op_pad=8, c_pad=4),                                 # ldc = N + 4 forces the narrow one
    _form("pitch_gelu_aux", ops.EPI_GELU_BF16, aux_out=True, op_pad=8, c_pad=8, aux_pad=4),
    _form("pitch_resid_aux", ops.EPI_RESID_F32, resid="aux", op_pad=8, c_pad=4, aux_pad=8),
    _form("overlap_bf16", ops.EPI_BF16, overlap=16),                                       # lda = 16 < K: the convolutions' sliding rows
)}
_BF16 = ("bf16", "gelu", "gelu_aux", "gelu_aux_ld2", "dgelu", "gelu_drop", "dgelu_drop")
_RESID = ("resid_inplace", "resid_aux", "resid_rowscale", "resid_drop")
_LN = ("resid_ln", "resid_ln_drop")
_PITCH = ("pitch8_bf16", "pitch4_bf16", "pitch_gelu_aux", "pitch_resid_aux")
_F32 = ("f32_a1_b0", "f32_a.5_b1", "f32_a-1_b1")
FULL = _BF16 + _RESID + _PITCH                  # what every kernel's cases include once (plus _LN, overlap_bf16, _F32 where the kernel has them)
SHORT = ("bf16", "resid_inplace")               # the other K of a wide shape
NARROW = ("bf16", "gelu_aux", "dgelu", "resid_inplace")


def _case(plan, M, N, K, forms, seed=0, dseed=DROP_SEED):
    return dict(plan=plan, M=M, N=N, K=K, forms=tuple(forms), seed=seed, dseed=dseed, id="%s-%dx%dx%d" % (plan, M, N, K))


CASES = (
    # 64 x 64 tiles, 5-deep ring of 32-wide k-tiles: one row; tile - 1 / tile / tile + 1; K = 1, 3, 5, 6 k-tiles; narrow (N = 4, 60, 132) and
    # wide (N = 384) stores; three row_scale samples at M = 771
    _case("small64", 1, 4, 32, SHORT + ("gelu_aux", "dgelu")),
    _case("small64", 63, 60, 96, SHORT + ("gelu_aux_ld2",)),
    _case("small64", 64, 64, 160, SHORT + ("dgelu", "resid_ln")),
    _case("small64", 65, 132, 192, FULL + _LN + ("overlap_bf16",), dseed=DROP_SEED + 20),
    _case("small64", 130, 4, 64, SHORT + ("resid_rowscale",)),
    _case("small64", 771, 384, 384, FULL + _LN + ("overlap_bf16",), dseed=DROP_SEED + 1),
    # 128 x 128 tiles, 3-deep ring: EPI_F32 lives here alone (one row, tile + 1, every (alpha, beta)); K = 1 .. 4 k-tiles; N = 388: narrow
    # store and a ragged column tile; 300 x 768 x 768: the K >= 768 rule keeps an under-filled grid off the 64 x 64 tiles
    _case("tile128", 1, 8, 32, _F32),
    _case("tile128", 129, 132, 128, _F32),
    _case("tile128", 11009, 384, 32, SHORT),
    _case("tile128", 11009, 384, 64, SHORT + _F32),
    _case("tile128", 11009, 384, 96, SHORT),
    _case("tile128", 11009, 384, 128, FULL + _LN + ("overlap_bf16",), dseed=DROP_SEED + 103),
    _case("tile128", 8321, 388, 384, FULL + _LN + _F32, dseed=DROP_SEED + 217),
    _case("tile128", 300, 768, 768, SHORT + ("resid_ln", "gelu_aux")),
    # ... split-K (EPI_F32, beta = 1): 33 k-tiles over 4 splits of 9 (ragged last split); the long-K case of test_gemm_epilogues
    _case("tile128", 136, 72, 1056, _F32[1:]),
    _case("tile128", 384, 1536, 4160, _F32[1:]),
    # two-wave-group 256 x 256 tiles, 10-slot ring of 64-wide k-tiles: 1, 2, 10, 11 k-tiles; ragged last row tile; N = 1152: whole and ragged
    # column tile (wide and narrow in one launch); N = 1156: narrow everywhere; N = 1024: whole column tiles; the K >= 768 rule
    _case("pp256", 39173, 1152, 64, SHORT),
    _case("pp256", 39173, 1152, 128, FULL + _LN + ("overlap_bf16",)),
    _case("pp256", 39173, 1156, 128, NARROW),
    _case("pp256", 48901, 1024, 640, SHORT),
    _case("pp256", 48901, 1024, 704, SHORT),
    _case("pp256", 10757, 768, 768, SHORT + ("resid_ln", "overlap_bf16")),
    # lockstep 256-row kernel: what the plan returns for K % 64 == 32
    _case("big256", 39173, 1152, 32, SHORT),
    _case("big256", 39173, 1152, 96, FULL),
    _case("big256", 39173, 1156, 96, NARROW),
    _case("big256", 8200, 1024, 800, SHORT),
)
# (dseed: the first dropout seed from DROP_SEED on whose mask has a kept and a dropped element on every 16 x 16 block of the last row tile, the
# clipped ones included -- one row of 16 at M = 11009 and 8321; searched on the CPU, asserted by tests/test_cpu_gemm_cases.py)
PRODUCTION_PLANS = ("small64", "tile128", "pp256", "big256")


def by_id(cid):
    return next(c for c in CASES if c["id"] == cid)


def form(name):
    return _F[name]


def params():
    """[(case, form)] and their ids, in an order that keeps the forms of one shape together (the float64 product is shared)."""
    pairs = [(c, _F[n]) for c in CASES for n in c["forms"]]
    return pairs, ["%s-%s" % (c["id"], f["name"]) for c, f in pairs]


# ---- seeded inputs -------------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.Generator(np.random.PCG64([int(k) for k in key]))


def _bf(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


@functools.lru_cache(maxsize=2)
def operands(M, N, K, seed, overlap):
    """(A, B) as bf16 CPU tensors: A [M, K], or with overlap the flat buffer of (M - 1) overlap + K elements whose rows slide by ``overlap``."""
    rng = _rng(seed, M, N, K, 1)
    if overlap:
        a = rng.standard_normal((M - 1) * overlap + K, dtype=np.float32)
        a[3::overlap] += 1.0
    else:
        a = rng.standard_normal((M, K), dtype=np.float32)
        a[:, 3] += 1.0
    b = 0.1 * rng.standard_normal((N, K), dtype=np.float32)
    b[min(5, N - 1)] += 0.25
    return _bf(a), _bf(b)


def a_rows(a, M, K, overlap):
    """the logical [M, K] view of operands()[0]"""
    return torch.as_strided(a, (M, K), (overlap, 1)) if overlap else a


def bias_of(c):
    return torch.from_numpy(_rng(c["seed"], c["N"], 2).standard_normal(c["N"], dtype=np.float32))


@functools.lru_cache(maxsize=2)
def resid_of(M, N):
    """fp32 [M, N]: the residual stream / C0 of the accumulating forms / the pre-LayerNorm sums (scaled and shifted: a real mean and variance)"""
    return torch.from_numpy(_rng(M, N, 3).standard_normal((M, N), dtype=np.float32)).mul_(1.5).add_(0.2)


@functools.lru_cache(maxsize=2)
def preact_of(M, N):
    """bf16 [M, N]: the saved pre-activations a DGELU epilogue reads"""
    return torch.from_numpy(_rng(M, N, 4).standard_normal((M, N), dtype=np.float32)).mul_(1.5).to(torch.bfloat16)


def row_scale_of(M):
    """fp32 [ceil(M / RPS)] in {0, 0.625, 1 / 0.9}: DropPath's per-sample scale; sample 0 kept, sample 1 dropped where there is one"""
    ns = (M + RPS - 1) // RPS
    sc = _rng(M, 5).choice(np.array([0.0, 0.625, 1.0 / 0.9], np.float32), size=ns)
    sc[0] = np.float32(1.0 / 0.9)
    if ns > 1:
        sc[1] = 0.0
    return torch.from_numpy(sc)


def ln_of(y, N):
    """(mean [M], rstd [M], gamma [N], beta [N]) fp32 of the pre-LayerNorm sums y, as a LayerNorm launch would have left them"""
    yd = y.double()
    mean = yd.mean(1)
    rstd = 1.0 / torch.sqrt(yd.var(1, unbiased=False) + 1e-12)
    r = _rng(N, 6)
    gamma = torch.from_numpy(1.0 + 0.1 * r.standard_normal(N, dtype=np.float32))
    beta = torch.from_numpy(0.1 * r.standard_normal(N, dtype=np.float32))
    return mean.float(), rstd.float(), gamma, beta


@functools.lru_cache(maxsize=2)
def keep_of(M, N, dseed):
    return torch.from_numpy(BR.keep_mask(dseed, DROP_SITE, (M, N), DROP_P))


# ---- allocations with poisoned padding ---------------------------------------------------------------------------------------------------
def _poison(buf, nan):
    if nan:
        buf.fill_(float("nan"))
    else:
        buf.view(torch.int16).fill_(PATTERN)
    return buf


def arena2(rows, width, ld, dtype, device, nan, fill=None):
    """(buffer, [rows, width] view at element FRONT with pitch ld): padding poisoned (NaN or PATTERN), the block itself = fill, or NaN."""
    buf = _poison(torch.empty(FRONT + (rows + ROWS_AFTER) * ld, dtype=dtype, device=device), nan)
    view = torch.as_strided(buf, (rows, width), (ld, 1), FRONT)
    if fill is not None:
        view.copy_(fill)
    else:
        view.fill_(float("nan"))
    return buf, view


def arena1(vec, device, extra=ROWS_AFTER):
    """a 1-d operand (bias, statistics, scales; or the flat buffer of overlapping rows) between NaN padding -> (buffer, view)"""
    buf = _poison(torch.empty(FRONT + vec.numel() + extra, dtype=vec.dtype, device=device), True)
    view = buf[FRONT:FRONT + vec.numel()]
    view.copy_(vec)
    return buf, view


class Launch:
    """Everything one (case, form) launch reads and writes, on ``device`` ('cpu' for the float32 restatement, 'cuda:0' for the kernels)."""

    def __init__(self, c, f, device):
        self.c, self.f, self.device = c, f, device
        M, N, K = c["M"], c["N"], c["K"]
        self.M, self.N, self.K = M, N, K
        a, b = operands(M, N, K, c["seed"], f["overlap"])
        if f["overlap"]:
            self.lda = f["overlap"]
            self.A_buf, flat = arena1(a, device, extra=ROWS_AFTER * self.lda)
            self.A = torch.as_strided(self.A_buf, (M, K), (self.lda, 1), FRONT)
        else:
            self.lda = K + f["op_pad"]
            self.A_buf, self.A = arena2(M, K, self.lda, torch.bfloat16, device, True, a)
        self.ldb = K + f["op_pad"]
        self.B_buf, self.B = arena2(N, K, self.ldb, torch.bfloat16, device, True, b)
        self.bias = arena1(bias_of(c), device)[1] if f["bias"] else None
        bf16_out = f["epi"] in BF16_EPIS
        self.ldc = N + f["c_pad"]
        self.ldaux = N + f["aux_pad"]
        self.resid = self.c0 = self.preact = self.aux_out = self.aux_out_buf = self.row_scale = self.ln = self.keep = None
        if f["resid"] is not None:
            r = resid_of(M, N)
            if f["resid"] == "aux":
                self.resid = arena2(M, N, self.ldaux, torch.float32, device, True, r)[1]
                self.C_buf, self.C = arena2(M, N, self.ldc, torch.float32, device, False)
            else:
                self.C_buf, self.C = arena2(M, N, self.ldc, torch.float32, device, False, r)
                self.resid = self.C.clone()
            if f["ln"]:
                self.ln = tuple(arena1(t, device)[1] for t in ln_of(r, N))
        elif f["epi"] == ops.EPI_F32:
            fill = resid_of(M, N) if f["beta"] != 0.0 else None
            self.C_buf, self.C = arena2(M, N, self.ldc, torch.float32, device, False, fill)
            self.c0 = self.C.clone() if fill is not None else None
        else:
            self.C_buf, self.C = arena2(M, N, self.ldc, torch.bfloat16, device, False)
        if f["epi"] == ops.EPI_DGELU_BF16:
            self.preact = arena2(M, N, self.ldaux, torch.bfloat16, device, True, preact_of(M, N))[1]
        if f["aux_out"]:
            self.aux_out_buf, self.aux_out = arena2(M, N, self.ldaux, torch.bfloat16, device, False)
        if f["row_scale"]:
            self.row_scale = arena1(row_scale_of(M), device)[1]
        if f["drop"]:
            self.keep = keep_of(M, N, c["dseed"]).to(device)
        assert bf16_out == (self.C.dtype == torch.bfloat16)
        self.before = [(buf, buf.clone()) for buf in (self.C_buf, self.aux_out_buf) if buf is not None]

    def drop(self):
        return ops.Drop(self.c["dseed"], DROP_SITE, DROP_P) if self.f["drop"] else None

    def row_scale_rows(self):
        """[M] the scale of every row, or None"""
        return None if self.row_scale is None else self.row_scale.repeat_interleave(RPS)[:self.M]

    def pad_touched(self):
        """element offsets (first few) of output padding that no longer holds what was there before the launch"""
        bad = []
        for (buf, was), ld in zip(self.before, (self.ldc, self.ldaux)):
            now, ref = buf.clone(), was
            torch.as_strided(now, (self.M, self.N), (ld, 1), FRONT).copy_(torch.as_strided(ref, (self.M, self.N), (ld, 1), FRONT))
            if not torch.equal(now.view(torch.int16), ref.view(torch.int16)):
                d = (now.view(torch.int16) != ref.view(torch.int16)).reshape(-1).nonzero().reshape(-1)[:4].tolist()
                n16 = buf.element_size() // 2
                bad += [("C" if buf is self.C_buf else "aux_out", i // n16 - FRONT) for i in d]
        return bad


# ---- float64 expectation -------------------------------------------------------------------------------------------------------------------
_PRODUCTS = {}


def product(c, overlap, device, keep=2):
    """(P, S0) = (A B^T, |A| |B|^T) in float64 on ``device`` from the bf16 values cast up; the last ``keep`` products stay cached (a shape's forms
    share one).  On the GPU this is the vendor library's float64 matmul -- independent of the code under test."""
    key = (c["M"], c["N"], c["K"], c["seed"], overlap, str(device))
    if key not in _PRODUCTS:
        while len(_PRODUCTS) >= keep:
            _PRODUCTS.pop(next(iter(_PRODUCTS)))
        a, b = operands(c["M"], c["N"], c["K"], c["seed"], overlap)
        A = a_rows(a, c["M"], c["K"], overlap).to(device).double()
        Bt = b.to(device).double().t()
        _PRODUCTS[key] = (A @ Bt, A.abs() @ Bt.abs())
    return _PRODUCTS[key]


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def half_ulp_bf16(x):
    """half the spacing of bf16 (8 significant bits) at magnitude x >= 0 (float64), exact: 2^(floor(log2 x) - 8), from the exponent bits;
    below the smallest normal 2^-126 the spacing is that of the denormals, 2^-133"""
    e = x.view(torch.int64) >> 52                       # the biased exponent (x >= 0: no sign bit); in place from here on: x has 4.5e7 elements
    e.clamp_(min=1023 - 126).sub_(8).bitwise_left_shift_(52)
    return e.view(torch.float64)


def _bf16_tol(want, lt, e=0.0):
    return half_ulp_bf16(want.abs().add_(lt)).add_(lt).add_(e)


def expect(L):
    """What the launch L must produce: dict(want, tol[, exact = (bool mask, fp32 / bf16 values those elements equal bit for bit)][, aux_want,
    aux_tol]) as float64 tensors on L.device."""
    f, dev = L.f, L.device
    P, S0 = product(L.c, f["overlap"], dev)
    u = 2.0 ** -24
    out = {}
    if f["epi"] == ops.EPI_F32:
        want, S = f["alpha"] * P, abs(f["alpha"]) * S0
        if L.c0 is not None:
            c0 = L.c0.double()
            want, S = want + f["beta"] * c0, S + abs(f["beta"]) * c0.abs()
        out.update(want=want, tol=C_ACC * u * S + 2.0 * u * want.abs())
        return out
    v, S = P, S0
    if L.bias is not None:
        v, S = v + L.bias.double(), S + L.bias.double().abs()
    s = 1.0 / (1.0 - DROP_P) if L.keep is not None else 1.0
    keepd = L.keep.double() if L.keep is not None else None
    tol32 = C_ACC * u * S
    if f["epi"] == ops.EPI_BF16:
        out.update(want=v, tol=_bf16_tol(v, tol32))
    elif f["epi"] == ops.EPI_GELU_BF16:
        want = gelu64(v) * s
        if keepd is not None:
            want = want * keepd
        out.update(want=want, tol=_bf16_tol(want, GELU_L * s * tol32, GELU_E * s))
        if L.aux_out is not None:
            out.update(aux_want=v, aux_tol=_bf16_tol(v, tol32))
    elif f["epi"] == ops.EPI_DGELU_BF16:
        d = gelu_grad64(L.preact.double())
        vd = v * s
        if keepd is not None:
            vd = vd * keepd
        want = vd * d
        out.update(want=want, tol=_bf16_tol(want, d.abs() * s * tol32, DGELU_ABS * vd.abs()))
    else:
        x = L.resid.double()
        extra = 0.0
        if L.ln is not None:
            mean, rstd, gamma, beta = (t.double() for t in L.ln)
            xg = (x - mean[:, None]) * rstd[:, None] * gamma
            x = xg + beta
            extra = 4.0 * u * (xg.abs() + beta.abs())
        w = v * s
        if keepd is not None:
            w = w * keepd
        Sw = S * s
        rs = L.row_scale_rows()
        if rs is not None:
            w, Sw = w * rs.double()[:, None], Sw * rs.double().abs()[:, None]
        want = x + w
        out.update(want=want, tol=C_ACC * u * (Sw + x.abs()) + 2.0 * u * want.abs() + extra)
        if L.ln is None:
            same = torch.zeros_like(want, dtype=torch.bool)
            if L.keep is not None:
                same |= ~L.keep
            if rs is not None:
                same |= (rs == 0)[:, None]
            out["exact"] = (same, L.resid)
    if L.keep is not None and f["epi"] in BF16_EPIS:
        out["exact"] = (~L.keep, torch.zeros((), dtype=torch.bfloat16, device=dev))
    return out


# ---- the check -----------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _worst(name, got, want, tol, tile):
    err = (got - want).abs_()
    if bool((err <= tol).all()):                          # (NaN compares false)
        return True, float(err.div_(tol.clamp_min(1e-300)).max()), ""
    over = torch.where(torch.isfinite(err), err - tol, torch.full_like(err, float("inf")))
    i = int(over.argmax())
    r, col = divmod(i, got.shape[1])
    msg = "%s: worst element row %d col %d (tile %d, %d; row %d col %d inside it): got %.9g want %.9g |diff| %.3e tol %.3e (%d of %d outside)" % (
        name, r, col, r // tile, col // tile, r % tile, col % tile, float(got[r, col]), float(want[r, col]), float(err[r, col]),
        float(tol[r, col]), int((over > 0).sum()), got.numel())
    return False, float("inf"), msg


def assert_within(name, got, want, tol, tile=128):
    """every element of ``got`` within ``tol`` of ``want`` (float64) and finite; returns max |got - want| / tol"""
    ok, ratio, msg = _worst(name, got.double(), want, tol, tile)
    assert ok, msg
    return ratio


def verify(L, ex=None):
    """Holds the outputs of the launch L (in its arenas) to expect(L): finite, within the per-element bound, exact where exactness is owed,
    padding untouched.  Returns max |got - want| / tol over the outputs; raises AssertionError naming the worst element."""
    ex = expect(L) if ex is None else ex
    tile = TILE[L.c["plan"]]
    name = "%s-%s" % (L.c["id"], L.f["name"])
    ratio = assert_within(name, L.C, ex["want"], ex["tol"], tile)
    if "aux_want" in ex:
        ratio = max(ratio, assert_within(name + " aux_out", L.aux_out, ex["aux_want"], ex["aux_tol"], tile))
    if "exact" in ex:
        mask, val = ex["exact"]
        same = (L.C == 0) if val.dim() == 0 else (_bits(L.C) == _bits(val))
        bad = mask & ~same
        if bool(bad.any()):
            r, col = divmod(int(bad.reshape(-1).to(torch.int8).argmax()), L.N)
            raise AssertionError("%s: row %d col %d must equal %s bit for bit, got %.9g (%d such elements)" % (
                name, r, col, "0" if val.dim() == 0 else "the residual %.9g" % float(val[r, col]), float(L.C[r, col]), int(bad.sum())))
    touched = L.pad_touched()
    assert not touched, "%s: output padding overwritten at (buffer, element offset from the first valid) %s" % (name, touched)
    return ratio


# ---- float32 restatements ------------------------------------------------------------------------------------------------------------------
def accumulate32(c, overlap, reverse=False):
    """A B^T accumulated in float32 over 32-wide k-chunks, first to last (the kernels' order) or last to first: float32 CPU tensor [M, N]"""
    a, b = operands(c["M"], c["N"], c["K"], c["seed"], overlap)
    A, B = a_rows(a, c["M"], c["K"], overlap).float(), b.float()
    acc = torch.zeros(c["M"], c["N"])
    ks = range(0, c["K"], 32)
    for k in (reversed(ks) if reverse else ks):
        acc += A[:, k:k + 32] @ B[:, k:k + 32].t()
    return acc


def chunk32(c, overlap, k0, rows, cols):
    """the float32 product of one 32-wide k-chunk on a block of rows x cols (what a kernel that skips the chunk there leaves out)"""
    a, b = operands(c["M"], c["N"], c["K"], c["seed"], overlap)
    return a_rows(a, c["M"], c["K"], overlap)[rows, k0:k0 + 32].float() @ b[cols, k0:k0 + 32].float().t()


def gelu_erf32(x):
    """csrc/common.h gelu_erf in float32"""
    w = x.abs() * 0.8493218
    t = 1.0 / (0.27273747 * w + 1.0)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    r = 1.0 - poly * torch.exp2(-(w * w))
    h = 0.5 * x
    return h.abs() * r + h


def gelu_erf_grad32(x):
    """csrc/common.h gelu_erf_grad (erf_as: Abramowitz-Stegun 7.1.26) in float32"""
    z = x * 0.70710678118654752440
    ax = z.abs()
    t = 1.0 / (1.0 + 0.3275911 * ax)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    erf = torch.copysign(1.0 - poly * torch.exp2(-ax * ax * 1.4426950408889634), z)
    cdf = 0.5 * (1.0 + erf)
    pdf = 0.39894228040143267794 * torch.exp2(-0.5 * x * x * 1.4426950408889634)
    return cdf + x * pdf


def restate(L, acc, row_scale_rows=None):
    """The launch in float32 on the CPU: ``acc`` (accumulate32) + bias, the epilogue as csrc/gemm.hip states it, rounded once to the output
    type, written into L's arenas as a kernel would.  row_scale_rows: the [M] scales to use instead of L's (a planted fault)."""
    f = L.f
    assert acc.dtype == torch.float32 and L.device == "cpu"
    if f["epi"] == ops.EPI_F32:
        x = np.float32(f["alpha"]) * acc
        if L.c0 is not None:
            x = x + np.float32(f["beta"]) * L.c0
        L.C.copy_(x)
        return
    v = acc + L.bias if L.bias is not None else acc.clone()
    s = np.float32(1.0 / (1.0 - DROP_P))
    zero = torch.zeros((), dtype=torch.float32)
    if f["epi"] == ops.EPI_BF16:
        L.C.copy_(v.to(torch.bfloat16))
    elif f["epi"] == ops.EPI_GELU_BF16:
        if L.aux_out is not None:
            L.aux_out.copy_(v.to(torch.bfloat16))
        h = gelu_erf32(v)
        if L.keep is not None:
            h = torch.where(L.keep, h * s, zero)
        L.C.copy_(h.to(torch.bfloat16))
    elif f["epi"] == ops.EPI_DGELU_BF16:
        if L.keep is not None:
            v = torch.where(L.keep, v * s, zero)
        L.C.copy_((v * gelu_erf_grad32(L.preact.float())).to(torch.bfloat16))
    else:
        x = L.resid.clone()
        if L.ln is not None:
            mean, rstd, gamma, beta = L.ln
            x = (x - mean[:, None]) * rstd[:, None] * gamma + beta
        if L.keep is not None:
            v = torch.where(L.keep, v * s, zero)
        rs = row_scale_rows if row_scale_rows is not None else L.row_scale_rows()
        if rs is not None:
            v = rs[:, None] * v
        L.C.copy_(x + v)


# ---- what the two constants are made of -----------------------------------------------------------------------------------------------------
def product_keys():
    """every distinct (case, overlap) product of CASES"""
    seen, keys = set(), []
    for c in CASES:
        for ov in sorted({_F[n]["overlap"] for n in c["forms"]}):
            k = (c["M"], c["N"], c["K"], c["seed"], ov)
            if k not in seen:
                seen.add(k)
                keys.append((c, ov))
    return keys


def acc_ratio(c, overlap, reverse):
    """largest |float32 restatement + bias - float64| / (2^-24 S) of one product"""
    P, S0 = product(c, overlap, "cpu")
    b = bias_of(c)
    got = (accumulate32(c, overlap, reverse) + b).double()
    return float(((got - (P + b.double())).abs() / (2.0 ** -24 * (S0 + b.double().abs()))).max())


def measure_c_acc():
    return max(acc_ratio(c, ov, rev) for c, ov in product_keys() for rev in (False, True))


def measure_dgelu_abs():
    """largest deviation of the float32 derivative formula from float64 GELU' over every finite bf16 value"""
    p = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    p = p[torch.isfinite(p.float())]
    return float((gelu_erf_grad32(p.float()).double() - gelu_grad64(p.double())).abs().max())
