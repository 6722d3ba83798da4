"""The cases of tests/test_{cpu,gpu}_mlp_fused_cases.py: the four shipped instantiations of csrc/mlp_fused.hip / mlp_fused_body.h -- srhip_mlp_fused
('dense': LayerNorm, fc1, GELU, fc2, residual, with the backward operands of the leading rows), srhip_mlp_fused_proj ('proj': + the attention output
projection, the first residual and the next block's norm1), its row-pitch form ('strided') and its DropPath-plan form ('planned') -- element by
element against float64.  Nothing is stored: every input is rebuilt from its seed (PCG64), every expected value is recomputed.  Everything here is
numpy on the host; run_gpu() alone touches the device (it uploads a Launch's buffers, launches, and brings the outputs back), so verify() is the
same function for a kernel's outputs and for the float32 restatement tests/test_cpu_mlp_fused_cases.py feeds it.

In scope: mlp_fused_kernel<384, 0, 4>, <384, 0, 4, true, 1>, <384, 0, 4, true, 1, true> and mlp_planned_kernel<384, 4>.  SR_TUNE_ENV of csrc/common.h
is a null pointer in a shipped build (it reads the environment only under SRHIP_TUNING), so SRHIP_MLP_SPREAD is inert there: the SPREAD = 0
instantiation and the SRHIP_MLP_DEBUG variants cannot be launched and are not tested.

Why element by element: the whole-tensor norms of test_mlp_fused / test_mlp_fused_proj move by 1 / sqrt(M) when one row is wrong and by far less
when one 64-wide hidden chunk of one 16-row wave is (tests/_gemm_cases.py has the figures for the GEMMs; test_cpu_mlp_fused_cases.py states them
for these kernels, NORM_BLIND below lists the planted faults they let pass).

Inputs.  x fp32 with column 7 shifted, ao bf16 with column 300 shifted, Wp / W1 / W2 bf16 with row 5 / 9 / 11 shifted (a transposed or permuted
fragment shows), non-trivial fp32 biases and LayerNorm affines.  b1 alternates between the levels 0.3 and 0.9 from one 64-wide hidden chunk to
the next (+- 0.1 noise): in every chunk a fixed share of the GELU outputs is clearly non-zero (share_clear(), asserted per case and chunk by the
CPU test), so a dropped, repeated or mis-biased chunk is far outside the bound on every row.  DropPath factors are drawn per sample from
{0, 1, 1 / 0.9, 1 / 0.95}; the first four samples of a case with two factors hold the four combinations of (rs1 = 0 or not, rs2 = 0 or not).
(A planned launch's rs2 pattern is what its n_mlp says: the four combinations occur over the n_mlp values of a shape, not inside n_mlp = 0.)
Every operand and output lies inside a larger allocation at a 16-byte-aligned non-zero offset (FRONT elements).  Operand padding -- the front,
the rows past M, and for the strided form the elements between the rows of x and ao -- is NaN.  Output padding holds PATTERN and must come back
bit for bit (strided: every element between the rows of x_out; the save buffers: rows save_rows ..); output blocks start as NaN.

References: float64, in the order of mlp_fused_body.h, with the kernel's rounding points where they can be restated: bf16(rs1 ao) (fp32 product,
then round-to-nearest-even: pack_bf2 of csrc/common.h is __builtin_convertvector to __bf16 = v_cvt_pk_bf16_f32, RNE) when ao_scaled is off and
rs1 != 1, bf16 of the normalised row, bf16(rs2 GELU).  u = 2^-24, hu(v) = half a bf16 ulp AT the magnitude v (exact; never a flat 2^-9 v:
tests/_attn_cases.py records why).

(1) Stage by stage, on what the kernel hands back (dense with save_rows; ln_next of the proj forms): every stage against float64 of that stage's
    ACTUAL input, so an error cannot cancel between stages.
      s_mean      |got - mean| <= C_STAT u mean|x|;    s_rstd  |got - rstd| <= C_STAT u rstd
      s_ln2       N = u (|xhat gamma| + |beta| + |gamma| rstd mean|x|):  |got - want| <= C_NORM N + hu(|want| + C_NORM N)
      s_pre       from the returned s_ln2: T = C_ACC u (|ln2| |W1|^T + |b1|):  <= T + hu(|want| + T)
      s_h         from the returned s_pre (the fp32 pre-activation is within hu(s_pre) of it): GELU_L hu(|s_pre|) + GELU_E + hu(|want| + those)
      x_out       saved rows, from the returned s_h: C_ACC u (|rs| (|h| |W2|^T + |b2|) + |x|) + 2 u |want|
      ln_next     from the returned x_out: C_NORM N + hu(|want| + C_NORM N)
(2) End to end (every row of every form), first order, as tests/_attn_cases.py does for the fused attention block:
      e1   = C_ACC u (|ao'| |Wp|^T + |rs1 bp| + |x|) + 2 u |x1|                 the projection and first residual (0 for dense)
      dxn  = LayerNorm's derivative applied to e1 + C_NORM N(x1);  exn = dxn + hu(|xn| + dxn)       per value
      dpre = exn |W1|^T + C_ACC u (|xn_b| |W1|^T + |b1|)
      dh   = |rs2| (GELU_L dpre + E(pre)) + u |h|;  eh = dh + hu(|h| + dh)      E = GELU_E (gelu_erf, dense), max(7e-5, 5e-6 |pre|) (gelu_poly2)
      tol  = e1 + |rs| eh |W2|^T + C_ACC u (|rs| (|h_b| |W2|^T + |b2|) + |x1|) + 2 u |want|
(2') The same propagation with the two rounding terms taken exactly instead of to first order.  The reference rounds xn and h where the kernel
    does, so the kernel's bf16 value IS the reference's unless a rounding boundary lies within dxn (dh) of the float64 value, and then it is
    the neighbour: exn = 0 or dxn + a whole ulp, per element (flip_bf16), likewise eh.  Rigorous, and two orders of magnitude below (2), whose
    worst-case sum of 384 x Hd half-ulps reaches 1.6 at Hd = 1536 -- more than a dropped hidden chunk moves a row.  x_out is held to the
    smaller of (2) and (2') per element: never wider than (2).
    (A ratio close to 1 on x_out is a row in which the one rounding boundary within reach was crossed: (2') is attained there, not exceeded.)
Exact: rows whose factors are all 0 equal x bit for bit; in place == out of place, strided == dense, planned == dense bit for bit (the GPU test).

Constants.  C_ACC, GELU_L, GELU_E and the gelu_poly2 figure come from tests/_gemm_cases.py.  C_STAT and C_NORM are measured by measure_constants()
on the float32 restatement of the LayerNorm alone (both register layouts: per lane, then the two cross-lane steps; forward and reversed),
without the bf16 rounding, against float64; committed as 8 x the measurement, and re-measured by the CPU test (held between 4 and 16 times).
They are never set from what a kernel produced: a kernel outside the bound is a finding.

Both large-M cases are restated and verified whole (every row of every tile; no sample is drawn): at Hd = 128 that costs about a second."""
import functools

import numpy as np
import torch

from _gemm_cases import C_ACC, GELU_E, GELU_L, GELU_POLY2_ABS, GELU_POLY2_REL

D, EPS = 384, 1e-6
FBM, WAVE_ROWS, CH, GRID = 128, 16, 64, 256      # rows per tile and per wave, hidden units per chunk, workgroups of a full launch
FRONT, ROWS_AFTER = 64, 64                       # elements before the first row, rows after the last
PATTERN = 0x4B1D                                 # every 16 bits of output padding (finite as bf16 and, doubled, as fp32)
NAN16 = 0x7FC0
U = 2.0 ** -24
BIG_M = GRID * FBM + 17                          # 32785: 257 tiles, workgroup 0 takes a second tile, and that tile is ragged
FACTORS = np.array([0.0, 1.0, 1.0 / 0.9, 1.0 / 0.95], np.float32)

# measured by measure_constants() (test_cpu_mlp_fused_cases.py holds each committed constant between 4 and 16 times its measurement):
#   largest |fp32 mean - mean| / (u mean|x|) and |fp32 rstd - rstd| / (u rstd):   C_STAT_MEASURED
#   largest |fp32 normalised value - float64| / N:                                C_NORM_MEASURED
C_STAT_MEASURED, C_NORM_MEASURED = 4.189, 4.611
C_STAT, C_NORM = 8.0 * C_STAT_MEASURED, 8.0 * C_NORM_MEASURED


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def _dense(M, Hd, rps, scale, save):
    return dict(entry="dense", M=M, Hd=Hd, rps=rps, scale=scale, save=save, fac=False, ao_scaled=False, ln=False, pitch=D,
                id="dense-%dx%d-rps%d%s-save%d" % (M, Hd, rps, "s" if scale else "", save))


def _proj(M, Hd, rps, fac, ao_scaled, ln, entry="proj", pitch=D):
    return dict(entry=entry, M=M, Hd=Hd, rps=rps, scale=False, save=0, fac=fac, ao_scaled=ao_scaled, ln=ln, pitch=pitch,
                id="%s-%dx%d-rps%d%s%s%s%s" % (entry, M, Hd, rps, "-fac" if fac else "", "-aos" if ao_scaled else "", "-ln" if ln else "",
                                               "-pitch%d" % pitch if entry == "strided" else ""))


def _planned(N, B, Hd, n_mlp, plan):
    return dict(entry="planned", M=N * B, Hd=Hd, rps=N, scale=False, save=0, fac=True, ao_scaled=True, ln=True, pitch=D, B=B, n_mlp=n_mlp,
                plan=plan, id="planned-%dx%d-Hd%d-nmlp%d-%s" % (N, B, Hd, n_mlp, plan))


DENSE = (
    _dense(1, 128, 0, False, 1),               # one row, saved: save_rows = M
    _dense(15, 256, 1, True, 0),               # a factor per row
    _dense(16, 128, 5, True, 16),              # save_rows = M on a wave boundary; three sample boundaries inside the wave
    _dense(17, 256, 5, True, 15),              # save_rows ends inside a wave's 16 rows
    _dense(127, 1536, 0, False, 17),           # ... one row into the second wave
    _dense(128, 1536, 257, True, 128),         # a whole tile, save_rows = M on the tile boundary
    _dense(129, 4096, 5, True, 128),           # the largest hidden width (156672 bytes of LDS); save_rows on the tile boundary, M one past it
    _dense(129, 128, 1, True, 1),
    _dense(3 * 257, 1536, 257, True, 130),     # save_rows inside the first wave of the second tile
    _dense(3 * 257, 256, 5, False, 3 * 257),   # rows_per_sample without a factor; every row saved
    _dense(BIG_M, 128, 257, True, BIG_M),      # saved rows in a workgroup's second tile; ragged last tile
)
PROJ = (
    _proj(1, 128, 0, False, False, True),
    _proj(15, 256, 1, True, False, False),
    _proj(16, 128, 5, True, True, True),
    _proj(17, 1536, 5, True, False, True),
    _proj(127, 256, 0, False, False, False),
    _proj(128, 128, 5, True, True, False),
    _proj(129, 4096, 5, True, False, True),
    _proj(3 * 257, 1536, 5, True, True, True),
    _proj(3 * 257, 256, 0, False, False, True),
    _proj(BIG_M, 128, 257, True, False, True),
)
STRIDED = (
    _proj(1, 128, 0, False, False, False, "strided", D + 8),
    _proj(17, 256, 1, True, False, True, "strided", D),           # ln_next: only at pitch D
    _proj(17, 128, 0, False, False, False, "strided", 257 * D),
    _proj(130, 1536, 1, True, True, False, "strided", 257 * D),   # the class-token rows of a [130, 257, D] residual stream
    _proj(130, 256, 5, True, False, False, "strided", D + 8),
    _proj(BIG_M, 128, 257, True, False, False, "strided", D + 8),
)
PLANNED = tuple(_planned(N, B, Hd, n, p) for N, B, Hd in ((257, 3, 1536), (5, 30, 256), (1, 130, 128))
                for n, p in ((0, "kernel"), (1, "kernel"), (1, "hand"), (B - 1, "kernel"), (B - 1, "hand"), (B, "kernel"), (B, "hand"))) + (
    # 33410 rows = 262 tiles: heavy tiles 256 .. 258 and the straddling tile 259 (129 * 257 = 33153 rows keep the MLP) are second tiles of their
    # workgroups, and so are the light tiles 260, 261
    _planned(257, 130, 128, 129, "hand"),)
CASES = DENSE + PROJ + STRIDED + PLANNED
BY_ENTRY = {"dense": DENSE, "proj": PROJ, "strided": STRIDED, "planned": PLANNED}


def by_id(cid):
    return next(c for c in CASES if c["id"] == cid)


def dense_twin(c):
    """the srhip_mlp_fused_proj launch of the same operands and factors (what a strided or planned launch must equal bit for bit)"""
    return dict(c, entry="proj", pitch=D, id=c["id"] + "-as-dense")


# ---- number formats ------------------------------------------------------------------------------------------------------------------------
def bf16_round(a):
    """float32 -> the nearest bf16 value (ties to even), as float32"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def bf16_round64(a):
    """float64 -> the nearest bf16 value (ties to even, one rounding), as float64 (normal range)"""
    u = np.ascontiguousarray(a, np.float64).view(np.uint64)
    return ((u + (((u >> np.uint64(45)) & np.uint64(1)) + np.uint64((1 << 44) - 1))) & np.uint64(0xFFFFE00000000000)).view(np.float64)


def to_bits(a):
    """float32 holding bf16 values -> uint16 bits"""
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def from_bits(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def half_ulp_bf16(x):
    """half the spacing of bf16 (8 significant bits) at magnitude x >= 0 (float64), exact: 2^(floor(log2 x) - 8); denormal spacing below 2^-126"""
    _, e = np.frexp(x)                                  # x = m 2^e, 0.5 <= m < 1
    return np.where(x < 2.0 ** -126, 2.0 ** -134, np.ldexp(1.0, np.maximum(e, -125) - 9))


def gelu64(x):
    """exact-erf GELU in float64 (torch's CPU erf: numpy has none)"""
    x = np.ascontiguousarray(x, np.float64)
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(x / np.sqrt(2.0))).numpy())


def gelu_poly2_err(pre):
    """what test_gelu_forms_against_exact_erf holds gelu_poly2 to"""
    return np.maximum(GELU_POLY2_ABS, GELU_POLY2_REL * np.abs(pre))


# ---- seeded inputs -------------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.Generator(np.random.PCG64([int(k) for k in key]))


@functools.lru_cache(maxsize=2)
def operands(M, Hd):
    """the logical operands of a shape as float32 arrays (bf16 operands hold bf16 values); ao32 is the attention output before its rounding"""
    r = _rng(M, Hd, 1)
    n = lambda *s: r.standard_normal(s, dtype=np.float32)       # noqa: E731
    x = n(M, D)
    x[x == 0] = 1.0                                   # (an exact zero turns up once in ~1e7 draws; -0 + 0 would not come back bit for bit)
    x[:, 7] += 3.0
    ao32 = np.float32(0.7) * n(M, D)
    ao32[:, 300] += 2.0
    Wp = np.float32(0.06) * n(D, D)
    Wp[5] += 0.05
    W1 = np.float32(0.05) * n(Hd, D)
    W1[9] += 0.03
    W2 = np.float32(0.03) * n(D, Hd)
    W2[11] += 0.03
    b1 = np.float32(0.1) * n(Hd) + np.where((np.arange(Hd) // CH) % 2 == 0, 0.3, 0.9).astype(np.float32)
    bp, b2 = np.float32(0.2) * n(D), np.float32(0.1) * n(D)
    bp[2], b2[3] = 0.5, -0.5
    o = dict(x=x, ao32=ao32, Wp=bf16_round(Wp), W1=bf16_round(W1), W2=bf16_round(W2), b1=b1, bp=bp, b2=b2,
             gam=1.0 + np.float32(0.2) * n(D), bet=np.float32(0.1) * n(D), gn=1.0 + np.float32(0.3) * n(D), bn=np.float32(0.2) * n(D))
    for v in o.values():
        v.setflags(write=False)
    return o


def factors_of(c):
    """(rs1, rs2) float32 per sample, None where the launch has none; dense: (None, row_scale)"""
    M, rps = c["M"], c["rps"]
    if not (c["scale"] or c["fac"]):
        return None, None
    ns = (M + rps - 1) // rps
    r = _rng(M, rps, 5)
    if c["entry"] == "planned" or "n_mlp" in c:
        perm = r.permutation(ns)
        r2 = np.zeros(ns, np.float32)
        r2[perm[:c["n_mlp"]]] = r.choice(FACTORS[1:], size=c["n_mlp"])
        r1 = r.choice(FACTORS[1:], size=ns)
        r1[perm[0::2]] = 0.0
        return r1, r2
    if c["scale"]:
        s = r.choice(FACTORS, size=ns)
        s[0] = FACTORS[2]
        if ns > 1:
            s[1] = 0.0
        return None, s
    r1, r2 = r.choice(FACTORS, size=ns), r.choice(FACTORS, size=ns)
    k = min(ns, 4)
    r1[:k] = np.array([0.0, FACTORS[3], 0.0, FACTORS[2]], np.float32)[:k]
    r2[:k] = np.array([0.0, 0.0, FACTORS[2], FACTORS[3]], np.float32)[:k]
    return r1, r2


def plan_of(c, r2):
    """int32 [1 + B]: n_mlp, then the samples that keep the MLP branch and the dropped ones -- 'kernel': each ascending (what
    srhip_vit_droppath_plan writes), 'hand': each descending (a permutation the plan kernel would not write, and the launch must still follow)"""
    keep, dropped = np.flatnonzero(r2 != 0), np.flatnonzero(r2 == 0)
    if c["plan"] == "hand":
        keep, dropped = keep[::-1], dropped[::-1]
    return np.concatenate([[len(keep)], keep, dropped]).astype(np.int32)


def share_clear(c):
    """per hidden chunk: the share of (row, hidden unit) whose GELU output is at least 0.25 in magnitude (float64, LayerNorm of x)"""
    o = operands(c["M"], c["Hd"])
    _, _, xhat = ln64(o["x"].astype(np.float64))
    pre = (xhat * o["gam"] + o["bet"]) @ o["W1"].astype(np.float64).T + o["b1"]
    return (np.abs(gelu64(pre)) >= 0.25).reshape(c["M"], -1, CH).mean(axis=(0, 2))


# ---- a launch: operands, arenas, outputs ------------------------------------------------------------------------------------------------------
def _arena(rows, width, pitch, dtype, nan, fill=None, rows_after=ROWS_AFTER):
    """(flat buffer, [rows, width] view at element FRONT with the given pitch); padding NaN or PATTERN; the block = fill, or NaN"""
    n = FRONT + (rows + rows_after) * pitch
    if dtype == np.uint16:
        buf = np.full(n, NAN16 if nan else PATTERN, np.uint16)
    elif dtype == np.int32:
        buf = np.full(n, -1, np.int32)
    else:
        buf = np.full(n, np.nan, np.float32) if nan else np.full(n, PATTERN * 0x10001, np.uint32).view(np.float32)
    view = np.lib.stride_tricks.as_strided(buf[FRONT:], (rows, width), (pitch * buf.itemsize, buf.itemsize))
    if fill is not None:
        view[...] = fill
    elif dtype == np.uint16:
        view[...] = NAN16
    elif dtype == np.float32:
        view[...] = np.nan
    return buf, view


def _bits(a):
    return a.view(np.uint16 if a.itemsize == 2 else np.uint32)


class Launch:
    """Everything one launch of a case reads and writes, on the host.  ``buf[name]`` are the flat allocations, ``v[name]`` their logical views
    (bf16 as uint16 bits).  Outputs: xo [, ln][, s_ln2, s_pre, s_h, s_mean, s_rstd]; ``init[name]`` is what each held before the launch."""

    def __init__(self, c, inplace=False, o=None, factors=None):
        """o, factors: other operands and factors than the case's own (the CPU test restates the inputs of tests/test_gpu_kernels.py)"""
        self.c, self.inplace = c, inplace
        M, Hd, pitch = c["M"], c["Hd"], c["pitch"]
        o = self.o = operands(M, Hd) if o is None else o
        self.proj = c["entry"] != "dense"
        self.r1, self.r2 = factors_of(c) if factors is None else factors
        self.plan = plan_of(c, self.r2) if c["entry"] == "planned" else None
        after = ROWS_AFTER if pitch <= 1024 else 2
        self.buf, self.v = {}, {}

        def add(name, rows, width, p, dtype, nan, fill=None, rows_after=ROWS_AFTER):
            self.buf[name], self.v[name] = _arena(rows, width, p, dtype, nan, fill, rows_after)

        add("x", M, D, pitch, np.float32, True, o["x"], after)
        for k, w in (("gam", D), ("bet", D), ("b1", Hd), ("b2", D), ("bp", D), ("gn", D), ("bn", D)):
            add(k, 1, w, w, np.float32, True, o[k])
        add("W1", Hd, D, D, np.uint16, True, to_bits(o["W1"]))
        add("W2", D, Hd, Hd, np.uint16, True, to_bits(o["W2"]))
        if self.proj:
            add("Wp", D, D, D, np.uint16, True, to_bits(o["Wp"]))
            ao = o["ao32"]
            if c["ao_scaled"]:                      # as the attention launch leaves it: rs1 applied before the rounding
                ao = self.rows(self.r1)[:, None] * ao
            self.ao = bf16_round(ao)
            add("ao", M, D, pitch, np.uint16, True, to_bits(self.ao), after)
            for k, r in (("r1", self.r1), ("r2", self.r2)):
                if r is not None:
                    add(k, 1, len(r), len(r), np.float32, True, r)
            if self.plan is not None:
                add("plan", 1, len(self.plan), len(self.plan), np.int32, True, self.plan)
        elif self.r2 is not None:
            add("r2", 1, len(self.r2), len(self.r2), np.float32, True, self.r2)
        self.outputs = ["xo"]
        if inplace:
            self.buf["xo"], self.v["xo"] = self.buf["x"], self.v["x"]
        else:
            add("xo", M, D, pitch, np.float32, False, None, after)
        if c["ln"]:
            add("ln", M, D, D, np.uint16, False)
            self.outputs.append("ln")
        if c["save"]:
            S = c["save"]
            add("s_ln2", S, D, D, np.uint16, False)
            add("s_pre", S, Hd, Hd, np.uint16, False)
            add("s_h", S, Hd, Hd, np.uint16, False)
            add("s_mean", 1, S, S, np.float32, False)
            add("s_rstd", 1, S, S, np.float32, False)
            self.outputs += ["s_ln2", "s_pre", "s_h", "s_mean", "s_rstd"]
        self.init = {k: self.buf[k].copy() for k in self.outputs}

    def rows(self, r, early=False):
        """[M] float32: the factor of every row (1 where the launch has none); early: looked up one row early (a planted fault)"""
        M, rps = self.c["M"], self.c["rps"]
        if r is None:
            return np.ones(M, np.float32)
        m = np.arange(M) + (1 if early else 0)
        return r[np.minimum(m // rps, len(r) - 1)]

    def vrow(self):
        """[M]: the virtual row of the launch that computes each physical row (the identity without a plan)"""
        M, N = self.c["M"], self.c["rps"]
        if self.plan is None:
            return np.arange(M)
        v = np.arange(M)
        pm = self.plan[1 + v // N].astype(np.int64) * N + v % N
        out = np.empty(M, np.int64)
        out[pm] = v
        return out

    def light(self):
        """[M] bool: physical rows computed by a light tile of a planned launch (they stop after the projection)"""
        if self.plan is None:
            return np.zeros(self.c["M"], bool)
        return (self.vrow() // FBM) * FBM >= int(self.plan[0]) * self.c["rps"]

    def got(self, name):
        """the logical output block as float (bf16 bits widened)"""
        a = self.v[name]
        return from_bits(a) if a.dtype == np.uint16 else a

    def pad_touched(self):
        """(buffer, element offsets) of output padding that no longer holds what was there before the launch"""
        bad = []
        for k in self.outputs:
            now = self.buf[k].copy()
            rows, width = self.v[k].shape
            p = self.v[k].strides[0] // now.itemsize
            blk = lambda b: np.lib.stride_tricks.as_strided(b[FRONT:], (rows, width), (p * b.itemsize, b.itemsize))     # noqa: E731
            blk(now)[...] = blk(self.init[k])
            d = np.flatnonzero(_bits(now) != _bits(self.init[k]))
            if len(d):
                bad.append((k, (d[:4] - FRONT).tolist(), len(d)))
        return bad


# ---- float64 expectation -------------------------------------------------------------------------------------------------------------------
def ln64(x):
    """(mean [M], rstd [M], xhat [M, D]) of float64 rows"""
    mu = x.mean(axis=1, keepdims=True)
    d = x - mu
    rstd = 1.0 / np.sqrt((d * d).mean(axis=1, keepdims=True) + EPS)
    return mu[:, 0], rstd[:, 0], d * rstd


def norm_term(x, xhat, rstd, g, b):
    """N of the module docstring: the size of one fp32 rounding of every operation of the normalisation, per element"""
    return U * (np.abs(xhat * g) + np.abs(b) + np.abs(g) * (rstd * np.abs(x).mean(axis=1))[:, None])


def ln_stage(x, g, b):
    """LayerNorm of fp32-exact rows x (float64) as the kernel owes it: (want, bound) of the bf16 output"""
    _, rstd, xhat = ln64(x)
    want = xhat * g + b
    t = C_NORM * norm_term(x, xhat, rstd, g, b)
    return want, t + half_ulp_bf16(np.abs(want) + t)


def flip_bf16(v, dv):
    """|bf16(w) - bf16(v)| for any w within dv of v (float64), rigorously: 0 where no rounding boundary lies within dv of v (both round to the
    same bf16 value), dv + a whole ulp elsewhere.  The boundaries of a binade [2^e, 2^(e+1)) are the odd multiples of hu; the nearest one below
    2^e is 2^e - hu / 2."""
    a = np.abs(v)
    hu = half_ulp_bf16(a)
    f = a / (2.0 * hu)
    near = (np.abs(f - np.floor(f) - 0.5) * 2.0 * hu <= dv) | (a - 255.5 * hu <= dv)
    return np.where(near, dv + 2.0 * half_ulp_bf16(a + dv), 0.0)


_E2E = {}


def expect_e2e(L):
    """dict(want, tol, exact [M] bool, x1, e1) of x_out, end to end (module docstring (2)); the last two cases stay cached: in-place and
    out-of-place launches, and a strided or planned launch and its dense twin, share one"""
    c = L.c
    key = (c["M"], c["Hd"], c["rps"], c["scale"], c["fac"], c["ao_scaled"], c.get("n_mlp"), L.proj)
    if key in _E2E:
        return _E2E[key]
    while len(_E2E) >= 2:
        _E2E.pop(next(iter(_E2E)))
    o = {k: v.astype(np.float64) for k, v in L.o.items()}
    x, W1, W2 = o["x"], o["W1"], o["W2"]
    r1, r2 = L.rows(L.r1).astype(np.float64)[:, None], L.rows(L.r2).astype(np.float64)[:, None]
    if L.proj:
        ao = L.ao
        if not c["ao_scaled"]:
            m = L.rows(L.r1) != 1.0
            ao = ao.copy()
            ao[m] = bf16_round(L.rows(L.r1)[m, None] * ao[m])            # fp32 product, then RNE: the kernel's own two roundings
        ao = ao.astype(np.float64)
        x1 = x + ao @ o["Wp"].T + r1 * o["bp"]
        e1 = C_ACC * U * (np.abs(ao) @ np.abs(o["Wp"]).T + np.abs(r1 * o["bp"]) + np.abs(x)) + 2.0 * U * np.abs(x1)
    else:
        x1, e1 = x, np.zeros_like(x)
    _, rstd, xhat = ln64(x1)
    g, b = o["gam"], o["bet"]
    xn = xhat * g + b
    rs = rstd[:, None]
    dln = rs * np.abs(g) * (e1 + e1.mean(axis=1, keepdims=True)) + np.abs(xhat * g) * rs * (np.abs(xhat) * e1).mean(axis=1, keepdims=True)
    dxn = dln + C_NORM * norm_term(x1, xhat, rstd, g, b)
    xnb = bf16_round64(xn)
    S1 = C_ACC * U * (np.abs(xnb) @ np.abs(W1).T + np.abs(o["b1"]))
    pre = xnb @ W1.T + o["b1"]
    ge = gelu_poly2_err(pre) if L.proj else GELU_E
    rh = r2 if L.proj else 1.0                       # proj: the factor rides on the GELU output before its rounding; dense: on the fp32 result
    ro = 1.0 if L.proj else r2
    h = rh * gelu64(pre)
    hb = bf16_round64(h)
    want = x1 + ro * (hb @ W2.T + rh * o["b2"])
    S2 = e1 + C_ACC * U * (np.abs(ro) * (np.abs(hb) @ np.abs(W2).T + np.abs(rh * o["b2"])) + np.abs(x1)) + 2.0 * U * np.abs(want)
    tol = None
    for rounding in (lambda v, dv: dv + half_ulp_bf16(np.abs(v) + dv), flip_bf16):        # (2), then (2') of the module docstring
        dpre = rounding(xn, dxn) @ np.abs(W1).T + S1
        dh = np.abs(rh) * (GELU_L * dpre + ge) + U * np.abs(h)
        t = S2 + np.abs(ro) * (rounding(h, dh) @ np.abs(W2).T)
        tol = t if tol is None else np.minimum(tol, t)
    light = L.light()
    if light.any():                                   # (planned == dense bit for bit says the same: rs2 = 0 rows are x1)
        assert not (r2[light] != 0).any()
    exact = (L.rows(L.r2) == 0) & ((L.rows(L.r1) == 0) if L.proj else True)
    _E2E[key] = dict(want=want, tol=tol, exact=exact)
    return _E2E[key]


# ---- the check -----------------------------------------------------------------------------------------------------------------------------
def _within(name, got, want, tol, ratios, key):
    """every element of got finite and within tol of want; records max |got - want| / tol under ratios[key]"""
    got, want, tol = (np.asarray(a).reshape(len(got), -1) for a in (got, want, tol))
    err = np.abs(got.astype(np.float64) - want)
    ok = err <= tol                                    # (NaN compares false)
    if not ok.all():
        over = np.where(np.isfinite(err), err - tol, np.inf)
        r, col = np.unravel_index(int(np.argmax(over)), over.shape)
        raise AssertionError("%s %s: worst element row %d (tile %d, wave %d, row %d of it) col %d (hidden chunk %d): got %.9g want %.9g |diff| %.3e "
                             "tol %.3e (%d of %d outside)" % (name, key, r, r // FBM, (r % FBM) // WAVE_ROWS, r % WAVE_ROWS, col, col // CH,
                                                              float(got[r, col]), float(want[r, col]), float(err[r, col]), float(tol[r, col]),
                                                              int((~ok).sum()), got.size))
    ratios[key] = max(ratios.get(key, 0.0), float((err / np.maximum(tol, 1e-300)).max()))


def verify(L):
    """Holds the outputs of the launch L (in its arenas) to the module docstring: padding untouched, every element finite and within its bound,
    stage by stage and end to end, exact where exactness is owed.  Returns {output: max |got - want| / bound}; raises AssertionError naming the
    worst element."""
    c, o = L.c, L.o
    name = c["id"] + ("-inplace" if L.inplace else "")
    touched = L.pad_touched()
    assert not touched, "%s: output padding overwritten: (buffer, element offsets from the first valid, count) %s" % (name, touched)
    ratios = {}
    xo = L.got("xo")
    e = expect_e2e(L)
    _within(name, xo, e["want"], e["tol"], ratios, "x_out")
    if e["exact"].any():
        bad = e["exact"][:, None] & (_bits(np.ascontiguousarray(xo)) != _bits(np.ascontiguousarray(o["x"])))
        if bad.any():
            r, col = np.argwhere(bad)[0]
            raise AssertionError("%s: row %d col %d has every factor 0 and must equal x = %.9g bit for bit, got %.9g (%d such elements)" % (
                name, r, col, float(o["x"][r, col]), float(xo[r, col]), int(bad.sum())))
    f64 = lambda k: o[k].astype(np.float64)            # noqa: E731
    if c["ln"]:
        want, tol = ln_stage(xo.astype(np.float64), f64("gn"), f64("bn"))
        _within(name, L.got("ln"), want, tol, ratios, "ln_next")
    S = c["save"]
    if S:
        x = f64("x")[:S]
        mu, rstd, xhat = ln64(x)
        _within(name, L.got("s_mean")[0], mu, C_STAT * U * np.abs(x).mean(axis=1), ratios, "s_mean")
        _within(name, L.got("s_rstd")[0], rstd, C_STAT * U * rstd, ratios, "s_rstd")
        want, tol = ln_stage(x, f64("gam"), f64("bet"))
        _within(name, L.got("s_ln2"), want, tol, ratios, "s_ln2")
        ln2, W1, W2 = L.got("s_ln2").astype(np.float64), f64("W1"), f64("W2")
        want = ln2 @ W1.T + f64("b1")
        t = C_ACC * U * (np.abs(ln2) @ np.abs(W1).T + np.abs(f64("b1")))
        _within(name, L.got("s_pre"), want, t + half_ulp_bf16(np.abs(want) + t), ratios, "s_pre")
        pre = L.got("s_pre").astype(np.float64)
        want = gelu64(pre)
        t = GELU_L * half_ulp_bf16(np.abs(pre)) + GELU_E
        _within(name, L.got("s_h"), want, t + half_ulp_bf16(np.abs(want) + t), ratios, "s_h")
        h = L.got("s_h").astype(np.float64)
        rs = L.rows(L.r2).astype(np.float64)[:S, None]
        want = x + rs * (h @ W2.T + f64("b2"))
        tol = C_ACC * U * (np.abs(rs) * (np.abs(h) @ np.abs(W2).T + np.abs(f64("b2"))) + np.abs(x)) + 2.0 * U * np.abs(want)
        _within(name, xo[:S], want, tol, ratios, "x_out(saved rows, from s_h)")
    return ratios


def same_bits(a, b, what):
    """the logical outputs of two launches agree bit for bit"""
    for k in a.outputs:
        ga, gb = np.ascontiguousarray(a.v[k]), np.ascontiguousarray(b.v[k])
        d = np.argwhere(_bits(ga) != _bits(gb))
        assert len(d) == 0, "%s: %s differs at %s: %r vs %r (%d elements)" % (what, k, d[0].tolist(), a.got(k)[tuple(d[0])], b.got(k)[tuple(d[0])], len(d))


# ---- float32 restatement -------------------------------------------------------------------------------------------------------------------
def ln32(x, g, b, layout, reverse=False):
    """LayerNorm in float32 in a kernel's order -> (mean, rstd, normalised rows before the bf16 rounding).  layout 'frag' (srhip_mlp_fused: lane
    group lg holds columns 32 k + 8 lg .. + 7, 24 quads summed per lane, then the two __shfl_xor steps) or 'acc' (the proj forms, from the
    accumulators: lane group lg holds columns 16 t + 4 lg + r, then rows_sum4); reverse: the per-lane sums taken last to first."""
    M = x.shape[0]
    if layout == "frag":
        q = x.reshape(M, 12, 4, 2, 4).transpose(0, 2, 1, 3, 4).reshape(M, 4, 24, 4)
    else:
        q = x.reshape(M, 24, 4, 4).transpose(0, 2, 1, 3)
    order = range(23, -1, -1) if reverse else range(24)
    s = np.zeros((M, 4), np.float32)
    for i in order:
        s += (q[:, :, i, 0] + q[:, :, i, 1]) + (q[:, :, i, 2] + q[:, :, i, 3])
    mu = ((s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])) * np.float32(1.0 / D)
    qq = np.zeros((M, 4), np.float32)
    for i in order:
        for e in (range(3, -1, -1) if reverse else range(4)):
            d = q[:, :, i, e] - mu[:, None]
            qq += d * d
    var = ((qq[:, 0] + qq[:, 1]) + (qq[:, 2] + qq[:, 3])) * np.float32(1.0 / D) + np.float32(EPS)
    rs = (np.float32(1.0) / np.sqrt(var)).astype(np.float32)
    return mu, rs, (x - mu[:, None]) * rs[:, None] * g + b


def acc32(acc, A, W, reverse=False):
    """acc + A W^T accumulated in float32 over 32-wide k-steps, first to last (the kernels' order) or last to first"""
    ks = range(0, A.shape[1], 32)
    for k in (reversed(ks) if reverse else ks):
        acc = acc + A[:, k:k + 32] @ W[:, k:k + 32].T
    return acc


def gelu_erf32(x):
    """csrc/common.h gelu_erf in float32"""
    w = np.abs(x) * np.float32(0.8493218)
    t = np.float32(1.0) / (np.float32(0.27273747) * w + np.float32(1.0))
    c = [np.float32(v) for v in (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)]
    poly = t * (c[0] + t * (c[1] + t * (c[2] + t * (c[3] + t * c[4]))))
    r = np.float32(1.0) - poly * np.exp2(-(w * w))
    h = np.float32(0.5) * x
    return (np.abs(h) * r + h).astype(np.float32)


def gelu_poly2_32(x):
    """csrc/common.h gelu_poly2 in float32 (each fused multiply-add rounded once: the products are exact in float64)"""
    xs = np.float32(4.252893)
    xc = np.clip(x, -xs, xs).astype(np.float64)
    t = (xc * xc).astype(np.float32).astype(np.float64)
    p = np.float64(np.float32(5.564872638e-11))
    for cf in (-5.327768675e-09, 2.255431416e-07, -5.626433893e-06, 9.341875929e-05, -1.108561217e-03, 9.815971766e-03, -6.634449185e-02,
               3.989023390e-01):
        p = (p * t + np.float64(np.float32(cf))).astype(np.float32).astype(np.float64)
    phi = (p * xc + 0.5).astype(np.float32)
    return (x * phi).astype(np.float32)


FAULTS = ("chunk_dropped", "b1_of_next_chunk", "b2_unscaled", "bp_unscaled", "factor_one_row_early", "stale_ring_slot", "permlane_pairing",
          "save_rows_off_by_one", "s_pre_holds_gelu", "light_tile_adds_b2", "plan_on_x_not_ao", "ln_next_at_virtual_row", "clamped_row_stored_twice", "xn_truncated_in_one_wave")
# ln_next addressed with the row pitch: srhip_mlp_fused_proj_strided refuses ln_next unless the pitch is D (the GPU test holds it to that), and
# every other launch has pitch D, so the two addressings are the same addresses in every launch the library accepts.
# gelu_erf instead of gelu_poly2 (or the reverse) before the bf16 rounding: the two differ by at most max(7e-5, 5e-6 |x|), which IS the GELU
# term of the end-to-end bound, and the saved s_h of the dense form is held to GELU_E = 1e-6 < 7e-5 only where half a bf16 ulp of the output
# (>= 2^-9 |h|) does not already cover 7e-5, i.e. for |h| < 0.036: gelu_poly2 there would show, gelu_erf in the proj forms cannot.
UNDETECTABLE = ("ln_next_addressed_with_the_row_pitch", "gelu_erf_in_the_proj_forms")


_APPLIES = {}


def fault_applies(fault, c, L=None):
    """whether the planted fault changes anything in the case"""
    if L is None and c["id"] in _APPLIES:
        return _APPLIES[c["id"]][fault]
    L = Launch(c) if L is None else L
    planned, proj = c["entry"] == "planned", c["entry"] != "dense"
    ns = 0 if L.r2 is None else len(L.r2)
    moved = planned and not np.array_equal(L.plan[1:], np.arange(c["B"]))
    live = bool((~L.light() & (L.rows(L.r2) != 0)).any())                  # some row's MLP branch is computed and counts
    table = {"chunk_dropped": live, "b1_of_next_chunk": live,
            "b2_unscaled": bool((L.rows(L.r2)[~L.light()] != 1).any()), "bp_unscaled": proj and bool((L.rows(L.r1) != 1).any()),
            "factor_one_row_early": ns >= 2 and not planned,
            "stale_ring_slot": c["M"] > GRID * FBM and not L.light()[L.vrow() >= GRID * FBM].all(),
            "permlane_pairing": proj,
            "save_rows_off_by_one": c["save"] > 0, "s_pre_holds_gelu": c["save"] > 0,
            "light_tile_adds_b2": bool(L.light().any()),
            "plan_on_x_not_ao": moved, "ln_next_at_virtual_row": moved,
            "clamped_row_stored_twice": c["M"] % FBM != 0,
            # (dense only: in the proj forms the gelu_poly2 term of the bound, 7e-5 per hidden unit, is the size of this fault's effect where no
            # factor and a narrow hidden layer keep everything else small -- proj-1x128, proj-127x256 and strided-1x128 let it pass)
            "xn_truncated_in_one_wave": live and not proj}
    _APPLIES[c["id"]] = table
    return table[fault]


def restate(L, fault=None, reverse=False):
    """The launch in float32 on the host, in the order of mlp_fused_body.h with its rounding points, written into L's arenas as the kernel
    would.  fault: one of FAULTS, planted."""
    assert fault is None or fault in FAULTS
    c, o = L.c, L.o
    M, Hd, N = c["M"], c["Hd"], c["rps"]
    x, W1, W2, b1, b2 = o["x"], o["W1"], o["W2"], o["b1"], o["b2"]
    early = fault == "factor_one_row_early"
    r1, r2 = L.rows(L.r1, early)[:, None], L.rows(L.r2, early)[:, None]
    vrow, light = L.vrow(), L.light()
    if L.proj:
        ao = L.ao
        if fault == "plan_on_x_not_ao":                # the physical row's computation reads ao at its virtual row
            ao = ao[vrow]
        if not c["ao_scaled"]:
            m = r1[:, 0] != 1.0
            ao = ao.copy()
            ao[m] = bf16_round(r1[m] * ao[m])
        x1 = acc32(x + (o["bp"] if fault == "bp_unscaled" else r1 * o["bp"]), ao, o["Wp"], reverse)
        _, _, xn = ln32(x1, o["gam"], o["bet"], "acc", reverse)
        acc = x1 + (b2 if fault == "b2_unscaled" else r2 * b2)
    else:
        mu, rs, xn = ln32(x, o["gam"], o["bet"], "frag", reverse)
        acc = np.zeros((M, D), np.float32)
    xn32, xn = xn, bf16_round(xn)
    if fault == "xn_truncated_in_one_wave":            # the normalised rows of one wave cut off to bf16 instead of rounded to nearest even
        w = (vrow // WAVE_ROWS) == int(vrow[np.flatnonzero(~light & (r2[:, 0] != 0))[0]]) // WAVE_ROWS
        xn[w] = (np.ascontiguousarray(xn32[w]).view(np.uint32) & 0xFFFF0000).view(np.float32)
    if fault == "permlane_pairing":                    # columns 8 g .. + 3 and 8 g + 4 .. + 7 of k-step 0 exchanged
        xn[:, :32] = xn[:, :32].reshape(M, 4, 2, 4)[:, :, ::-1].reshape(M, 32)
    b1u = b1
    if fault == "b1_of_next_chunk":
        b1u = b1.copy()
        b1u[:CH] = b1[CH:2 * CH]
    pre = acc32(np.broadcast_to(b1u, (M, Hd)), xn, W1, reverse)
    if fault == "stale_ring_slot":                     # chunk 0 of W1 is still the last chunk's, in a workgroup's second tile
        t2 = vrow >= GRID * FBM
        pre[t2, :CH] = acc32(np.broadcast_to(b1[:CH], (int(t2.sum()), CH)), xn[t2], W1[Hd - CH:], reverse)
    if L.proj:
        h = bf16_round(gelu_poly2_32(pre) * r2)
    else:
        h = bf16_round(gelu_erf32(pre))
    hm = h
    if fault == "chunk_dropped":                       # the last hidden chunk, for the wave of the first heavy row
        v0 = int(vrow[np.flatnonzero(~light & (r2[:, 0] != 0))[0]])          # ... whose GELU output is not multiplied by zero
        w = (vrow // WAVE_ROWS) == v0 // WAVE_ROWS
        hm = h.copy()
        hm[w, Hd - CH:] = 0.0
    acc = acc32(acc, hm, W2, reverse)
    if L.proj:
        out = acc
        out[light] = (x1 + b2)[light] if fault == "light_tile_adds_b2" else x1[light]
    elif fault == "b2_unscaled":
        out = x + (r2 * acc + b2)
    else:
        out = x + r2 * (acc + b2)
    L.v["xo"][...] = out
    if fault == "clamped_row_stored_twice":            # rows M .. of the last tile exist for the kernel: it computes row M - 1 in their place
        extra = min(FBM - M % FBM, (len(L.buf["xo"]) - FRONT) // c["pitch"] - M)
        np.lib.stride_tricks.as_strided(L.buf["xo"][FRONT + M * c["pitch"]:], (extra, D), (c["pitch"] * 4, 4))[...] = out[M - 1]
    if c["ln"]:
        _, _, y = ln32(out, o["gn"], o["bn"], "acc", reverse)
        y = bf16_round(y)
        if fault == "permlane_pairing":
            y[:, :32] = y[:, :32].reshape(M, 4, 2, 4)[:, :, ::-1].reshape(M, 32)
        if fault == "ln_next_at_virtual_row":
            L.v["ln"][vrow] = to_bits(y)
        else:
            L.v["ln"][...] = to_bits(y)
    S = c["save"]
    if S:
        rows = np.arange(S)
        if fault == "save_rows_off_by_one":
            rows = np.concatenate([rows[:-1], [S]])    # (row S of the buffers is padding: ROWS_AFTER rows follow the last saved one)
        wide = lambda k, w: np.lib.stride_tricks.as_strided(L.buf[k][FRONT:], (S + 1, w), (w * 2, 2))     # noqa: E731
        src = np.minimum(rows, M - 1)
        wide("s_ln2", D)[rows] = to_bits(xn[src])
        wide("s_pre", Hd)[rows] = to_bits(h[src] if fault == "s_pre_holds_gelu" else bf16_round(pre[src]))
        wide("s_h", Hd)[rows] = to_bits(h[src])
        L.buf["s_mean"][FRONT + rows] = mu[src]
        L.buf["s_rstd"][FRONT + rows] = rs[src]
    return L


# ---- the two measured constants ------------------------------------------------------------------------------------------------------------
def measure_constants(cases=CASES):
    """(C_STAT, C_NORM) measurements: the float32 LayerNorm restatement (both layouts, both orders, no bf16 rounding) against float64, over
    the x of every distinct shape of the cases"""
    c_stat = c_norm = 0.0
    for M, Hd in sorted({(c["M"], c["Hd"]) for c in cases}):
        o = operands(M, Hd)
        x64 = o["x"].astype(np.float64)
        mu, rstd, xhat = ln64(x64)
        g, b = o["gam"].astype(np.float64), o["bet"].astype(np.float64)
        want, nt = xhat * g + b, norm_term(x64, xhat, rstd, g, b)
        for layout in ("frag", "acc"):
            for rev in (False, True):
                m32, r32, y32 = ln32(o["x"], o["gam"], o["bet"], layout, rev)
                c_stat = max(c_stat, float((np.abs(m32 - mu) / (U * np.abs(x64).mean(axis=1))).max()), float((np.abs(r32 - rstd) / (U * rstd)).max()))
                c_norm = max(c_norm, float((np.abs(y32 - want) / nt).max()))
    return c_stat, c_norm


# ---- the device ----------------------------------------------------------------------------------------------------------------------------
def upload(L, dev="cuda:0"):
    """L's buffers on the device -> (tensors by name, p(name) = the 1-d tensor that starts at the first valid element, or None)"""
    t = {}
    for k, b in L.buf.items():
        if not (k == "xo" and L.inplace):
            t[k] = torch.from_numpy(b.view(np.int16) if b.dtype == np.uint16 else b).to(dev)
    if L.inplace:
        t["xo"] = t["x"]

    def p(k):
        if k not in t:
            return None
        a = t[k][FRONT:]
        return a.view(torch.bfloat16) if a.dtype == torch.int16 else a
    return t, p


def download(L, t):
    """the output buffers back into L"""
    torch.cuda.synchronize()
    for k in L.outputs:
        L.buf[k][...] = t[k].cpu().numpy().view(L.buf[k].dtype)
    return L


def run_gpu(L, dev="cuda:0"):
    """Uploads L's buffers, launches its entry point through semireward_amd.ops (an ordinary launch), and brings the outputs back into L.
    A 'kernel' plan is built on the device by ops.vit_droppath_plan from the factors and must equal plan_of()."""
    from semireward_amd import ops
    c = L.c
    M, Hd = c["M"], c["Hd"]
    t, p = upload(L, dev)
    if c["entry"] == "dense":
        save = (c["save"], p("s_ln2"), p("s_pre"), p("s_h"), p("s_mean"), p("s_rstd")) if c["save"] else None
        ops.mlp_fused(p("x"), p("gam"), p("bet"), EPS, p("W1"), p("b1"), p("W2"), p("b2"), p("r2"), c["rps"], M, D, Hd, x_out=p("xo"), save=save)
    else:
        kw = {}
        if c["entry"] == "strided":
            kw["row_pitch"] = c["pitch"]
        if c["entry"] == "planned":
            if c["plan"] == "kernel":
                dp = torch.stack([p("r1")[:c["B"]], p("r2")[:c["B"]]])[None].contiguous()
                plan = torch.full((1, 1 + c["B"]), -1, dtype=torch.int32, device=dev)
                ops.vit_droppath_plan(dp, 1, c["B"], plan)
                assert np.array_equal(plan[0].cpu().numpy(), L.plan), "srhip_vit_droppath_plan is not the stable partition"
                t["plan"][FRONT:FRONT + 1 + c["B"]] = plan[0]
            kw["plan_row"] = p("plan")
        ops.mlp_fused_proj(p("x"), p("ao"), p("Wp"), p("bp"), p("r1"), p("gam"), p("bet"), EPS, p("W1"), p("b1"), p("W2"), p("b2"), p("r2"),
                           c["rps"], M, D, Hd, x_out=p("xo"), ln_next=p("ln"), next_gamma=p("gn") if c["ln"] else None,
                           next_beta=p("bn") if c["ln"] else None, ao_scaled=c["ao_scaled"], **kw)
    return download(L, t)


# what the criteria of test_mlp_fused / test_mlp_fused_proj let pass at 10285 rows on their own inputs (test_cpu_mlp_fused_cases.py prints every
# figure): they catch each fault of the issue's list there -- what they cannot see is what they never launch (a second tile in three of the
# four kernels, Hd other than 1536, save_rows at an edge) and a fault of the size of the rounding itself on a few rows
NORM_BLIND = ("dense:xn_truncated_in_one_wave",)
