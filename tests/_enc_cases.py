"""The cases of tests/test_{cpu,gpu}_enc_cases.py: every kernel of csrc/enc_ops.hip (the post-LN encoder glue of the BERT, Wav2Vec2 and HuBERT steps)
and csrc/optim.hip (AdamW over the flat block, the clip_grad_norm_ coefficient) element by element against float64.  Nothing is stored: every
input is rebuilt from its seed (numpy PCG64, nothing from the GPU), every expected value is recomputed.  Importing this module launches nothing.

Why element by element: test_embed_postln_meanpool (tests/test_gpu_bert.py) holds enc_ops.hip to whole-tensor relative L2 norms (2e-6, 1e-5, 4e-3)
at one shape, and test_adamw_flat_matches_oracle (tests/test_gpu_kernels.py) reads p and pb after four steps of one form.  A norm over 73 000
elements cannot see one wrong row, column pair or partial workgroup; tests/test_cpu_enc_cases.py plants thirteen such faults in the float32
restatement, shows verify() rejecting each and states what the old tests would have read (NORM_BLIND below: the ones they let pass).

Every launch class below builds its inputs, owns its output buffers (class Out: every buffer sits between FRONT elements of PATTERN and is
allocated larger than what the kernel may write -- rows >= M, table rows no id names, the gaps of an offsets chunk table, the partial copies no
workgroup maps to -- and all of that must come back bit for bit), states the float64 reference from the exact fp32 inputs (expect), launches
through semireward_amd.ops (run_hip) or writes a float32 numpy restatement into the same buffers (restate), and holds what is there to the
reference (verify -> headroom max |got - want| / tol per output).  Accumulating outputs start from non-zero contents that the reference adds.

Bounds.  tol = C * base + extra per element, never a norm, never dependent on the order of a sum (the column sums go through atomics):
  * a sum: base = 2^-24 sum |terms| (contents before the launch included);
  * LayerNorm forward, row v of mean mu, variance var, rs = 1 / sqrt(var + eps), xh = (v - mu) rs, o = gamma xh + beta, A = mean |v|:
        base(o) = 2^-24 (|gamma| (rs A + |xh|) + |o|),   extra(o) = |gamma xh| (E^2 / (2 (var + eps)) + RSQRT_ULP 2^-23),   E = C_LN 2^-24 A.
    rs A >= |mu| rs is the conditioning term: the error of the mean, at most E, moves every element of the row by rs E.  It is what lets the
    rows of mean 300 be judged by the same constant as the unit rows.  E^2 is the second-order effect of the same error on the variance.
    mean: C_LN 2^-24 A.  rstd: rs (C_LN 2^-24 + E^2 / (2 (var + eps)) + RSQRT_ULP 2^-23).  The embedding sums three fp32 rows first: S = |word| +
    |pos| + |type| joins A, and rs S the per-element terms.
  * LayerNorm backward (mean and rstd are INPUTS: the fp32 roundings of the float64 statistics), dh = dy gamma, c1 = mean dh, c2 = mean dh xh,
    dx = rs (dh - c1 - xh c2):  base(dx) = 2^-24 rs (|dh| + mean |dh| + |xh| mean |dh xh|)   (+ the S terms of the embedding).
  * a bf16 output adds half a bf16 ulp at |want| + tol; a kept dropout element one rounding of the product with the scale.
  * GELU: 0.5 v (1 + erf(t)), t = v / sqrt 2: base = 2^-24 (|0.5 v| (1 + |erf| + |t| erf'(t)) + |want|), extra = |0.5 v| ERF_ULP 2^-23 |erf|; the
    derivative adds the density term |v phi| (1 + v^2 / 2) and EXP_ULP 2^-23 |v phi|.
  * AdamW: p: 2^-24 (2 |p decay| + |p'|) (the product, one ulp of a decay formed with or without contraction, the difference) + C_ADAM 2^-24 U, U = step (|b1 m| + |(1 - b1) g|) / denom >= |update|; m, v: 2^-24 |result| + C_ADAM 2^-24
    sum |terms|.  lr lr_factor, decay, step, the bias corrections (ops.adam_bias_corrections) and grad_scale clip enter the float64 formula as the
    fp32 values the kernel forms.
The constants C_* are measured: the worst error of the float32 restatement against float64 in units of base, over every case and two summation
orders (row sums: the kernels' own tree and neighbours pairwise; sums over rows, workgroups and atomics: first to last and last to first), times 8 -- the margin the GEMM, attention and WideResNet tests give the GPU's different
reduction tree.  They are never set from what a kernel produced.  The intrinsic allowances (ERF_ULP, EXP_ULP, RSQRT_ULP) are 8 times the worst
error in ulps of torch's float32 erf, exp and rsqrt against float64 over the case inputs (measure_intrinsics): no document on the ROCm
installation states an accuracy for erff, expf or rsqrtf.

Held to bits: dropped elements (0.0), dword[pad_id], the filler rows of meanpool_bwd, mask_lengths, dropout_cast (bf16 RNE of fl32(x scale)), pb
(bf16 RNE of the p the launch wrote), the EMA (three separately rounded fp32 operations on the launch's own p, 1 - m rounded from double),
coef_out[0] from the launch's own coef_out[1], g after either zero_grad, the frozen tensor's p and pb, dyn against by-value, dx aliasing dy
against out of place, a constant LayerNorm row (the output is beta)."""
import itertools
import math

import numpy as np
import torch

from _attn_cases import PATTERN, half_ulp_bf16
from _wrn_cases import _rng, bits, to_bf16, worst
from oracle import bert_ref as BR
from semireward_amd import ops
from semireward_amd.optim import build_chunk_table

# measured by measure_constants() / measure_intrinsics() (tests/test_cpu_enc_cases.py holds each between 4 and 16 times its fresh measurement)
C_LN_MEASURED, C_LNB_MEASURED, C_COL_MEASURED, C_POOL_MEASURED = 2.413, 2.684, 3.170, 2.995
C_GELU_MEASURED, C_ADAM_MEASURED, C_NORM_MEASURED = 1.127, 1.275, 2.788
ERF_ULP_MEASURED, EXP_ULP_MEASURED, RSQRT_ULP_MEASURED = 0.935, 0.552, 1.287
NAMES = ("C_LN", "C_LNB", "C_COL", "C_POOL", "C_GELU", "C_ADAM", "C_NORM", "ERF_ULP", "EXP_ULP", "RSQRT_ULP")
C_LN, C_LNB, C_COL, C_POOL, C_GELU, C_ADAM, C_NORM, ERF_ULP, EXP_ULP, RSQRT_ULP = (
    8.0 * v for v in (C_LN_MEASURED, C_LNB_MEASURED, C_COL_MEASURED, C_POOL_MEASURED, C_GELU_MEASURED, C_ADAM_MEASURED, C_NORM_MEASURED,
                      ERF_ULP_MEASURED, EXP_ULP_MEASURED, RSQRT_ULP_MEASURED))

FRONT = 64                          # elements of PATTERN before and after every output buffer
U24, U23 = 2.0 ** -24, 2.0 ** -23
SEED = (7 << 32) + 11               # the 64-bit call seed of every dropout site here
LN_REP = 16                         # partial copies nets/encoder.py asks of postln_bwd_part
CLIP_WG = 1024                      # the fixed partition of srhip_clip_grad_coef
F = np.float32
ORDERS = ("tree", "pair")        # row sums: the kernels' own tree / adjacent pairs; sums over rows, workgroups and atomics: first to last / last to first


def const(name):
    return globals()[name]


# ---- buffers ------------------------------------------------------------------------------------------------------------------------------------
def is_pattern(t):
    return bool((t.contiguous().view(torch.int16) == PATTERN).all())


class RowsView:
    """A [rows, L] window of a wider tensor handed to ops as it stands (ld = the base's row stride, last dimension dense), as ops.RawRows does for
    offsets: the argument check of ops wants contiguous tensors, the kernels take ld_ids / ld."""
    is_cuda = True

    def __init__(self, view):
        assert view.stride(1) == 1 and view.stride(0) > view.shape[1]
        self.view = view

    def data_ptr(self):
        return self.view.data_ptr()

    def stride(self, i):
        return self.view.stride(i)

    def is_contiguous(self):
        return True


class Out:
    """The output buffers of one launch: each between FRONT elements of PATTERN; init None: PATTERN inside as well."""

    def __init__(self, device):
        self.device, self.bufs = device, {}

    def new(self, name, shape, dtype=torch.float32, init=None):
        n = int(np.prod(shape))
        buf = torch.empty(n + 2 * FRONT, dtype=dtype, device=self.device)
        buf.view(torch.int16).fill_(PATTERN)
        v = buf[FRONT:FRONT + n].view(shape)
        if init is not None:
            v.copy_(torch.as_tensor(init).to(dtype))
        assert v.data_ptr() % 16 == 0
        self.bufs[name] = (buf, n)
        return v

    def check(self, cid):
        for name, (buf, n) in self.bufs.items():
            assert is_pattern(buf[:FRONT]) and is_pattern(buf[FRONT + n:]), "%s: the surroundings of %s were overwritten" % (cid, name)


def put(view, a):
    view.copy_(torch.as_tensor(np.ascontiguousarray(a)).to(view.dtype).view(view.shape))


def npy(t):
    t = t.detach().cpu()
    return (t.float() if t.dtype == torch.bfloat16 else t).numpy().copy()


def same_bits(what, got, want):
    got, want = torch.as_tensor(got).cpu().contiguous(), torch.as_tensor(want).cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    ne = bits(got) != bits(want)
    assert not bool(ne.any()), "%s: %d of %d elements differ in bits, first at %s" % (what, int(ne.sum()), ne.numel(), tuple(int(i) for i in ne.nonzero()[0]))


def judge(cid, entries, got):
    """entries: output -> (want, constant name, base, extra); every element of got[output] within C base + extra -> headroom per output"""
    return {k: worst("%s %s" % (cid, k), got[k], want, const(cn) * base + extra) for k, (want, cn, base, extra) in entries.items()}


def ratios(entries, got):
    """constant name -> the largest (|got - want| - extra) / base: what measure_constants() takes the worst of"""
    R = {}
    for k, (want, cn, base, extra) in entries.items():
        err = np.maximum(np.abs(np.asarray(got[k], dtype=np.float64) - want) - extra, 0.0)
        nz = np.broadcast_to(base, err.shape) > 0
        if nz.any():
            R[cn] = max(R.get(cn, 0.0), float((err[nz] / np.broadcast_to(base, err.shape)[nz]).max()))
    return R


def keep_of(site, shape, p):
    """(boolean keep mask of oracle.bert_ref, ops.Drop, fp32 scale) of one site; p = 0: (ones, None, 1)"""
    if not p:
        return np.ones(shape, dtype=bool), None, F(1.0)
    return BR.keep_mask(SEED, site, tuple(shape), p), ops.Drop(SEED, site, p), F(1.0 / (1.0 - p))


# ---- float32 sums in two orders ---------------------------------------------------------------------------------------------------------------------
def rowsum32(v, order):
    """sum over the last axis (D = 128 NV) of float32 v [M, D]: 'tree' = a lane's NV float2 in turn, then the xor butterfly of wave_sum over the
    64 lanes; 'pair' = neighbours added pairwise, level by level"""
    v = np.ascontiguousarray(v, dtype=F)
    if order == "pair":
        return pairsum32(v)
    M, D = v.shape
    ln = v.reshape(M, D // 128, 64, 2)
    s = np.zeros((M, 64), dtype=F)
    for i in range(D // 128):
        s = s + (ln[:, i, :, 0] + ln[:, i, :, 1])
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ o]
    return s[:, 0]


def pairsum32(v):
    """sum over the last axis of float32 v, neighbours added pairwise level by level (zero padding to a power of two)"""
    n = 1 << max(int(v.shape[-1]) - 1, 0).bit_length()
    t = np.zeros(v.shape[:-1] + (n,), dtype=F)
    t[..., :v.shape[-1]] = v
    while t.shape[-1] > 1:
        t = (t[..., 0::2] + t[..., 1::2]).astype(F)
    return t[..., 0]


def colsum32(terms, rows_per_block, order):
    """[M, D] float32 -> [blocks, D]: the rows of a workgroup added in turn (first to last, or last to first)"""
    M, D = terms.shape
    nb = -(-M // rows_per_block)
    t = np.zeros((nb * rows_per_block, D), dtype=F)
    t[:M] = terms
    t = t.reshape(nb, rows_per_block, D)
    if order == "pair":
        t = t[:, ::-1]
    return np.cumsum(t, axis=1, dtype=F)[:, -1]


def fold32(acc, blocks, order):
    """acc [D] += the block sums, in turn"""
    acc = acc.astype(F).copy()
    for b in (reversed(range(len(blocks))) if order == "pair" else range(len(blocks))):
        acc = (acc + blocks[b]).astype(F)
    return acc


# ---- LayerNorm: float64 reference with its bound, float32 restatement ---------------------------------------------------------------------------
def ln_fwd_ref(v, S_in, A_terms, g, b, eps):
    """v [M, D] float64 (the exact row), S_in [M, D] (sum of |terms| of an element that was itself summed in fp32; 0: v is an input), A_terms
    [M, D] (|terms| of the row's mean) -> dict of float64 (o, mu, rs, var, xh) and the base / extra of o, mu, rs"""
    mu = v.mean(1)
    var = ((v - mu[:, None]) ** 2).mean(1)
    rs = 1.0 / np.sqrt(var + eps)
    xh = (v - mu[:, None]) * rs[:, None]
    o = xh * g + b
    A, Sm = A_terms.mean(1), S_in.mean(1)
    E = C_LN * U24 * A
    second = 0.5 * E * E / (var + eps) + RSQRT_ULP * U23
    ag = np.abs(g)
    base_o = U24 * (ag * (rs[:, None] * (A[:, None] + S_in) + np.abs(xh) * (1.0 + (rs * Sm)[:, None])) + np.abs(o))
    return dict(o=o, mu=mu, rs=rs, var=var, xh=xh, base_o=base_o, extra_o=np.abs(g * xh) * second[:, None], base_mu=U24 * A, base_rs=U24 * rs * (1.0 + rs * Sm),
                extra_rs=rs * second)


def ln_fwd32(v, g, b, eps, order, one_pass=False):
    """the forward kernels' arithmetic in float32: (o, mu, rs)"""
    D = v.shape[1]
    inv = F(1.0) / F(D)
    mu = (rowsum32(v, order) * inv).astype(F)
    d = (v - mu[:, None]).astype(F)
    if one_pass:                                         # planted: E[x^2] - mu^2
        var = ((rowsum32((v * v).astype(F), order) * inv).astype(F) - (mu * mu).astype(F)).astype(F)
    else:
        var = (rowsum32((d * d).astype(F), order) * inv).astype(F)
    rs = (F(1.0) / np.sqrt((var + F(eps)).astype(F))).astype(F)
    o = (((d * rs[:, None]).astype(F) * g).astype(F) + b).astype(F)
    return o, mu, rs


def ln_bwd_ref(d, xh, rs, g, S_x=None):
    """d [M, D] float64 (dy, masked and scaled where a dropout sits in front), xh float64 from the fp32 mean / rstd the kernel reads, S_x: the
    absolute error unit of xh beyond its own rounding (embedding: rs S) -> dx float64 and its base"""
    dh = d * g
    c1, c2 = dh.mean(1), (dh * xh).mean(1)
    dx = rs[:, None] * (dh - c1[:, None] - xh * c2[:, None])
    T = np.abs(dh) + np.abs(dh).mean(1)[:, None] + np.abs(xh) * np.abs(dh * xh).mean(1)[:, None]
    if S_x is not None:
        T = T + S_x * np.abs(c2)[:, None] + np.abs(xh) * (np.abs(dh) * S_x).mean(1)[:, None]
    return dx, U24 * rs[:, None] * T


def ln_bwd32(d, xh, rs, g, order):
    dh = (d * g).astype(F)
    inv = F(1.0) / F(d.shape[1])
    c1 = (rowsum32(dh, order) * inv).astype(F)
    c2 = (rowsum32((dh * xh).astype(F), order) * inv).astype(F)
    return (rs[:, None] * ((dh - c1[:, None]).astype(F) - (xh * c2[:, None]).astype(F)).astype(F)).astype(F)


def drop_entry(want, base, extra, keep, scale):
    """the (want, base, extra) of an output behind a dropout: kept elements times the fp32 scale (one more rounding), dropped ones exactly 0"""
    s = float(scale)
    w = np.where(keep, want * s, 0.0)
    base = np.where(keep, base * s + (U24 * np.abs(want * s) if s != 1.0 else 0.0), 0.0)
    return w, base, np.where(keep, extra * s, 0.0)


# ---- embed_ln_fwd / embed_ln_bwd ------------------------------------------------------------------------------------------------------------------
SITE_EMB, SITE_LN, SITE_POOL, SITE_CAST = 1, 6, 3, 9
V_WORDS, PAD_ID, POS_EXTRA, IDS_PAD = 11, 3, 4, 5


def _embed_cases():
    out = []
    for D, (B, L), (gather, p) in itertools.product((128, 384, 768), ((1, 1), (3, 23), (2, 33)), ((False, 0.0), (True, 0.1), (False, 0.1), (True, 0.0))):
        out.append(dict(id="emb-d%d-b%dl%d-%s-p%g" % (D, B, L, "gather" if gather else "plain", p), D=D, B=B, L=L, gather=gather, p=p,
                        kernel="embed_ln_fwd_kernel<%d> embed_ln_bwd_kernel<%d>" % (D // 128, D // 128), seed=len(out)))
    return tuple(out)


EMBED_CASES = _embed_cases()
OLD_EMBED = dict(id="old-embed-shape", D=128, B=5, L=19, gather=True, p=0.1, kernel="", seed=900, old=True)     # test_embed_postln_meanpool's shape


class EmbedLaunch:
    def __init__(self, c, device):
        self.c, self.device = c, device
        D, B, L = c["D"], c["B"], c["L"]
        rng = _rng(c["seed"], 0xE1)
        S = 3 if c.get("old") else (max(B - 1, 1) if c["gather"] else B)
        self.idx = (np.array([2, 0, 1, 1, 2]) if c.get("old") else np.arange(B)[::-1] % S).astype(np.int32) if c["gather"] else None
        base = rng.integers(0, V_WORDS - 2, size=(S, L + IDS_PAD), dtype=np.int64)             # (the last two table rows: named by no id)
        base[:, 2 + L - min(3, L - 1 if L > 1 else 0):] = PAD_ID                                 # [PAD] at the end of every sequence
        if L > 8:
            base[0, 2 + 4] = PAD_ID
        base[:, :2] = -(2 ** 40)
        base[:, 2 + L:] = -(2 ** 40)                                                             # (outside the window: an id that would fault)
        self.ids_base, self.ids = base, base[:, 2:2 + L]
        self.word = (0.5 * rng.standard_normal((V_WORDS, D))).astype(F)
        self.pos = (0.5 * rng.standard_normal((L + POS_EXTRA, D))).astype(F)
        self.typ = (0.5 * rng.standard_normal((2, D))).astype(F)
        self.g = (1.0 + 0.1 * rng.standard_normal(D)).astype(F)
        self.b = (0.1 * rng.standard_normal(D)).astype(F)
        self.dy = rng.standard_normal((B * L, D)).astype(F)
        self.M, self.eps = B * L, 1e-12
        self.keep, self.drop, self.scale = keep_of(SITE_EMB, (self.M, D), c["p"])
        self.pre = dict(dword=rng.standard_normal((V_WORDS, D)).astype(F), dpos=rng.standard_normal((L + POS_EXTRA, D)).astype(F),
                        dtype0=rng.standard_normal(D).astype(F), dgamma=rng.standard_normal(D).astype(F), dbeta=rng.standard_normal(D).astype(F))
        self.pre["dword"][PAD_ID] = 0.0
        rows = self.ids[self.idx if self.idx is not None else np.arange(B)].reshape(-1)
        self.row_id, self.row_pos = rows, np.tile(np.arange(L), B)
        self.ex = self._expect()
        M = self.M
        O = self.O = Out(device)
        self.x, self.xb = O.new("x", (M + 2, D)), O.new("xb", (M + 2, D), torch.bfloat16)
        self.mean, self.rstd = O.new("mean", (M + 2,)), O.new("rstd", (M + 2,))
        self.acc = {k: O.new(k, v.shape, init=v) for k, v in self.pre.items()}

    def _expect(self):
        f8 = lambda a: a.astype(np.float64)   # noqa: E731
        w, ps, t = f8(self.word)[self.row_id], f8(self.pos)[self.row_pos], f8(self.typ[0])[None]
        v, S = w + ps + t, np.abs(w) + np.abs(ps) + np.abs(t)
        g, b = f8(self.g), f8(self.b)
        R = ln_fwd_ref(v, S, S, g, b, self.eps)
        ow, ob, oe = drop_entry(R["o"], R["base_o"], R["extra_o"], self.keep, self.scale)
        E = dict(x=(ow, "C_LN", ob, oe), xb=(ow, "C_LN", ob, oe + half_ulp_bf16(np.abs(ow) + C_LN * ob + oe)),
                 mean=(R["mu"], "C_LN", R["base_mu"], 0.0), rstd=(R["rs"], "C_LN", R["base_rs"], R["extra_rs"]))
        # backward: mean / rstd are inputs (fp32 roundings of the float64 statistics)
        self.mean_in, self.rstd_in = R["mu"].astype(F), R["rs"].astype(F)
        mu, rs = f8(self.mean_in), f8(self.rstd_in)
        xh = (v - mu[:, None]) * rs[:, None]
        d = np.where(self.keep, f8(self.dy) * float(self.scale), 0.0)
        Sx = rs[:, None] * S
        dx, bdx = ln_bwd_ref(d, xh, rs, g, Sx)
        self.dx64 = dx
        tdx = C_LNB * bdx
        V_, P_ = self.word.shape[0], self.pos.shape[0]

        def scatter(index, n, select=None):
            want, tl, ab = np.zeros((n, v.shape[1])), np.zeros((n, v.shape[1])), np.zeros((n, v.shape[1]))
            sel = np.ones(len(index), dtype=bool) if select is None else select
            np.add.at(want, index[sel], dx[sel])
            np.add.at(tl, index[sel], tdx[sel])
            np.add.at(ab, index[sel], np.abs(dx)[sel])
            return want, tl, ab
        for name, (want, tl, ab) in (("dword", scatter(self.row_id, V_, self.row_id != PAD_ID)), ("dpos", scatter(self.row_pos, P_)),
                                     ("dtype0", scatter(np.zeros(len(self.row_id), dtype=np.int64), 1))):
            pre = f8(self.pre[name]).reshape(want.shape)
            E[name] = ((want + pre).reshape(self.pre[name].shape), "C_COL", (U24 * (ab + np.abs(pre))).reshape(self.pre[name].shape), tl.reshape(self.pre[name].shape))
        E["dgamma"] = ((d * xh).sum(0) + f8(self.pre["dgamma"]), "C_COL", U24 * ((np.abs(d) * (np.abs(xh) + Sx)).sum(0) + np.abs(f8(self.pre["dgamma"]))), 0.0)
        E["dbeta"] = (d.sum(0) + f8(self.pre["dbeta"]), "C_COL", U24 * (np.abs(d).sum(0) + np.abs(f8(self.pre["dbeta"]))), 0.0)
        return E

    def _dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def run_hip(self):
        c, dv = self.c, self._dev
        base = dv(self.ids_base)
        ids = RowsView(base[:, 2:2 + c["L"]])
        idx = dv(self.idx) if self.idx is not None else None
        word, pos, typ, g, b = dv(self.word), dv(self.pos), dv(self.typ), dv(self.g), dv(self.b)
        ops.embed_ln_fwd(ids, idx, word, pos, typ, g, b, self.eps, self.x, self.xb, self.mean, self.rstd, c["B"], c["L"], c["D"], self.drop)
        A = self.acc
        ops.embed_ln_bwd(dv(self.dy), ids, idx, word, pos, typ, dv(self.mean_in), dv(self.rstd_in), g, A["dword"], A["dpos"], A["dtype0"], A["dgamma"],
                         A["dbeta"], c["B"], c["L"], c["D"], PAD_ID, self.drop)
        self._keep_alive = base

    def restate(self, fault=None, order="tree"):
        M, D = self.M, self.c["D"]
        v = ((self.word[self.row_id] + self.pos[self.row_pos]).astype(F) + self.typ[0][None]).astype(F)
        o, mu, rs = ln_fwd32(v, self.g, self.b, self.eps, order)
        keep = self.keep
        if fault == "dropout_pair_swapped":
            keep = keep.reshape(-1, 2)[:, ::-1].reshape(keep.shape)
        o = np.where(keep, (o * self.scale).astype(F) if self.c["p"] else o, F(0.0)).astype(F)
        put(self.x[:M], o); put(self.xb[:M], o); put(self.mean[:M], mu); put(self.rstd[:M], rs)
        xh = ((v - self.mean_in[:, None]).astype(F) * self.rstd_in[:, None]).astype(F)
        d = np.where(keep, (self.dy * self.scale).astype(F) if self.c["p"] else self.dy, F(0.0)).astype(F)
        dx = ln_bwd32(d, xh, self.rstd_in, self.g, order)
        acc = {k: v_.copy() for k, v_ in self.pre.items()}
        for r in (reversed(range(M)) if order == "pair" else range(M)):
            if self.row_id[r] != PAD_ID or fault == "pad_receives_gradient":
                acc["dword"][self.row_id[r]] += dx[r]
            acc["dpos"][self.row_pos[r]] += dx[r]
        rows_g = M - (M % 32 or 32) if fault == "last_partial_workgroup_missing_from_dgamma" else M
        acc["dgamma"] = fold32(acc["dgamma"], colsum32((d * xh).astype(F)[:rows_g], 32, order), order)
        acc["dbeta"] = fold32(acc["dbeta"], colsum32(d, 32, order), order)
        acc["dtype0"] = fold32(acc["dtype0"], colsum32(dx, 32, order), order)
        for k, a in acc.items():
            put(self.acc[k], a)

    def got(self):
        M = self.M
        G = dict(x=npy(self.x[:M]), xb=npy(self.xb[:M]), mean=npy(self.mean[:M]), rstd=npy(self.rstd[:M]))
        G.update({k: npy(v) for k, v in self.acc.items()})
        return G

    def verify(self):
        cid, M, G = self.c["id"], self.M, self.got()
        self.O.check(cid)
        for k in ("x", "xb", "mean", "rstd"):
            assert is_pattern(getattr(self, k)[M:]), "%s: %s written past row M" % (cid, k)
        dropped = ~self.keep
        assert not G["x"][dropped].any() and not G["xb"][dropped].any(), "%s: a dropped element is not exactly 0" % cid
        same_bits(cid + " dword[pad_id]", self.acc["dword"][PAD_ID], torch.zeros(self.c["D"]))
        unnamed = sorted(set(range(V_WORDS)) - set(int(i) for i in self.row_id))
        same_bits(cid + " dword rows no id names", self.acc["dword"][unnamed], torch.from_numpy(self.pre["dword"][unnamed]))
        same_bits(cid + " dpos rows past L", self.acc["dpos"][self.c["L"]:], torch.from_numpy(self.pre["dpos"][self.c["L"]:]))
        return judge(cid, self.ex, G)


# ---- postln_fwd -----------------------------------------------------------------------------------------------------------------------------------------
FORMS = ("out_of_place", "x_aliases_y", "x_none", "stats_none")
FAMILIES = ("unit", "mean300", "spread1e-3", "constant2")         # the row families of family_rows, by index


def _pln_fwd_cases():
    out = []
    for di, D in enumerate((128, 384, 768)):
        for mi, M in enumerate((1, 7, 8, 9, 69)):
            for j in (0, 2):
                form = FORMS[(di + mi + j) % 4]
                eps = 1e-12 if (j == 0) == (mi % 2 == 0) else 1e-5
                out.append(dict(id="plnf-d%d-m%d-%s-eps%g" % (D, M, form, eps), D=D, M=M, form=form, eps=eps, kernel="postln_fwd_kernel<%d>" % (D // 128),
                                seed=len(out)))
    return tuple(out)


PLN_FWD_CASES = _pln_fwd_cases()


def family_rows(rng, M, D, first):
    """[M, D] fp32 rows cycling through FAMILIES from ``first``, and the family index of every row"""
    fam = (np.arange(M) + first) % 4
    y = rng.standard_normal((M, D)).astype(F)
    y[fam == 1] += F(300.0)
    y[fam == 2] *= F(1e-3)
    y[fam == 3] = F(2.0)
    return y, fam


class PlnFwdLaunch:
    def __init__(self, c, device):
        self.c, self.device = c, device
        M, D = c["M"], c["D"]
        rng = _rng(c["seed"], 0xF2)
        if c.get("old"):
            self.y, self.fam = (2.0 * rng.standard_normal((M, D)) + 0.3).astype(F), np.zeros(M, dtype=np.int64)
        else:
            self.y, self.fam = family_rows(rng, M, D, c["seed"])
        self.g, self.b = (1.0 + 0.1 * rng.standard_normal(D)).astype(F), (0.1 * rng.standard_normal(D)).astype(F)
        y8 = self.y.astype(np.float64)
        R = self.R = ln_fwd_ref(y8, np.zeros_like(y8), np.abs(y8), self.g.astype(np.float64), self.b.astype(np.float64), c["eps"])
        form = c["form"]
        E = dict(xb=(R["o"], "C_LN", R["base_o"], R["extra_o"] + half_ulp_bf16(np.abs(R["o"]) + C_LN * R["base_o"] + R["extra_o"])))
        if form != "x_none":
            E["x"] = (R["o"], "C_LN", R["base_o"], R["extra_o"])
        if form != "stats_none":
            E["mean"], E["rstd"] = (R["mu"], "C_LN", R["base_mu"], 0.0), (R["rs"], "C_LN", R["base_rs"], R["extra_rs"])
        self.ex = E
        O = self.O = Out(device)
        y_init = np.concatenate([self.y, np.full((2, D), np.nan, dtype=F)])
        if form == "x_aliases_y":
            self.x = self.yv = O.new("x", (M + 2, D))
            put(self.x[:M], self.y)
        else:
            self.yv = torch.from_numpy(y_init).to(device)
            self.x = O.new("x", (M + 2, D)) if form != "x_none" else None
        self.xb = O.new("xb", (M + 2, D), torch.bfloat16)
        self.mean, self.rstd = (O.new("mean", (M + 2,)), O.new("rstd", (M + 2,))) if form != "stats_none" else (None, None)

    def run_hip(self):
        c = self.c
        ops.postln_fwd(self.yv, torch.from_numpy(self.g).to(self.device), torch.from_numpy(self.b).to(self.device), c["eps"], self.x, self.xb, self.mean,
                       self.rstd, c["M"], c["D"])

    def restate(self, fault=None, order="tree"):
        M = self.c["M"]
        o, mu, rs = ln_fwd32(self.y, self.g, self.b, self.c["eps"], order, one_pass=fault == "one_pass_variance")
        if self.x is not None:
            put(self.x[:M], o)
        put(self.xb[:M], o)
        if self.mean is not None:
            put(self.mean[:M], mu); put(self.rstd[:M], rs)
        if fault == "second_row_of_odd_pair_written" and M % 2:
            put(self.xb[M:M + 1], o[M - 1:M])

    def got(self):
        M = self.c["M"]
        return {k: npy(getattr(self, k)[:M]) for k in self.ex}

    def verify(self):
        cid, M, G = self.c["id"], self.c["M"], self.got()
        self.O.check(cid)
        for k in self.ex:
            assert is_pattern(getattr(self, k)[M:]), "%s: %s written past row M" % (cid, k)
        const_rows = self.fam == 3                               # a constant row: (v - mu) is exactly 0, the output is beta
        if const_rows.any():
            n = int(const_rows.sum())
            if "x" in G:
                same_bits(cid + " x of a constant row", torch.from_numpy(G["x"][const_rows]), torch.from_numpy(np.tile(self.b, (n, 1))))
            same_bits(cid + " xb of a constant row", to_bf16(G["xb"][const_rows]), to_bf16(np.tile(self.b, (n, 1))))
            if "mean" in G:
                same_bits(cid + " mean of a constant row", torch.from_numpy(G["mean"][const_rows]), torch.full((n,), 2.0))
        return judge(cid, self.ex, G)


# ---- postln_bwd / postln_bwd_part ----------------------------------------------------------------------------------------------------------------------
def _pln_bwd_cases():
    out = []
    for M, D in itertools.product((1, 9, 69), (128, 384, 768)):
        for n_rep, p, alias in ((0, 0.1, False), (0, 0.0, True), (LN_REP, 0.1, True), (1, 0.0, False)):
            out.append(dict(M=M, D=D, n_rep=n_rep, p=p, alias=alias, rpw=2))
    out += [dict(M=16384 + 5, D=128, n_rep=0, p=0.1, alias=False, rpw=8), dict(M=16384 + 5, D=128, n_rep=LN_REP, p=0.1, alias=True, rpw=8)]
    for i, c in enumerate(out):
        c.update(id="plnb-d%d-m%d-%s-p%g%s" % (c["D"], c["M"], "part%d" % c["n_rep"] if c["n_rep"] else "direct", c["p"], "-inplace" if c["alias"] else ""),
                 kernel="postln_bwd_kernel<%d, %d>%s" % (c["D"] // 128, c["rpw"], " part" if c["n_rep"] else ""), seed=i)
    return tuple(out)


PLN_BWD_CASES = _pln_bwd_cases()
OLD_PLN_FWD = dict(id="old-postln-fwd-shape", D=128, M=95, form="out_of_place", eps=1e-12, kernel="", seed=904, old=True)
OLD_PLN_BWD = dict(id="old-postln-bwd-shape", M=95, D=128, n_rep=0, p=0.1, alias=False, rpw=2, kernel="", seed=901)


class PlnBwdLaunch:
    def __init__(self, c, device):
        self.c, self.device = c, device
        M, D, n_rep = c["M"], c["D"], c["n_rep"]
        rng = _rng(c["seed"], 0xB3)
        self.y, self.dy = (2.0 * rng.standard_normal((M, D)) + 0.3).astype(F), rng.standard_normal((M, D)).astype(F)
        self.g = (1.0 + 0.1 * rng.standard_normal(D)).astype(F)
        y8 = self.y.astype(np.float64)
        mu8 = y8.mean(1)
        self.mean_in, self.rstd_in = mu8.astype(F), (1.0 / np.sqrt(((y8 - mu8[:, None]) ** 2).mean(1) + 1e-12)).astype(F)
        self.keep, self.drop, self.scale = keep_of(SITE_LN, (M, D), c["p"])
        self.rows_per_block = 4 * c["rpw"]
        self.grid = -(-M // self.rows_per_block)
        self.copies = n_rep + 2 if n_rep else 0
        self.pre = rng.standard_normal((self.copies, 2, D)).astype(F) if n_rep else rng.standard_normal((2, D)).astype(F)
        mu, rs, g = self.mean_in.astype(np.float64), self.rstd_in.astype(np.float64), self.g.astype(np.float64)
        xh = (y8 - mu[:, None]) * rs[:, None]
        d = self.dy.astype(np.float64)
        dx, bdx = ln_bwd_ref(d, xh, rs, g)
        mw, mb, _ = drop_entry(dx, bdx, 0.0 * bdx, self.keep, self.scale)
        E = dict(dx=(dx, "C_LNB", bdx, 0.0), dxb=(mw, "C_LNB", mb, half_ulp_bf16(np.abs(mw) + C_LNB * mb)))
        pre8 = self.pre.astype(np.float64)
        tg, tb = d * xh, d
        if n_rep:
            blk = np.arange(M) // self.rows_per_block
            want, base = pre8.copy(), U24 * np.abs(pre8)
            for k in range(min(n_rep, self.grid)):
                sel = blk % n_rep == k
                want[k, 0] += tg[sel].sum(0); want[k, 1] += tb[sel].sum(0)
                base[k, 0] += U24 * np.abs(tg[sel]).sum(0); base[k, 1] += U24 * np.abs(tb[sel]).sum(0)
            E["part"] = (want, "C_COL", base, 0.0)
        else:
            E["dgamma"] = (tg.sum(0) + pre8[0], "C_COL", U24 * (np.abs(tg).sum(0) + np.abs(pre8[0])), 0.0)
            E["dbeta"] = (tb.sum(0) + pre8[1], "C_COL", U24 * (np.abs(tb).sum(0) + np.abs(pre8[1])), 0.0)
        self.ex = E
        O = self.O = Out(device)
        self.dx, self.dxb = O.new("dx", (M + 2, D)), O.new("dxb", (M + 2, D), torch.bfloat16)
        if n_rep:
            self.part = O.new("part", self.pre.shape, init=self.pre)
        else:
            self.dgamma, self.dbeta = O.new("dgamma", (D,), init=self.pre[0]), O.new("dbeta", (D,), init=self.pre[1])
        if c["alias"]:                                       # the second launch, dx aliasing dy: the same bits
            self.dx2, self.dxb2 = O.new("dx2", (M + 2, D)), O.new("dxb2", (M + 2, D), torch.bfloat16)
            put(self.dx2[:M], self.dy)
            self.scratch = O.new("scratch", self.pre.shape, init=self.pre)

    def run_hip(self):
        c, dv = self.c, lambda a: torch.from_numpy(a).to(self.device)   # noqa: E731
        y, mean, rstd, g, dy = dv(self.y), dv(self.mean_in), dv(self.rstd_in), dv(self.g), dv(self.dy)
        M, D, n_rep = c["M"], c["D"], c["n_rep"]
        if n_rep:
            ops.postln_bwd_part(dy, y, mean, rstd, g, self.dx, self.dxb, self.part, n_rep, M, D, self.drop)
            if c["alias"]:
                ops.postln_bwd_part(self.dx2, y, mean, rstd, g, self.dx2, self.dxb2, self.scratch, n_rep, M, D, self.drop)
        else:
            ops.postln_bwd(dy, y, mean, rstd, g, self.dx, self.dxb, self.dgamma, self.dbeta, M, D, self.drop)
            if c["alias"]:
                ops.postln_bwd(self.dx2, y, mean, rstd, g, self.dx2, self.dxb2, self.scratch[0], self.scratch[1], M, D, self.drop)

    def restate(self, fault=None, order="tree"):
        c, M, n_rep = self.c, self.c["M"], self.c["n_rep"]
        xh = ((self.y - self.mean_in[:, None]).astype(F) * self.rstd_in[:, None]).astype(F)
        dx = ln_bwd32(self.dy, xh, self.rstd_in, self.g, order)
        keep = self.keep.reshape(-1, 2)[:, ::-1].reshape(self.keep.shape) if fault == "dropout_pair_swapped" else self.keep
        scale = F(1.0) if fault == "dropout_scale_left_off_bf16_branch" else self.scale
        m = np.where(keep, (dx * scale).astype(F) if c["p"] else dx, F(0.0)).astype(F)
        put(self.dx[:M], dx); put(self.dxb[:M], m)
        if c["alias"]:
            put(self.dx2[:M], dx); put(self.dxb2[:M], m)
        bg, bb = colsum32((self.dy * xh).astype(F), self.rows_per_block, order), colsum32(self.dy, self.rows_per_block, order)
        if n_rep:
            acc = self.pre.copy()
            for k in range(min(n_rep, self.grid)):
                sel = np.arange(self.grid) % n_rep == k
                if fault == "part_copy_overwritten" and k == 0:
                    acc[k] = 0.0
                acc[k, 0], acc[k, 1] = fold32(acc[k, 0], bg[sel], order), fold32(acc[k, 1], bb[sel], order)
            put(self.part, acc)
        else:
            put(self.dgamma, fold32(self.pre[0], bg, order)); put(self.dbeta, fold32(self.pre[1], bb, order))

    def got(self):
        M = self.c["M"]
        G = dict(dx=npy(self.dx[:M]), dxb=npy(self.dxb[:M]))
        G.update(dict(part=npy(self.part)) if self.c["n_rep"] else dict(dgamma=npy(self.dgamma), dbeta=npy(self.dbeta)))
        return G

    def verify(self):
        c, cid, M, G = self.c, self.c["id"], self.c["M"], self.got()
        self.O.check(cid)
        for k in ("dx", "dxb") + (("dx2", "dxb2") if c["alias"] else ()):
            assert is_pattern(getattr(self, k)[M:]), "%s: %s written past row M" % (cid, k)
        assert not G["dxb"][~self.keep].any(), "%s: a dropped element of dxb is not exactly 0" % cid
        if c["alias"]:
            same_bits(cid + " dx, dx aliasing dy", self.dx2[:M], self.dx[:M])
            same_bits(cid + " dxb, dx aliasing dy", self.dxb2[:M], self.dxb[:M])
        if c["n_rep"]:
            first = min(c["n_rep"], self.grid)
            same_bits(cid + " partial copies no workgroup maps to", self.part[first:], torch.from_numpy(self.pre[first:]))
        return judge(cid, self.ex, G)


# ---- meanpool_fwd / meanpool_bwd ------------------------------------------------------------------------------------------------------------------------
def _pool_cases():
    out, Ds = [], (64, 128, 768)
    for i, L in enumerate((1, 3, 4, 16, 17, 19, 35)):
        for j in (0, 1):
            D = Ds[(i + j) % 3]
            for sl, p in (((True, 0.1), (False, 0.0)) if (i + j) % 2 else ((False, 0.1), (True, 0.0))):
                out.append(dict(id="pool-d%d-l%d-%s-p%g" % (D, L, "seqlen" if sl else "all", p), D=D, L=L, B=3, seq_len=sl, p=p,
                                kernel="meanpool_fwd_kernel meanpool_bwd_kernel", seed=len(out)))
    return tuple(out)


POOL_CASES = _pool_cases()
OLD_POOL = dict(id="old-meanpool-shape", D=128, L=19, B=5, seq_len=True, p=0.1, kernel="", seed=902, old=True)


class PoolLaunch:
    def __init__(self, c, device):
        self.c, self.device = c, device
        B, L, D = c["B"], c["L"], c["D"]
        rng = _rng(c["seed"], 0xA4)
        self.x, self.df = rng.standard_normal((B, L, D)).astype(F), rng.standard_normal((B, D)).astype(F)
        self.sl = (np.array([L, L - 4, 1, L, 7]) if c.get("old") else np.array([L, 1, (L + 1) // 2])).astype(np.int32) if c["seq_len"] else None
        Ls = self.sl.astype(np.int64) if self.sl is not None else np.full(B, L)
        self.Ls = Ls
        self.keep, self.drop, self.scale = keep_of(SITE_POOL, (B, L, D), c["p"])
        self.valid = np.arange(L)[None, :, None] < Ls[:, None, None]
        use = self.keep & self.valid
        x8 = self.x.astype(np.float64)
        f = (float(self.scale) / Ls)[:, None]
        feat = np.where(use, x8, 0.0).sum(1) * f
        dx = np.where(use, self.df.astype(np.float64)[:, None, :] * f[:, :, None], 0.0)       # (the kernel: fl32(scale / Ls), then one product: two roundings)
        self.ex = dict(feat=(feat, "C_POOL", U24 * np.where(use, np.abs(x8), 0.0).sum(1) * f, 0.0), dx=(dx, "C_POOL", 0.0 * dx, 2.01 * U24 * np.abs(dx)))
        O = self.O = Out(device)
        self.feat, self.dx = O.new("feat", (B + 1, D)), O.new("dx", (B * L * D + 3,))
        self.n = B * L * D

    def run_hip(self):
        c, dv = self.c, lambda a: torch.from_numpy(a).to(self.device)   # noqa: E731
        sl = dv(self.sl) if self.sl is not None else None
        ops.meanpool_fwd(dv(self.x), self.feat, c["B"], c["L"], c["D"], self.drop, sl)
        ops.meanpool_bwd(dv(self.df), self.dx, c["B"], c["L"], c["D"], self.drop, sl)

    def restate(self, fault=None, order="tree"):
        c, B, L = self.c, self.c["B"], self.c["L"]
        use = self.keep & self.valid
        t = np.where(use, self.x, F(0.0)).astype(F)
        if order == "pair":
            s = np.cumsum(t[:, ::-1], axis=1, dtype=F)[:, -1]
        else:                                               # four waves take every fourth row; a wave's four rows in flight have a sum each
            tp = np.zeros((B, -(-L // 16) * 16, c["D"]), dtype=F)
            tp[:, :L] = t
            lanes = np.cumsum(tp.reshape(B, -1, 16, c["D"]), axis=1, dtype=F)[:, -1]         # [B, 16, D]: row p lands in slot p % 16
            w = lanes.reshape(B, 4, 4, c["D"])                                                 # slot = 4 u + wave
            per_wave = ((w[:, 0] + w[:, 1]).astype(F) + (w[:, 2] + w[:, 3]).astype(F)).astype(F)
            s = ((per_wave[:, 0] + per_wave[:, 1]).astype(F) + per_wave[:, 2]).astype(F) + per_wave[:, 3]
        den = np.full(B, L, dtype=F) if fault == "meanpool_divides_by_L" else self.Ls.astype(F)
        fac = (self.scale / den).astype(F)
        put(self.feat[:B], (s.astype(F) * fac[:, None]).astype(F))
        dx = np.where(use, (self.df[:, None, :] * (self.scale / self.Ls.astype(F)).astype(F)[:, None, None]).astype(F), F(0.0))
        put(self.dx[:self.n], dx.reshape(-1))

    def got(self):
        c = self.c
        return dict(feat=npy(self.feat[:c["B"]]), dx=npy(self.dx[:self.n]).reshape(c["B"], c["L"], c["D"]))

    def verify(self):
        cid, G = self.c["id"], self.got()
        self.O.check(cid)
        assert is_pattern(self.feat[self.c["B"]:]) and is_pattern(self.dx[self.n:]), "%s: written past the end" % cid
        z = np.broadcast_to(~self.valid, G["dx"].shape)
        same_bits(cid + " filler rows of dx", torch.from_numpy(G["dx"][z]), torch.zeros(int(z.sum())))
        same_bits(cid + " dropped elements of dx", torch.from_numpy(G["dx"][~self.keep]), torch.zeros(int((~self.keep).sum())))
        return judge(cid, self.ex, G)


# ---- gelu_f32 / gelu_bwd_f32 -----------------------------------------------------------------------------------------------------------------------------
PLANTED = (0.0, -0.0, 1e-30, -1e-30, 0.75, -0.75, 5.0, -5.0, 10.0, -10.0, 40.0, -40.0, 1e4, -1e4)
GELU_CASES = tuple(dict(id="gelu-n%d-r%d" % (n, r), n=n, first=r, kernel="gelu_f32_kernel gelu_bwd_f32_kernel", seed=i)
                   for i, (n, r) in enumerate([(n, 0) for n in (255, 257, 4099)] + [(1, r) for r in range(len(PLANTED))]))
RSQRT2, RSQRT2PI = 0.70710678118654752440, 0.39894228040143267794


def gelu_inputs(c):
    rng = _rng(c["seed"], 0x6E)
    v, dout = (2.0 * rng.standard_normal(c["n"])).astype(F), rng.standard_normal(c["n"]).astype(F)
    k = min(c["n"], len(PLANTED))
    v[:k] = np.array(PLANTED, dtype=F)[(np.arange(k) + c["first"]) % len(PLANTED)]
    return v, dout


class GeluLaunch:
    def __init__(self, c, device):
        self.c, self.device = c, device
        self.v, self.dout = gelu_inputs(c)
        v, do = torch.from_numpy(self.v).double(), self.dout.astype(np.float64)
        t = v * RSQRT2
        erf = torch.erf(t).numpy()
        v, t = v.numpy(), t.numpy()
        dens = np.exp(-0.5 * v * v)
        derf = 2.0 / math.sqrt(math.pi) * np.exp(-t * t)
        out = 0.5 * v * (1.0 + erf)
        Phi, vphi = 0.5 * (1.0 + erf), v * RSQRT2PI * dens
        dpre = do * (Phi + vphi)
        self.ex = dict(out=(out, "C_GELU", U24 * (np.abs(0.5 * v) * (1.0 + np.abs(erf) + np.abs(t) * derf) + np.abs(out)), np.abs(0.5 * v) * ERF_ULP * U23 * np.abs(erf)),
                       dpre=(dpre, "C_GELU", U24 * np.abs(do) * (0.5 * (1.0 + np.abs(erf) + np.abs(t) * derf) + np.abs(vphi) * (1.0 + 0.5 * v * v) + np.abs(Phi + vphi)),
                             np.abs(do) * (0.5 * ERF_ULP * U23 * np.abs(erf) + EXP_ULP * U23 * np.abs(vphi))))
        O = self.O = Out(device)
        self.out, self.dpre = O.new("out", (c["n"] + 3,)), O.new("dpre", (c["n"] + 3,))

    def run_hip(self):
        n, dv = self.c["n"], lambda a: torch.from_numpy(a).to(self.device)   # noqa: E731
        ops.gelu_f32(dv(self.v), self.out, n)
        ops.gelu_bwd_f32(dv(self.dout), dv(self.v), self.dpre, n)

    def restate(self, fault=None, order="tree"):
        n, v = self.c["n"], torch.from_numpy(self.v)
        erf = torch.erf(v * float(F(RSQRT2)))
        put(self.out[:n], (0.5 * v * (1.0 + erf)).numpy())
        dens = torch.exp(-0.5 * v * v)
        put(self.dpre[:n], (torch.from_numpy(self.dout) * (0.5 * (1.0 + erf) + v * float(F(RSQRT2PI)) * dens)).numpy())

    def got(self):
        return dict(out=npy(self.out[:self.c["n"]]), dpre=npy(self.dpre[:self.c["n"]]))

    def verify(self):
        cid, n, G, v = self.c["id"], self.c["n"], self.got(), self.v
        self.O.check(cid)
        assert is_pattern(self.out[n:]) and is_pattern(self.dpre[n:]), "%s: written past n" % cid
        assert np.isfinite(G["out"]).all() and np.isfinite(G["dpre"]).all(), "%s: a non-finite result" % cid
        big, far = np.abs(v) >= 10.0, np.abs(v) >= 40.0          # erf(|v| / sqrt 2) is 1 in fp32 from 10 on; the density term is below every ulp from 40 on
        assert (G["out"][big & (v > 0)] == v[big & (v > 0)]).all() and (G["out"][big & (v < 0)] == 0.0).all() and (G["out"][v == 0.0] == 0.0).all(), cid + ": limit of gelu"
        assert (G["dpre"][far & (v > 0)] == self.dout[far & (v > 0)]).all() and (G["dpre"][far & (v < 0)] == 0.0).all(), cid + ": limit of gelu'"
        return judge(cid, self.ex, G)


# ---- dropout_cast / mask_lengths (held to bits) ----------------------------------------------------------------------------------------------------------
CAST_CASES = tuple(dict(id="cast-n%d-p%g" % (n, p), n=n, p=p, kernel="dropout_cast_kernel", seed=i) for i, (n, p) in enumerate(itertools.product((2, 510, 514), (0.0, 0.1, 0.5))))
MASK_CASES = tuple(dict(id="mask-l%d" % L, L=L, kernel="mask_len_kernel", seed=i) for i, L in enumerate((1, 63, 64, 65, 512)))


class CastLaunch:
    def __init__(self, c, device):
        self.c, self.device = c, device
        self.x = _rng(c["seed"], 0xCA).standard_normal(c["n"]).astype(F)
        self.keep, self.drop, self.scale = keep_of(SITE_CAST, (c["n"],), c["p"])
        self.O = Out(device)
        self.out = self.O.new("out", (c["n"] + 4,), torch.bfloat16)
        self.want = to_bf16(np.where(self.keep, (self.x * self.scale).astype(F) if c["p"] else self.x, F(0.0)).astype(F))

    def run_hip(self):
        ops.dropout_cast(torch.from_numpy(self.x).to(self.device), self.out, self.c["n"], self.drop)

    def restate(self, fault=None, order="tree"):
        keep = self.keep.reshape(-1, 2)[:, ::-1].reshape(-1) if fault == "dropout_pair_swapped" else self.keep
        put(self.out[:self.c["n"]], np.where(keep, (self.x * self.scale).astype(F) if self.c["p"] else self.x, F(0.0)).astype(F))

    def verify(self):
        cid, n = self.c["id"], self.c["n"]
        self.O.check(cid)
        assert is_pattern(self.out[n:]), "%s: written past n" % cid
        same_bits(cid + " out", self.out[:n], self.want)
        return {}


class MaskLaunch:
    def __init__(self, c, device):
        self.c, self.device = c, device
        L, rng = c["L"], _rng(c["seed"], 0x3A)
        self.counts = [0, L, L // 2, 1, (L + 2) // 3]
        base = rng.integers(1, 9, size=(len(self.counts), L + 3), dtype=np.int64) * rng.choice([-1, 1], size=(len(self.counts), L + 3))
        for r, n in enumerate(self.counts):
            base[r, 1 + n:1 + L] = 0
        self.base = base                                   # (column 0 and the two columns after the window are non-zero and must not count)
        self.O = Out(device)
        self.klen = self.O.new("klen", (len(self.counts) + 2,), torch.int32)

    def run_hip(self):
        self._base = torch.from_numpy(self.base).to(self.device)
        ops.mask_lengths(RowsView(self._base[:, 1:1 + self.c["L"]]), self.klen, len(self.counts), self.c["L"])

    def restate(self, fault=None, order="tree"):
        put(self.klen[:len(self.counts)], (self.base[:, 1:1 + self.c["L"]] != 0).sum(1).astype(np.int32))

    def verify(self):
        cid, B = self.c["id"], len(self.counts)
        self.O.check(cid)
        assert is_pattern(self.klen[B:]), "%s: written past B" % cid
        assert self.klen[:B].cpu().tolist() == self.counts, (cid, self.klen[:B].cpu().tolist(), self.counts)
        return {}


# ---- adamw_flat / adamw_flat_dyn ---------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 255, 256, 257, 4096, 4097, 5000)
LR_T = (5e-4, 2.5e-4, 0.0, 1e-3, 5e-4, 1.25e-4, 5e-4)         # tensor 2 is frozen (lr = wd = 0), tensors 1 and 6 have no weight decay
WD_T = (5e-4, 0.0, 0.0, 5e-4, 0.05, 5e-4, 0.0)
GAPS = (3, 1, 64, 0, 7, 250, 2, 5)                              # elements before tensor i of an ``offsets`` table (and after the last)
PLANT_G = (0.0, 1e-12, -1e-12, 1e3, -1e3)
LR_FACTOR = 0.37


def _adam(cid, table, step, pb, ema, zero_grad, grad_scale, clip, ema_m, dyn):
    return dict(id=cid, table=table, step=step, pb=pb, ema=ema, zero_grad=zero_grad, grad_scale=grad_scale, clip=clip, ema_m=ema_m, dyn=dyn,
                kernel="adamw_flat_kernel" + (" dyn" if dyn else " by-value"))


ADAM_CASES = (
    _adam("adam-dense-s1-all", "dense", 1, True, True, True, 1.0, False, 0.9, False),
    _adam("adam-gaps-s2-all-keepgrad-scale-clip-dyn", "gaps", 2, True, True, False, 0.25, True, 0.999, True),
    _adam("adam-gaps-s1000-nopb-scale", "gaps", 1000, False, True, True, 0.25, False, 0.9, False),
    _adam("adam-dense-s1000-noema-keepgrad-clip-dyn", "dense", 1000, True, False, False, 1.0, True, 0.9, True),
    _adam("adam-gaps-s2-bare-clip", "gaps", 2, False, False, True, 1.0, True, 0.9, False),
    _adam("adam-dense-s1-all-scale-dyn", "dense", 1, True, True, True, 0.25, False, 0.999, True),
)
for _i, _c in enumerate(ADAM_CASES):
    _c["seed"] = _i
OLD_ADAM = dict(_adam("old-adamw-form", "dense", 1, True, True, True, 1.0, False, 0.9, False), seed=903, old=True)


class AdamLaunch:
    CLIP0 = F(0.6180339887)

    def __init__(self, c, device):
        self.c, self.device = c, device
        rng = _rng(c["seed"], 0xAD)
        if c["table"] == "gaps":
            offs, o = [], 0
            for gap, n in zip(GAPS, SIZES):
                o += gap
                offs.append(o)
                o += n
            self.offsets, self.total = offs, o + GAPS[-1]
            self.table = build_chunk_table(list(SIZES), offsets=offs)
        else:
            self.offsets, self.total = list(np.cumsum((0,) + SIZES[:-1])), sum(SIZES)
            self.table = build_chunk_table(list(SIZES))
        inside = np.zeros(self.total, dtype=bool)
        tid = np.zeros(self.total, dtype=np.int64)
        for i, (o, n) in enumerate(zip(self.offsets, SIZES)):
            inside[o:o + n], tid[o:o + n] = True, i
        self.inside, self.tid = inside, tid
        n = self.total
        p, g, m = (0.05 * rng.standard_normal(n)).astype(F), (0.1 * rng.standard_normal(n)).astype(F), (0.01 * rng.standard_normal(n)).astype(F)
        v = (1e-4 * rng.uniform(0.5, 1.5, n)).astype(F)
        if c.get("old"):
            m[:], v[:] = 0.0, 0.0
        else:
            for o, sz in zip(self.offsets, SIZES):          # planted gradients at the head of every tensor that holds them; the +-1e-12 ones with tiny moments
                k = min(sz, len(PLANT_G)) if sz >= 255 else 0
                g[o:o + k] = np.array(PLANT_G[:k], dtype=F)
                m[o:o + min(k, 3)], v[o:o + min(k, 3)] = F(1e-13), F(1e-26)
                p[o + 3:o + k] = F(1e-7)                   # (and a parameter far below its update: what the order of decay and update shows on)
        self.init = dict(p=p, g=g, m=m, v=v, ema=(p + (0.01 * rng.standard_normal(n)).astype(F)).astype(F))
        self.bc1, self.bc2s = (F(x) for x in ops.adam_bias_corrections(0.9, 0.999, c["step"]))
        self.lrf = F(LR_FACTOR)
        self.gs = (F(c["grad_scale"]) * self.CLIP0).astype(F) if c["clip"] else F(c["grad_scale"])
        self.ema_m, self.ema_1m = F(c["ema_m"]), F(1.0 - c["ema_m"])
        self.ex = self._expect()
        O = self.O = Out(device)
        self.buf, ins_t = {}, torch.from_numpy(inside).to(device)
        for tag in ("", "2") if c["dyn"] else ("",):
            for k, a in self.init.items():
                if k != "ema" or c["ema"]:
                    self.buf[k + tag] = O.new(k + tag, (n,))
                    self.buf[k + tag][ins_t] = torch.from_numpy(a[inside]).to(device)
            if c["pb"]:
                self.buf["pb" + tag] = O.new("pb" + tag, (n,), torch.bfloat16)
                self.buf["pb" + tag][ins_t] = to_bf16(p[inside]).to(device)

    def scalars(self):
        """per element, in the kernel's fp32: lr, decay, step; b1, 1 - b1, b2, 1 - b2, eps"""
        lr = (np.array(LR_T, dtype=F) * self.lrf).astype(F)
        decay = (F(1.0) - (lr * np.array(WD_T, dtype=F)).astype(F)).astype(F)
        step = (lr / self.bc1).astype(F)
        b1, b2 = F(0.9), F(0.999)
        return lr[self.tid], decay[self.tid], step[self.tid], b1, F(1.0) - b1, b2, F(1.0) - b2, F(1e-8)

    def _expect(self):
        f8 = lambda a: np.asarray(a, dtype=np.float64)   # noqa: E731
        _, decay, step, b1, ob1, b2, ob2, eps = (f8(s) for s in self.scalars())
        R = adamw_ref(f8(self.init["p"]), f8(self.init["g"]) * float(self.gs), f8(self.init["m"]), f8(self.init["v"]), decay, step, b1, ob1, b2, ob2,
                      float(self.bc2s), eps)
        self.ref = R
        return dict(p=(R["p"], "C_ADAM", U24 * R["U"], U24 * (2.0 * np.abs(R["pi"]) + np.abs(R["p"]))),
                    m=(R["m"], "C_ADAM", U24 * R["m_terms"], U24 * np.abs(R["m"])), v=(R["v"], "C_ADAM", U24 * R["v_terms"], U24 * np.abs(R["v"])))

    def run_hip(self):
        c, dv = self.c, lambda a: torch.as_tensor(a).to(self.device)   # noqa: E731
        table = self.table.to(self.device).contiguous()
        lr_t, wd_t = dv(np.array(LR_T, dtype=F)), dv(np.array(WD_T, dtype=F))
        clip = dv(np.array([self.CLIP0, 123.0], dtype=F)) if c["clip"] else None
        B = self.buf
        kw = dict(ema_m=c["ema_m"], grad_scale=c["grad_scale"], zero_grad=c["zero_grad"], clip_coef=clip)
        if c["dyn"]:
            self._dyn = dv(np.array([self.lrf, self.bc1, self.bc2s], dtype=F))
            ops.adamw_flat(B["p"], B["g"], B["m"], B["v"], B.get("pb"), B.get("ema"), table, table.shape[0], lr_t, wd_t, 0.0, 0, dyn=self._dyn.data_ptr(), **kw)
            ops.adamw_flat(B["p2"], B["g2"], B["m2"], B["v2"], B.get("pb2"), B.get("ema2"), table, table.shape[0], lr_t, wd_t, LR_FACTOR, c["step"], **kw)
        else:
            ops.adamw_flat(B["p"], B["g"], B["m"], B["v"], B.get("pb"), B.get("ema"), table, table.shape[0], lr_t, wd_t, LR_FACTOR, c["step"], **kw)

    def restate(self, fault=None, order="tree"):
        c, I = self.c, self.init
        _, decay, step, b1, ob1, b2, ob2, eps = self.scalars()
        bc1, bc2s = (self.bc2s, self.bc1) if fault == "bc1_and_bc2_swapped" else (self.bc1, self.bc2s)
        if fault == "bc1_and_bc2_swapped":
            step = (self.scalars()[0] / bc1).astype(F)
        gi = (I["g"] * self.gs).astype(F)
        if order == "tree":                                   # every operation rounded on its own
            mi = ((b1 * I["m"]).astype(F) + (ob1 * gi).astype(F)).astype(F)
            vi = ((b2 * I["v"]).astype(F) + ((ob2 * gi).astype(F) * gi).astype(F)).astype(F)
        else:                                                 # the sums contracted into fused multiply-adds
            mi = (b1.astype(np.float64) * I["m"] + (ob1 * gi).astype(F)).astype(F)
            vi = (b2.astype(np.float64) * I["v"] + ((ob2 * gi).astype(F) * gi).astype(F)).astype(F)
        upd = ((step * mi).astype(F) / ((np.sqrt(vi) / bc2s).astype(F) + eps).astype(F)).astype(F)
        if fault == "weight_decay_after_the_update":
            pi = ((I["p"] - upd).astype(F) * decay).astype(F)
        else:
            pi = ((I["p"] * decay).astype(F) - upd).astype(F)
        done = self.inside.copy()
        if fault == "chunk_tail_skipped":
            for o, ln, _, _ in self.table.tolist():
                if ln % 256:
                    done[o:o + ln] = False
        e1m = (F(1.0) - self.ema_m) if fault == "ema_one_minus_m_in_float32" else self.ema_1m
        ema = ((e1m * pi).astype(F) + (self.ema_m * I["ema"]).astype(F)).astype(F)
        new = dict(p=pi, m=mi, v=vi, ema=ema, g=np.where(c["zero_grad"], F(0.0), I["g"]).astype(F))
        sel = torch.from_numpy(done)
        for tag in ("", "2") if c["dyn"] else ("",):
            for k, a in new.items():
                if k + tag in self.buf:
                    self.buf[k + tag][sel] = torch.from_numpy(a[done])
            if c["pb"]:
                self.buf["pb" + tag][sel] = to_bf16(pi[done])

    def got(self):
        ins = self.inside
        return {k: np.where(ins, npy(self.buf[k]), self.ex[k][0]) for k in ("p", "m", "v")}

    def verify(self):
        c, cid, B, ins, I = self.c, self.c["id"], self.buf, torch.from_numpy(self.inside), self.init
        self.O.check(cid)
        for k, t in B.items():
            assert is_pattern(t.cpu()[~ins]), "%s: %s written in a gap of the chunk table" % (cid, k)
        p_got = B["p"].cpu()[ins]
        if c["pb"]:
            same_bits(cid + " pb against bf16 RNE of the p the launch wrote", B["pb"].cpu()[ins], p_got.to(torch.bfloat16))
        if c["ema"]:
            pg, e0 = p_got.numpy(), I["ema"][self.inside]
            want = ((self.ema_1m * pg).astype(F) + (self.ema_m * e0).astype(F)).astype(F)
            same_bits(cid + " ema against its three fp32 operations on the launch's p", B["ema"].cpu()[ins], torch.from_numpy(want))
        same_bits(cid + " g after zero_grad=%s" % c["zero_grad"], B["g"].cpu()[ins], torch.zeros(int(ins.sum())) if c["zero_grad"] else torch.from_numpy(I["g"][self.inside]))
        frozen = torch.from_numpy(self.inside & (self.tid == 2))
        same_bits(cid + " p of the frozen tensor", B["p"].cpu()[frozen], torch.from_numpy(I["p"][frozen.numpy()]))
        if c["pb"]:
            same_bits(cid + " pb of the frozen tensor", B["pb"].cpu()[frozen], to_bf16(I["p"][frozen.numpy()]))
        if c["dyn"]:
            for k in [k for k in B if not k.endswith("2")]:
                same_bits(cid + " %s: dyn against by-value" % k, B[k], B[k + "2"])
        return judge(cid, self.ex, self.got())


def adamw_ref(p, g, m, v, decay, step, b1, ob1, b2, ob2, bc2s, eps):
    """the kernel's formula in float64 (g: already scaled) -> p, m, v, pi = p decay, U = step (|b1 m| + |(1 - b1) g|) / denom, the |terms| of m and v"""
    pi = p * decay
    mi, vi = b1 * m + ob1 * g, b2 * v + ob2 * g * g
    den = np.sqrt(vi) / bc2s + eps
    return dict(p=pi - step * mi / den, m=mi, v=vi, pi=pi, U=step * (np.abs(b1 * m) + np.abs(ob1 * g)) / den, m_terms=np.abs(b1 * m) + np.abs(ob1 * g), v_terms=vi)


# ---- clip_grad_coef ------------------------------------------------------------------------------------------------------------------------------------------
def _clip_cases():
    out = []
    for i, n in enumerate((1, 1023, 1024, 1025, 300001)):
        for j, (pre, below) in enumerate(((0.5, True), (1.0, False)) if i % 2 == 0 else ((1.0, True), (0.5, False))):
            out.append(dict(id="clip-n%d-pre%g-%s" % (n, pre, "clipped" if below else "coef1"), n=n, pre=pre, below=below, dominant=False))
    out.append(dict(id="clip-n1025-dominant", n=1025, pre=1.0, below=True, dominant=True))
    for i, c in enumerate(out):
        c.update(seed=i, kernel="sumsq_part_kernel clip_coef_kernel")
    return tuple(out)


CLIP_CASES = _clip_cases()


class ClipLaunch:
    def __init__(self, c, device):
        self.c, self.device = c, device
        n, rng = c["n"], _rng(c["seed"], 0xC1)
        self.g = rng.standard_normal(n).astype(F)
        if c["dominant"]:
            self.g *= F(1e-3)
            self.g[777] = F(1e3)
        g8 = self.g.astype(np.float64)
        per = -(-n // CLIP_WG)
        self.per = per
        sq = np.zeros(CLIP_WG * per)
        sq[:n] = g8 * g8
        parts = sq.reshape(CLIP_WG, per).sum(1)
        norm = c["pre"] * math.sqrt(parts.sum())
        self.max_norm = float(F(norm * (0.5 if c["below"] else 2.0)))
        self.ex = dict(ws=(parts, "C_NORM", U24 * parts, 0.0), norm=(np.array([norm]), "C_NORM", U24 * np.array([norm]), 0.0))
        O = self.O = Out(device)
        self.ws, self.coef = O.new("ws", (CLIP_WG + 8,)), O.new("coef", (6,))

    def run_hip(self):
        c = self.c
        assert ops.clip_grad_ws_floats() == CLIP_WG
        ops.clip_grad_coef(torch.from_numpy(self.g).to(self.device), c["n"], c["pre"], self.max_norm, self.ws, self.coef)

    def restate(self, fault=None, order="tree"):
        c, n, per = self.c, self.c["n"], self.per
        sq = np.zeros(CLIP_WG * per, dtype=F)
        sq[:n] = (self.g * self.g).astype(F)
        sq = sq.reshape(CLIP_WG, per)
        if order == "pair":
            parts = pairsum32(sq)
        else:                                               # a thread takes every 256th element in turn; the wave tree, the four waves
            t = np.zeros((CLIP_WG, -(-per // 256) * 256), dtype=F)
            t[:, :per] = sq
            parts = pairsum32(np.cumsum(t.reshape(CLIP_WG, -1, 256), axis=1, dtype=F)[:, -1])
        used = parts.astype(np.float64)
        if fault == "clip_norm_misses_the_last_partition":
            used = used[:(n - 1) // per]
        total = F(c["pre"]) * F(math.sqrt(used.sum()))
        put(self.ws[:CLIP_WG], parts)
        put(self.coef[:2], np.array([min(F(1.0), F(self.max_norm) / (total + F(1e-6))), total], dtype=F))

    def got(self):
        return dict(ws=npy(self.ws[:CLIP_WG]), norm=npy(self.coef[1:2]))

    def verify(self):
        cid, G = self.c["id"], self.got()
        self.O.check(cid)
        assert is_pattern(self.ws[CLIP_WG:]) and is_pattern(self.coef[2:]), "%s: written past the end" % cid
        assert not bool((self.ws[:CLIP_WG].cpu().view(torch.int32) == PATTERN * 0x10001).any()), "%s: a partial was left unwritten" % cid
        total = G["norm"].astype(F)[0]
        cf = F(self.max_norm) / (total + F(1e-6))
        same_bits(cid + " coef_out[0] from the launch's own norm", self.coef[:1], torch.tensor([cf if cf < F(1.0) else F(1.0)], dtype=torch.float32))
        assert (float(self.coef[0]) < 1.0) == self.c["below"], "%s: the case was to land on the %s branch" % (cid, "coef < 1" if self.c["below"] else "coef = 1")
        return judge(cid, self.ex, G)


# ---- the tables, the measurements ------------------------------------------------------------------------------------------------------------------------
FAMILY = (("embed", EmbedLaunch, EMBED_CASES), ("postln_fwd", PlnFwdLaunch, PLN_FWD_CASES), ("postln_bwd", PlnBwdLaunch, PLN_BWD_CASES),
          ("meanpool", PoolLaunch, POOL_CASES), ("gelu", GeluLaunch, GELU_CASES), ("dropout_cast", CastLaunch, CAST_CASES),
          ("mask_lengths", MaskLaunch, MASK_CASES), ("adamw", AdamLaunch, ADAM_CASES), ("clip_grad_coef", ClipLaunch, CLIP_CASES))


def all_cases():
    return [(cls, c) for _, cls, cs in FAMILY for c in cs]


def measure_constants():
    """name -> the worst error of the float32 restatement in units of base, over every case with a bound and both orders"""
    R = {}
    for cls, c in all_cases():
        if cls in (CastLaunch, MaskLaunch):
            continue
        for order in ORDERS:
            L = cls(c, "cpu")
            L.restate(order=order)
            for k, v in ratios(L.ex, L.got()).items():
                R[k] = max(R.get(k, 0.0), v)
    return R


def ulps_of(got32, want64):
    """|got - want| in units of the last place of the fp32 nearest want"""
    want64 = np.asarray(want64, dtype=np.float64)
    ulp = np.spacing(np.abs(want64).astype(F)).astype(np.float64)
    ok = np.isfinite(want64) & (np.abs(want64) >= 2.0 ** -126)
    return float((np.abs(np.asarray(got32, dtype=np.float64) - want64)[ok] / ulp[ok]).max()) if ok.any() else 0.0


def measure_intrinsics():
    """worst error in ulps of torch's float32 erf, exp and rsqrt against float64 over the arguments the cases hand them"""
    t, e, r = [], [], []
    for c in GELU_CASES:
        v = gelu_inputs(c)[0]
        t.append((v * F(RSQRT2)).astype(F))
        e.append((F(-0.5) * v * v).astype(F))
    for c in PLN_FWD_CASES:
        L = PlnFwdLaunch(c, "cpu")
        r.append((L.R["var"] + c["eps"]).astype(F))
    for c in EMBED_CASES[::4]:
        L = EmbedLaunch(c, "cpu")
        r.append((1.0 / L.rstd_in.astype(np.float64) ** 2).astype(F))
    t, e, r = (torch.from_numpy(np.concatenate(a)) for a in (t, e, r))
    return dict(ERF_ULP=ulps_of(torch.erf(t).numpy(), torch.erf(t.double()).numpy()), EXP_ULP=ulps_of(torch.exp(e).numpy(), torch.exp(e.double()).numpy()),
                RSQRT_ULP=ulps_of(torch.rsqrt(r).numpy(), torch.rsqrt(r.double()).numpy()))


# ---- what the old tests let through --------------------------------------------------------------------------------------------------------------------------
# Planted faults (tests/test_cpu_enc_cases.py::FAULTS) that test_embed_postln_meanpool (rel-L2 2e-6 / 1e-5 / 4e-3 at B L = 95) or
# test_adamw_flat_matches_oracle (rtol 2e-6 on p, pb) would have passed, at those tests' shapes, inputs and forms -- either because the norm stays
# under the threshold or because the test never launches the path or reads the output.  test_what_the_old_tests_let_pass computes every figure
# and asserts this list.
NORM_BLIND = ("one_pass_variance", "part_copy_overwritten", "second_row_of_odd_pair_written", "weight_decay_after_the_update", "ema_one_minus_m_in_float32",
              "clip_norm_misses_the_last_partition")
