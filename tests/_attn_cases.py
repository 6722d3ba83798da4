"""The cases of tests/test_{cpu,gpu}_attn_cases.py: every kernel of csrc/attention.hip (the whole-row forward at NKT 2 / 8 / 14 / 18, the paired
forward at NKT 32, the LDS and the L2 form of both backward roles at every blockIdx.y extent the launcher picks, masked and unmasked entry
points, dropout), element by element against float64.  Nothing is stored: every input is rebuilt from its seed, every expected value is
recomputed.  Importing this module launches nothing and does not touch CUDA.

Why element by element: the whole-tensor norms of test_attention_fwd_bwd / test_attention_masked_dropout_fwd_bwd (6e-3 on the output, 1.5e-2
on the gradients) move by 1 / sqrt(rows) when one row is wrong and by far less when one key of one row is.  tests/test_cpu_attn_cases.py
states, fault by fault, what those norms read at the shapes of those tests (NORM_BLIND below lists the planted faults they let pass) and shows
verify() rejecting every one of them.

Inputs.  bf16 operands from a PCG64 stream (Q, K of standard deviation 0.5, V and dO of 1).  In every head Q row i gets a component along K
row pi(i mod key_len), pi a fixed permutation of the valid keys, sized so that this key carries at least DECISIVE = 0.25 of the row's
probability in the float64 reference (asserted for every case by the CPU test): every key is decisive for some output row, so a dropped,
duplicated or permuted key shows far above the bound.  Dimensions 62 and 63 of Q and K are zero except for the spikes: two keys per head
carry one (SPIKE_A in dimension 63 of key s1, which lies in the first 128-key block, SPIKE_B in dimension 62 of key s2, which lies in the
last valid block); query qa = pi^-1(s1) has SPIKE_A in dimension 63, query qb = pi^-1(s2) has both, so its raw score is 64 at s1 and 144
at s2 (80 more): the running maximum of the paired forward moves in a later block, and the raw score of the spiked key is >= 40 above every
other (asserted).  The CPU test walks the float32 restatement over every head of a case of up to six heads and over sample_heads() of the
larger ones (the heads of a case differ only in their draws and key lengths, and every key length is met); the conditions on the inputs are
asserted for every head, and the GPU test checks every head.  The no-trivial-mask assertion counts whole 16 x 16 tiles: a ragged edge tile of
one row or column is all-kept at p = 0.1 with probability 0.9^16 = 0.18.  Every operand lies inside a larger allocation at a
16-byte-aligned non-zero offset; the front and the ROWS_AFTER rows after the last sequence are NaN.  The K and V thirds of padded rows
(key_len[b] <= row < N) hold +-2^12 (garbage 0) or +-6144 in another sign pattern (garbage 1): finite in bf16 and in every product, and the two
launches must agree bit for bit.  Every output starts as NaN inside its block and as the bit pattern PATTERN around it, which must come back.

References (float64, numpy).  Forward: P = softmax(scale Q K^T + key mask), out = (P o keep / (1 - p)) V, lse = max + log-sum of the scaled
masked scores, keep = oracle/bert_ref.keep_mask at the attention site.  Backward: the kernels' formula on the very arrays handed to the kernel:
P = exp(scale S - lse_given), delta = rowsum(dO o out_given), dV = (P o m)^T dO, dP = (dO V^T) o m, dS = P o (dP - delta), dQ = scale dS K,
dK = scale dS^T Q with m = keep / (1 - p), out_given the bf16 rounding of the float64 forward and lse_given its float32 rounding -- the
backward is tested on its own, not behind the forward kernel.  (The CPU test shows the formula equal to float64 autograd of the forward to
1e-12 when out and lse are unrounded, masks and dropout on.)

Bound of an element (never a norm): the first-order propagation, in float64 with absolute values, of the roundings the kernels make.
  forward   scores and softmax statistics fp32; probabilities bf16 into the PV product (row sum over the unrounded values); fp32 accumulation;
            one bf16 rounding of the output:
              out   |got - want| <= tol + half_ulp_bf16(|want| + tol),  tol = sum_k hu(Pm) |V| + F32(C_F32 tau_q) sum_k Pm |V|,
                    tau_q = scale max_k sum_d |q_d k_d| + 1 (the score's accumulation error through the exponential),  Pm = P o m,
                    hu(Pm) = half_ulp_bf16 of the probability as the kernel rounds it, rescaled: exp(S - row max) before 1 / ((1 - p) Z) in the
                    whole-row forward; exp(S - running max of the 128-key blocks so far) in the paired forward, whose later rescaling is fp32
              lse   |got - want| <= F32(C_F32 (1 + |lse| + scale max_k sum_d |q_d k_d|))
  backward  P bf16 into the dV product, dS (scale included) bf16 into the dQ and dK products, everything else fp32, one bf16 rounding:
              T_qk = scale sum_d |q_d k_d| + |lse_q| + 1   (relative fp32 error of the recomputed probability, in units of 2^-24)
              E_qk = P_qk (T_qk |dP_qk - delta_q| + m_qk sum_d |dO_qd v_kd| + sum_d |dO_qd out_qd|)     (fp32 error of dS / scale)
              dV    tol = sum_q half_ulp_bf16(Pm) |dO| + F32(C_BWD) sum_q Pm T |dO|
              dQ    tol = sum_k half_ulp_bf16(scale dS) |K| + scale F32(C_BWD) sum_k E |K|;   dK likewise over q with |Q|
              delta |got - want| <= F32(C_BWD) sum_d |dO out|
  The rounding term of a bf16 operand is half an ulp of that very value: between 2^-9 (top of a binade) and 2^-8 (bottom) of it.  A flat
  2^-9 of the value -- half an ulp only at the top of a binade -- is not a bound: the float32 restatement itself left it (dk[0, 0, 5, 14] of
  nkt2-B2N15H2: 1.170e-3 against 1.154e-3, one dominant dS at the bottom of its binade), so the term is taken per rounded value.
  F32(c) = 2^-24 (c + 4 EXP_ULP): EXP_ULP = 1 is the documented accuracy of v_exp_f32 and v_log_f32 (AMD Instinct CDNA3 / CDNA4 instruction
  set reference, V_EXP_F32 and V_LOG_F32: "1 ULP"; the kernels use the raw instruction, common.h fast_exp2, whose only other deviation is
  flushing results below 2^-126, absorbed by TINY) -- the one operation a CPU cannot restate; 1 ULP = 2 * 2^-24 relative, met once in a
  numerator and once in the row sum.
C_F32 and C_BWD are measured (measure_constants) on the float32 restatements below, which make the kernels' fp32 operations with the
accumulation in 16-key tiles in the kernels' order and in reverse, WITHOUT the bf16 rounding points (those are the 2^-9 terms), against the
float64 reference in units of the fp32 term of each bound; the committed constants are 8 times the measurement, the margin _gemm_cases.py gives
a restatement.  They are never set from what a kernel produced: a kernel outside the bound is a finding.
Exact: entries the mask or the dropout removes are zero (tol = 0 there); dK and dV rows of padded keys are zero, either sign; padding comes
back untouched; launches with different garbage in padded K / V rows agree bit for bit; sequence 0 launched alone gives the bytes it gives in
the batch.

Probability read-out.  With V[k] = e_{k - 64 j} inside key window j and 0 elsewhere, out[q, d] is the dropped, scaled probability Pm[q, 64 j + d];
with dO[q] = e_{q - 64 j}, dV[k, d] = Pm[64 j + d, k] as the BACKWARD regenerates the mask (drop_keep_attn against the forward's inlined hash).
ceil(N / 64) launches read the whole matrix; the same bound applies per element, so dropped and masked entries must be exactly zero, and the
zero sets of both are compared with the oracle's.

The fused block (srhip_attn_block_fused, D = 384, H = 6, N in {257, 197}, B in {1, 3, 9}).  The float64 reference is taken from the bf16 xn,
the bf16 weights and the fp32 bias; q, k and v are rounded to bf16 inside the kernel from fp32 accumulators the test cannot see, so the bound
gains the first-order effect of perturbing every q, k and v element by half a bf16 ulp of itself plus the projection's fp32 accumulation
error (C_ACC of _gemm_cases.py): ds_qk = scale sum_d (dq_d |k_d| + |q_d| dk_d) on a score, carried through the softmax as
P_qk (ds_qk + sum_j P_qj ds_qj), and dv on V.  The kernel walks the keys in chunks of 64 with a running maximum, so the rounding term of the
probabilities sits there (head_probs, block = 64); the unfused pair (srhip_gemm_nt + srhip_attn_fwd) has it at the row maximum, and each of
the two results is held to both bounds.  Every element is checked, row 256 of every image and head (the extra query) like any other.
out_scale is NOT held to that bound (it is ten times what the kernel does): the scaled launch is held against the unscaled launch of the same
operands, half a bf16 ulp of the unrounded value scaled plus half an ulp of the result (verify_out_scale).
Read-out: Wv of head BLOCK_READ_HEAD is a selector of the 64 columns 320 .. 383 of xn, which the q and k weights (and the other heads' v
weights) ignore; xn carries e_{k - 64 j} there for the keys of window j, so that head's output is the probability matrix itself -- done for the
window that holds key 256."""
import functools
import math

import numpy as np
import torch

from oracle import bert_ref as BR
from semireward_amd import ops

# measured by measure_constants() over CASES, either accumulation order (tests/test_cpu_attn_cases.py holds each constant between 4 and 16 times
# its measurement): largest |float32 restatement without bf16 points - float64| in units of 2^-24 x the fp32 term of the bound
C_F32_MEASURED, C_BWD_MEASURED = 2.624, 1.691
C_F32, C_BWD = 8.0 * C_F32_MEASURED, 8.0 * C_BWD_MEASURED
EXP_ULP = 1.0
TINY = 1e-36                         # absolute: v_exp_f32 flushes results below 2^-126

SCALE = 0.125
HD = 64
FRONT, FRONT_F32, ROWS_AFTER = 8, 4, 3      # 16 bytes before the block (bf16 / fp32 elements), rows after the last sequence
PATTERN = 0x4B1D                             # every 16 bits of the output padding: finite as bf16 and as fp32 (0x4B1D4B1D)
DECISIVE = 0.25
SPIKE_A, SPIKE_B = 8.0, 12.0
DROP_SITE = 4 * 3 + BR.SITE_PROBS            # the attention site of layer 3
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453


def F32(c):
    return 2.0 ** -24 * (c + 4.0 * EXP_ULP)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
def key_lens(N, B=None):
    """key_len[0] = N, then {1, 15, 16, 17, 127, 128, 129, N - 1} cut to [1, N), one per sequence (cycled when B is given)."""
    rest = sorted({x for x in (1, 15, 16, 17, 127, 128, 129, N - 1) if 1 <= x < N})
    kl = [N] + rest
    return tuple(kl if B is None else [kl[i % len(kl)] for i in range(B)])


def _case(what, B, N, H, *, masked=False, p=0.0, dseed=0, plan=None, forms=("fwd", "bwd"), seed=0):
    kl = key_lens(N, B if masked == "cycle" else None) if masked else None
    if kl is not None:
        B = len(kl)
    assert plan is not None, "a case names the kernel and grid it means to reach"
    cid = "%s-B%dN%dH%d%s%s" % (what, B, N, H, "-kl" if masked else "", ("-p%g-s%d" % (p, dseed)) if p else "")
    return dict(id=cid, what=what, B=B, N=N, H=H, key_len=kl, var=bool(masked) or p > 0, p=p, dseed=(77 << 32) + 1000 * dseed + N,
                plan=plan, forms=tuple(forms), seed=seed + 131 * N + 7 * B + H)


def _P(nkt, pair, split):
    return ops.AttnPlan(nkt, pair, pair, split)


CASES = (
    # whole-row forward, unmasked entry points (VAR = false: "tiles below the previous size are complete"): first and last N of every
    # instantiation, one tile +- 1; N < 113 leaves waves without a tile; B*H >= 9 once per instantiation (the tile -> wave map rotates)
    _case("nkt2", 1, 1, 1, plan=_P(2, False, 1)),
    _case("nkt2", 2, 15, 2, plan=_P(2, False, 1)),
    _case("nkt2", 1, 16, 3, plan=_P(2, False, 1)),
    _case("nkt2", 3, 17, 3, plan=_P(2, False, 1), forms=("fwd", "fwd_nolse", "bwd")),
    _case("nkt2", 1, 32, 1, plan=_P(2, False, 1)),
    _case("nkt8", 2, 33, 1, plan=_P(8, False, 1)),
    _case("nkt8", 1, 64, 2, plan=_P(8, False, 1)),
    _case("nkt8", 3, 127, 3, plan=_P(8, False, 1), forms=("fwd", "fwd_nolse", "bwd")),
    _case("nkt8", 1, 128, 1, plan=_P(8, False, 1)),
    _case("nkt14", 1, 129, 2, plan=_P(14, False, 2)),
    _case("nkt14", 3, 197, 3, plan=_P(14, False, 2), forms=("fwd", "fwd_nolse", "bwd")),
    _case("nkt14", 1, 224, 1, plan=_P(14, False, 2)),
    _case("nkt18", 1, 225, 1, plan=_P(18, False, 2)),
    _case("nkt18", 3, 257, 3, plan=_P(18, False, 3), forms=("fwd", "fwd_nolse", "bwd")),
    _case("nkt18", 1, 288, 2, plan=_P(18, False, 3)),
    # paired forward and the L2 backward, unmasked: 289 = a second round whose partner tile is past the end; 384 = exactly three 128-key
    # blocks; 385 = one more block with one key
    _case("nkt32", 1, 289, 1, plan=_P(32, True, 3)),
    _case("nkt32", 1, 384, 2, plan=_P(32, True, 3)),
    _case("nkt32", 3, 385, 3, plan=_P(32, True, 4), forms=("fwd", "fwd_nolse", "bwd")),
    _case("nkt32", 1, 511, 1, plan=_P(32, True, 4)),
    _case("nkt32", 1, 512, 2, plan=_P(32, True, 4)),
    # masked entry points: key_len per sequence in {N, 1, 15, 16, 17, 127, 128, 129, N - 1}
    _case("masked", 0, 17, 1, masked=True, plan=_P(2, False, 1)),
    _case("masked", 0, 64, 2, masked=True, plan=_P(8, False, 1), forms=("fwd", "fwd_nolse", "bwd")),
    _case("masked", 0, 197, 1, masked=True, plan=_P(14, False, 2)),
    _case("masked", 0, 257, 1, masked=True, plan=_P(18, False, 3), forms=("fwd", "fwd_nolse", "bwd")),
    _case("masked", 0, 300, 2, masked=True, plan=_P(32, True, 3)),
    _case("masked", 0, 512, 1, masked=True, plan=_P(32, True, 4), forms=("fwd", "fwd_nolse", "bwd")),
    # dropout (the masked entry with key_len = NULL, and with key lengths): odd N has ceil(N / 2) pairs per row
    _case("drop", 2, 64, 1, p=0.1, dseed=1, plan=_P(8, False, 1), forms=("fwd", "bwd", "readout")),
    _case("drop", 0, 64, 1, masked=True, p=0.5, dseed=2, plan=_P(8, False, 1)),
    _case("drop", 1, 257, 2, p=0.5, dseed=1, plan=_P(18, False, 3)),
    _case("drop", 0, 257, 1, masked=True, p=0.1, dseed=2, plan=_P(18, False, 3), forms=("fwd", "bwd", "readout")),
    _case("drop", 2, 401, 1, p=0.1, dseed=1, plan=_P(32, True, 4)),
    _case("drop", 0, 401, 1, masked=True, p=0.5, dseed=2, plan=_P(32, True, 4)),
    _case("drop", 1, 512, 2, p=0.5, dseed=1, plan=_P(32, True, 4)),
    _case("drop", 0, 512, 1, masked=True, p=0.1, dseed=2, plan=_P(32, True, 4), forms=("fwd", "bwd", "readout")),
    # backward grids.  LDS form: 257 at B*H = 66 / 32 / 9 (split 1 / 2 / 3: at split 1 every wave walks several rounds of tile pairs),
    # 197 at 64 / 12, N <= 128 alone (waves without a tile)
    _case("bwd_lds", 11, 257, 6, plan=_P(18, False, 1)),
    _case("bwd_lds", 16, 257, 2, plan=_P(18, False, 2), forms=("bwd",)),
    _case("bwd_lds", 3, 257, 3, masked="cycle", p=0.1, dseed=3, plan=_P(18, False, 3), forms=("bwd",)),
    _case("bwd_lds", 16, 197, 4, plan=_P(14, False, 1), forms=("bwd",)),
    _case("bwd_lds", 4, 197, 3, plan=_P(14, False, 2), forms=("bwd",)),
    _case("bwd_lds", 1, 100, 1, plan=_P(8, False, 1), forms=("bwd",)),
    # L2 form: 512 at B*H = 64 / 32 / 1 (split 1 / 2 / 4), 289 at 64 / 32 / 1 (split 1 / 2 / 3); masked with dropout at split 1
    _case("bwd_l2", 16, 512, 4, masked="cycle", p=0.1, dseed=4, plan=_P(32, True, 1)),
    _case("bwd_l2", 16, 512, 2, plan=_P(32, True, 2), forms=("bwd",)),
    _case("bwd_l2", 1, 512, 1, masked="cycle", p=0.1, dseed=5, plan=_P(32, True, 4), forms=("bwd",)),
    _case("bwd_l2", 16, 289, 4, masked="cycle", p=0.1, dseed=6, plan=_P(32, True, 1), forms=("bwd",)),
    _case("bwd_l2", 16, 289, 2, plan=_P(32, True, 2), forms=("bwd",)),
    _case("bwd_l2", 1, 289, 1, masked="cycle", p=0.1, dseed=7, plan=_P(32, True, 3), forms=("bwd",)),
)
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)
CASE_FORMS = tuple((c["id"], f) for c in CASES for f in c["forms"])


def kernel_name(c, form):
    if form.startswith("fwd") or form == "readout":
        return "attn_fwd_pair_kernel<%s>" % c["var"] if c["plan"].fwd_pair else "attn_fwd_kernel<%d, %s>" % (c["plan"].nkt, c["var"])
    return "attn_bwd_kernel<%d, %s, %s> grid.y=%d" % (c["plan"].nkt, c["var"], c["plan"].bwd_l2, c["plan"].bwd_split)


# ---- number formats ------------------------------------------------------------------------------------------------------------------------
def bf16(x):
    """Nearest-even bf16 rounding of a float array, returned as float64."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).double().numpy()


def bf16_f32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def half_ulp_bf16(x):
    """Half a unit in the last place of bf16 (8 significant bits) at magnitude x; 0 at 0."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    e = np.frexp(x)[1] - 1                                 # floor(log2 x) for x > 0
    return np.where(x > 0, np.ldexp(1.0, np.maximum(e, -126) - 8), 0.0)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def keep_of(c):
    """Boolean keep mask [B, H, N, N] of the case (None without dropout) and its ops.Drop."""
    if not c["p"]:
        return None, None
    return BR.keep_mask(c["dseed"], DROP_SITE, (c["B"], c["H"], c["N"], c["N"]), c["p"]), ops.Drop(c["dseed"], DROP_SITE, c["p"])


def make_inputs(c, garbage=0, gaussian=None):
    """q, k, v, do: float64 arrays [B, H, N, 64] of bf16 values; klen int [B]; pi [B, H, N]; spikes [(b, h, qa, s1, qb, s2)].
    gaussian = s: plain N(0, s^2) operands (the inputs of the norm tests; no decisive keys, no spikes)."""
    B, N, H = c["B"], c["N"], c["H"]
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    klen = np.array(c["key_len"] if c["key_len"] is not None else [N] * B, dtype=np.int64)
    if gaussian is not None:
        q, k, v = (gaussian * rng.standard_normal((B, H, N, HD)) for _ in range(3))
        do = rng.standard_normal((B, H, N, HD))
        return dict(q=bf16(q), k=bf16(k), v=bf16(v), do=bf16(do), klen=klen, pi=None, spikes=[])
    q, k = 0.5 * rng.standard_normal((B, H, N, HD)), 0.5 * rng.standard_normal((B, H, N, HD))
    v, do = rng.standard_normal((B, H, N, HD)), rng.standard_normal((B, H, N, HD))
    q[..., 62:], k[..., 62:] = 0.0, 0.0                    # dimensions 62 and 63 belong to the spikes: no other row sees them
    pi = np.zeros((B, H, N), dtype=np.int64)
    spikes = []
    x = (math.log(N) + 1.5) / SCALE                       # raw score the component adds at key pi(i)
    for b in range(B):
        L = int(klen[b])
        for h in range(H):
            perm = rng.permutation(L)
            pi[b, h] = perm[np.arange(N) % L]
            sp = None
            if L >= 4:
                s1 = int(rng.integers(0, min(L, 128)))
                lo = (L - 1) // 128 * 128
                s2 = int(rng.integers(lo, L))
                if s2 == s1:
                    s2 = lo + (s1 - lo + 1) % (L - lo) if L - lo > 1 else (s1 + 1) % L
                qa, qb = int(np.nonzero(perm == s1)[0][0]), int(np.nonzero(perm == s2)[0][0])
                k[b, h, s1, 63], k[b, h, s2, 62] = SPIKE_A, SPIKE_B
                sp = (b, h, qa, s1, qb, s2)
            kk = k[b, h, pi[b, h]]
            q[b, h] += x * kk / (kk * kk).sum(-1, keepdims=True)
            if sp:
                q[b, h, qa, 63] = SPIKE_A
                q[b, h, qb, 63], q[b, h, qb, 62] = SPIKE_A, SPIKE_B
                spikes.append(sp)
    q, k, v, do = bf16(q), bf16(k), bf16(v), bf16(do)
    fill_garbage(k, v, klen, garbage)
    return dict(q=q, k=k, v=v, do=do, klen=klen, pi=pi, spikes=spikes)


def fill_garbage(k, v, klen, garbage):
    """Padded rows of K and V: +-2^12 (garbage 0) or +-6144 in another sign pattern (garbage 1)."""
    B, H, N, _ = k.shape
    d = np.arange(HD)
    for b in range(B):
        L = int(klen[b])
        if L < N:
            r = np.arange(L, N)[:, None]
            sign = np.where((r + d) % 2 == 0, 1.0, -1.0) if garbage == 0 else np.where((r // 2 + d // 3) % 2 == 0, -1.0, 1.0)
            k[b, :, L:] = (4096.0 if garbage == 0 else 6144.0) * sign
            v[b, :, L:] = (4096.0 if garbage == 0 else 6144.0) * -sign


def readout_v(c, inp, j):
    """V of key window j: V[k] = e_{k - 64 j} inside the window, 0 elsewhere (padded rows keep their garbage)."""
    v = np.zeros_like(inp["v"])
    for kk in range(64 * j, min(64 * j + 64, c["N"])):
        v[:, :, kk, kk - 64 * j] = 1.0
    fill_garbage(np.zeros_like(v), v, inp["klen"], 0)
    return v


def readout_do(c, inp, j):
    do = np.zeros_like(inp["do"])
    for qq in range(64 * j, min(64 * j + 64, c["N"])):
        do[:, :, qq, qq - 64 * j] = 1.0
    return do


# ---- float64 references and bounds --------------------------------------------------------------------------------------------------------
def head_probs(q, k, L, keep, p, block=None):
    """One head: P [N, L] over the valid keys, Pm = P o keep / (1 - p), lse, aS = scale |Q| |K|^T, S; hu = the half ulp of every probability
    at its rounding point, rescaled to Pm (block = 128: the paired forward, which rounds exp(S - running max) block by block)."""
    S = SCALE * (q @ k[:L].T)
    aS = SCALE * (np.abs(q) @ np.abs(k[:L]).T)
    m = S.max(1)
    E = np.exp(S - m[:, None])
    Z = E.sum(1)
    P = E / Z[:, None]
    M = keep[:, :L] / (1.0 - p) if keep is not None else None
    # the kernels round the unnormalised exp(S - max), kept elements only, and scale the accumulated row by 1 / ((1 - p) Z) afterwards
    if block is None:
        hu = half_ulp_bf16(E)
    else:
        run = np.maximum.accumulate(np.stack([S[:, i:i + block].max(1) for i in range(0, L, block)]), axis=0)      # [blocks, N]
        mr = run.T[:, np.arange(L) // block]
        hu = half_ulp_bf16(np.exp(S - mr)) * np.exp(mr - m[:, None])
    hu = hu / Z[:, None] * (M if M is not None else 1.0)
    return dict(S=S, aS=aS, P=P, Pm=P * M if M is not None else P, M=M, lse=m + np.log(Z), hu=hu)


def head_fwd(q, k, v, L, keep, p, block=None):
    r = head_probs(q, k, L, keep, p, block)
    amax = r["aS"].max(1)
    A = r["Pm"] @ np.abs(v[:L])
    r["out"] = r["Pm"] @ v[:L]
    r["out_f32"] = (amax + 1.0)[:, None] * A              # x F32(C_F32): the fp32 term of the bound, in units the constants are measured in
    r["out_bf"] = (r["hu"] @ np.abs(v[:L]))               # the probabilities' bf16 rounding: half an ulp of each one as it is rounded
    r["out_tol"] = r["out_bf"] + F32(C_F32 * (amax + 1.0))[:, None] * A + TINY * (A > 0)
    r["lse_f32"] = 1.0 + np.abs(r["lse"]) + amax
    r["lse_tol"] = F32(C_F32 * r["lse_f32"])
    return r


def head_bwd(q, k, v, do, out_g, lse_g, L, keep, p):
    """The kernels' backward formula in float64 on the given arrays; rows of padded keys are zero with bound zero."""
    N = q.shape[0]
    S = SCALE * (q @ k[:L].T)
    aS = SCALE * (np.abs(q) @ np.abs(k[:L]).T)
    P = np.exp(S - lse_g[:, None])
    M = keep[:, :L] / (1.0 - p) if keep is not None else 1.0
    Pm = P * M
    delta, aD = (do * out_g).sum(1), (np.abs(do) * np.abs(out_g)).sum(1)
    dPm = (do @ v[:L].T) * M
    aA = (np.abs(do) @ np.abs(v[:L]).T) * M
    dS = P * (dPm - delta[:, None])
    T = aS + np.abs(lse_g)[:, None] + 1.0
    E = P * (T * np.abs(dPm - delta[:, None]) + aA + aD[:, None])
    ado, ak, aq, adS = np.abs(do), np.abs(k[:L]), np.abs(q), np.abs(dS)
    z = np.zeros((N, HD))
    hS, hP = half_ulp_bf16(SCALE * dS), half_ulp_bf16(Pm)  # dS is rounded with scale on it, P with the dropout scale on it
    r = dict(delta=delta, delta_f32=aD, dq=SCALE * (dS @ k[:L]), dq_bf=hS @ ak, dq_f32=SCALE * (E @ ak), dk=z.copy(), dk_bf=z.copy(),
             dk_f32=z.copy(), dv=z.copy(), dv_bf=z.copy(), dv_f32=z.copy())
    r["dk"][:L], r["dk_bf"][:L], r["dk_f32"][:L] = SCALE * (dS.T @ q), hS.T @ aq, SCALE * (E.T @ aq)
    r["dv"][:L], r["dv_bf"][:L], r["dv_f32"][:L] = Pm.T @ do, hP.T @ ado, (Pm * T).T @ ado
    for n in ("dq", "dk", "dv"):
        r[n + "_tol"] = r[n + "_bf"] + F32(C_BWD) * r[n + "_f32"] + TINY * (r[n + "_f32"] > 0)
    r["delta_tol"] = F32(C_BWD) * aD
    r["Pm"] = Pm
    r["Pm_tol"] = hP + F32(C_BWD) * Pm * T + TINY * (Pm > 0)
    return r


FWD_KEYS = ("out", "out_tol", "out_f32", "lse", "lse_tol", "lse_f32")
BWD_KEYS = ("delta", "delta_tol", "delta_f32") + tuple(n + s for n in ("dq", "dk", "dv") for s in ("", "_tol", "_f32"))


def _stack(c, fn, keys):
    B, H = c["B"], c["H"]
    res = [[fn(b, h) for h in range(H)] for b in range(B)]
    return {key: np.stack([np.stack([res[b][h][key] for h in range(H)]) for b in range(B)]) for key in keys}


def reference_fwd(c, inp, keep, v=None):
    """out [B, H, N, 64], lse [B, H, N] and their bounds; out_given (bf16 of out) and lse_given (float32 of lse) for the backward."""
    v = inp["v"] if v is None else v
    r = _stack(c, lambda b, h: head_fwd(inp["q"][b, h], inp["k"][b, h], v[b, h], int(inp["klen"][b]), None if keep is None else keep[b, h],
                                        c["p"], 128 if c["plan"].fwd_pair else None), FWD_KEYS)
    r["out_given"], r["lse_given"] = bf16(r["out"]), r["lse"].astype(np.float32).astype(np.float64)
    return r


def reference_bwd(c, inp, keep, fwd, do=None):
    do = inp["do"] if do is None else do
    return _stack(c, lambda b, h: head_bwd(inp["q"][b, h], inp["k"][b, h], inp["v"][b, h], do[b, h], fwd["out_given"][b, h],
                                           fwd["lse_given"][b, h], int(inp["klen"][b]), None if keep is None else keep[b, h], c["p"]), BWD_KEYS)


@functools.lru_cache(maxsize=2)
def case_reference(cid):
    """Inputs, keep mask and both references of a case (shared by the forms of the case; treat as read-only)."""
    c = BY_ID[cid]
    inp = make_inputs(c)
    keep, drop = keep_of(c)
    fwd = reference_fwd(c, inp, keep)
    bwd = reference_bwd(c, inp, keep, fwd)
    return dict(c=c, inp=inp, keep=keep, drop=drop, fwd=fwd, bwd=bwd)


def readout_reference(c, inp, keep, fwd):
    """The dropped, scaled probability matrices [B, H, N, N] (zero at masked keys) with their per-element tolerances: as the forward makes
    them (softmax) and as the backward regenerates them (exp(S - lse_given)); zero [B, H, N, N] = the oracle's zero set."""
    B, H, N = c["B"], c["H"], c["N"]
    r = {n: np.zeros((B, H, N, N)) for n in ("fwd", "fwd_tol", "bwd", "bwd_tol")}
    r["zero"] = np.ones((B, H, N, N), dtype=bool)
    for b in range(B):
        L = int(inp["klen"][b])
        for h in range(H):
            kp = None if keep is None else keep[b, h]
            f = head_probs(inp["q"][b, h], inp["k"][b, h], L, kp, c["p"], 128 if c["plan"].fwd_pair else None)
            amax = f["aS"].max(1)
            r["fwd"][b, h, :, :L] = f["Pm"]
            r["fwd_tol"][b, h, :, :L] = f["hu"] + F32(C_F32 * (amax + 1.0))[:, None] * f["Pm"] + TINY * (f["Pm"] > 0)
            w = head_bwd(inp["q"][b, h], inp["k"][b, h], inp["v"][b, h], inp["do"][b, h], fwd["out_given"][b, h], fwd["lse_given"][b, h], L, kp,
                         c["p"])
            r["bwd"][b, h, :, :L], r["bwd_tol"][b, h, :, :L] = w["Pm"], w["Pm_tol"]
            r["zero"][b, h, :, :L] = ~kp[:, :L] if kp is not None else False
    return r


def readout_window(mat, j, transpose=False):
    """What a read-out launch of window j returns, [B, H, N, 64]: out[q, d] = mat[q, 64 j + d]; (transpose) dV[k, d] = mat[64 j + d, k]."""
    B, H, N, _ = mat.shape
    w = np.zeros((B, H, N, HD), dtype=mat.dtype)
    n = min(64, N - 64 * j)
    w[..., :n] = mat[:, :, 64 * j:64 * j + n, :].transpose(0, 1, 3, 2) if transpose else mat[:, :, :, 64 * j:64 * j + n]
    return w


def decisive_mass(c, inp, keep=None):
    """Smallest probability, over all query rows of the case, of the key the row was built to depend on; and the smallest margin of a spiked
    raw score over the row's other raw scores."""
    least, margin = 1.0, np.inf
    for b in range(c["B"]):
        L = int(inp["klen"][b])
        for h in range(c["H"]):
            P = head_probs(inp["q"][b, h], inp["k"][b, h], L, None, 0.0)["P"]
            least = min(least, float(P[np.arange(c["N"]), inp["pi"][b, h]].min()))
    for b, h, qa, s1, qb, s2 in inp["spikes"]:
        L = int(inp["klen"][b])
        raw = inp["q"][b, h] @ inp["k"][b, h, :L].T
        for qq, s in ((qa, s1), (qb, s2)):
            margin = min(margin, float(raw[qq, s] - np.delete(raw[qq], s).max())) if L > 1 else margin
    return least, margin


# ---- verify --------------------------------------------------------------------------------------------------------------------------------
def where_is(name, idx):
    """Which head, 16-row tile, MFMA lane and lane group own element idx = ([b, h,] row, d) of a [..., N, 64] array ((.., row) of lse / delta_ws)."""
    vec = name in ("lse", "delta_ws")
    row, bh = (idx[-1], idx[:-1]) if vec else (idx[-2], idx[:-2])
    s = ("sequence %d head %d " % tuple(bh) if len(bh) == 2 else "") + "row %d = tile %d lane l15 %d" % (row, row // 16, row % 16)
    return s if vec else s + ", d %d = d-tile %d lane group g %d register %d" % (idx[-1], idx[-1] // 16, (idx[-1] % 16) // 4, idx[-1] % 4)


def verify(kernel, name, got, want, tol, rounded=True, where=None):
    """Every element of got inside its bound: |got - want| <= tol + half_ulp_bf16(|want| + tol) (rounded) or tol.  Returns the largest
    |got - want| / bound over the elements with a non-zero bound; raises AssertionError naming the worst element otherwise."""
    got, want, tol = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(tol, dtype=np.float64)
    assert got.shape == want.shape == tol.shape, (name, got.shape, want.shape, tol.shape)
    bound = tol + half_ulp_bf16(np.abs(want) + tol) if rounded else tol
    err = np.abs(got - want)
    bad = ~(err <= bound)                                  # NaN (an element never written) is bad
    if bad.any():
        score = np.where(bad, np.where(np.isfinite(err), err / np.maximum(bound, 1e-300), np.inf), -1.0)
        idx = tuple(int(i) for i in np.unravel_index(int(np.argmax(score)), got.shape))
        raise AssertionError("%s: %s%s got %r want %r |diff| %.3e bound %.3e (%d of %d elements outside); %s" % (
            kernel, name, list(idx), float(got[idx]), float(want[idx]), float(err[idx]), float(bound[idx]), int(bad.sum()), bad.size,
            where(idx) if where is not None else where_is(name, idx)))
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def verify_fwd(kernel, got_out, got_lse, ref):
    r = {"out": verify(kernel, "out", got_out, ref["out"], ref["out_tol"])}
    if got_lse is not None:
        r["lse"] = verify(kernel, "lse", got_lse, ref["lse"], ref["lse_tol"], rounded=False)
    return r


def verify_bwd(kernel, got, ref):
    """got: dict dq, dk, dv [B, H, N, 64], delta [B, H, N]."""
    r = {n: verify(kernel, n, got[n], ref[n], ref[n + "_tol"]) for n in ("dq", "dk", "dv")}
    r["delta"] = verify(kernel, "delta_ws", got["delta"], ref["delta"], ref["delta_tol"], rounded=False)
    return r


# ---- float32 restatements (the kernels' fp32 operations and rounding points on the CPU) ---------------------------------------------------
_f = np.float32
SC2 = _f(_f(SCALE) * _f(LOG2E))


def _raw_scores(a, b, reverse):
    a, b = a.astype(_f), b.astype(_f)
    lo, hi = a[:, :32] @ b[:, :32].T, a[:, 32:] @ b[:, 32:].T
    return (hi + lo) if reverse else (lo + hi)


def _tiles(n, reverse, step=16):
    t = [slice(i, min(i + step, n)) for i in range(0, n, step)]
    return t[::-1] if reverse else t


def _rb(x, on):
    return bf16_f32(x) if on else x


def restate_fwd(q, k, v, L, keep, p, *, points=True, reverse=False, block=None, fault=None, osc=1.0):
    """One head in float32.  points: the bf16 rounding points (probabilities, output); block = 128: the online softmax of the paired forward.
    fault: a planted fault (tests/test_cpu_attn_cases.py).  Returns out [N, 64], lse [N] as float64 arrays of the float32 / bf16 values."""
    N = q.shape[0]
    fault = fault or (None,)
    s = _raw_scores(q, k[:L], reverse)
    if fault[0] == "drop_key":
        s[fault[1], fault[2]] = -np.inf
    vv = v[:L].astype(_f).copy()
    if fault[0] == "swap_v":
        vv[[fault[1], fault[2]]] = vv[[fault[2], fault[1]]]
    kp = np.ones((N, L), dtype=_f) if keep is None else keep[:, :L].astype(_f)
    dscale = _f(1.0 / (1.0 - p)) if keep is not None else _f(1.0)
    o, sm, mx = np.zeros((N, HD), dtype=_f), np.zeros(N, dtype=_f), np.full(N, -np.inf, dtype=_f)
    blocks = [slice(0, L)] if block is None else _tiles(L, False, block)
    bm = mx
    for bs in blocks:
        sb = s[:, bs]
        bm = sb.max(1)
        mn = np.maximum(mx, bm)
        with np.errstate(invalid="ignore"):
            alpha = np.where(np.isfinite(mx), np.exp2((mx - mn) * SC2), _f(0.0)).astype(_f)
        mx = mn
        sm, o = sm * alpha, o * alpha[:, None]
        e = np.exp2(sb * SC2 + (-mn * SC2)[:, None]).astype(_f)
        eb = _rb(e * kp[:, bs], points)
        for t in _tiles(sb.shape[1], reverse):
            sm = sm + (bf16_f32(e[:, t]) if fault[0] == "sum_after_rounding" else e[:, t]).sum(1, dtype=_f)
            o = o + eb[:, t] @ vv[bs][t]
    out = _rb(o * (dscale * _f(osc) / sm)[:, None], points)            # (the block kernel: inv = osc / sum)
    top = bm if fault[0] == "block_max_lse" else mx
    lse = (top * SC2 + np.log2(sm)) * _f(LN2)
    return out.astype(np.float64), lse.astype(np.float64)


def restate_bwd(q, k, v, do, out_g, lse_g, L, keep, p, *, points=True, reverse=False, fault=None):
    """One head of both backward roles in float32: dq, dk, dv [N, 64] (rows of padded keys zero), delta [N]."""
    N = q.shape[0]
    fault = fault or (None,)
    s = _raw_scores(q, k[:L], reverse)
    dp = _raw_scores(do, v[:L], reverse)
    d32, o32 = do.astype(_f), out_g.astype(_f)
    prod = d32 * o32
    dl = (prod[:, ::-1] if reverse else prod).sum(1, dtype=_f)
    if fault[0] == "delta":
        dl = fault[1].astype(_f)
    pm = np.exp2(s * SC2 - (lse_g.astype(_f) * _f(LOG2E))[:, None]).astype(_f)
    kp = np.ones((N, L), dtype=_f) if keep is None else keep[:, :L].astype(_f)
    dscale = _f(1.0 / (1.0 - p)) if keep is not None else _f(1.0)
    ds = _rb(pm * (dp * dscale * kp - dl[:, None]) * (_f(1.0) if fault[0] == "no_scale" else _f(SCALE)), points)
    ds_k = _rb(pm * (dp * dscale * kp - dl[:, None]) * _f(SCALE), points)
    pk = _rb(pm * dscale * kp, points)
    k32, q32 = k[:L].astype(_f), q.astype(_f)
    dq, dk, dv = np.zeros((N, HD), dtype=_f), np.zeros((N, HD), dtype=_f), np.zeros((N, HD), dtype=_f)
    for t in _tiles(L, reverse):
        dq = dq + ds[:, t] @ k32[t]
    for t in _tiles(N, reverse):
        dk[:L] = dk[:L] + ds_k[t].T @ q32[t]
        dv[:L] = dv[:L] + pk[t].T @ d32[t]
    return dict(dq=_rb(dq, points).astype(np.float64), dk=_rb(dk, points).astype(np.float64), dv=_rb(dv, points).astype(np.float64),
                delta=dl.astype(np.float64))


def restate_case(c, inp, keep, fwd, *, points=True, reverse=False, heads=None):
    """Both restatements over the heads of a case (heads: a list of (b, h), default all): arrays shaped like the references, NaN elsewhere."""
    B, H, N = c["B"], c["H"], c["N"]
    r = {n: np.full((B, H, N, HD), np.nan) for n in ("out", "dq", "dk", "dv")}
    r.update({n: np.full((B, H, N), np.nan) for n in ("lse", "delta")})
    for b, h in (heads if heads is not None else [(b, h) for b in range(B) for h in range(H)]):
        L, kp = int(inp["klen"][b]), None if keep is None else keep[b, h]
        r["out"][b, h], r["lse"][b, h] = restate_fwd(inp["q"][b, h], inp["k"][b, h], inp["v"][b, h], L, kp, c["p"], points=points,
                                                     reverse=reverse, block=128 if c["plan"].fwd_pair else None)
        g = restate_bwd(inp["q"][b, h], inp["k"][b, h], inp["v"][b, h], inp["do"][b, h], fwd["out_given"][b, h], fwd["lse_given"][b, h], L, kp,
                        c["p"], points=points, reverse=reverse)
        for n in g:
            r[n][b, h] = g[n]
    return r


def sample_heads(c, n=6):
    """The heads the CPU restatement walks: all of them up to n; else one head of each of the first nine sequences when the case has key
    lengths (the lengths cycle with period <= 9, so every one is met), n spread evenly otherwise.  The heads of a case differ only in their
    draws and key lengths."""
    allh = [(b, h) for b in range(c["B"]) for h in range(c["H"])]
    if len(allh) <= n:
        return allh
    if c["key_len"] is not None:
        return [(b, (b * 5) % c["H"]) for b in range(min(c["B"], 9))]
    return [allh[round(i * (len(allh) - 1) / (n - 1))] for i in range(n)]


def measure_constants(cases=CASES):
    """Largest fp32-only restatement error in units of 2^-24 x the fp32 term of each bound: (forward, backward)."""
    cf, cb = 0.0, 0.0
    for c in cases:
        inp = make_inputs(c)
        keep, _ = keep_of(c)
        heads = sample_heads(c, 3)
        for b, h in heads:
            L, kp = int(inp["klen"][b]), None if keep is None else keep[b, h]
            a = (inp["q"][b, h], inp["k"][b, h], inp["v"][b, h])
            f = head_fwd(*a, L, kp, c["p"], 128 if c["plan"].fwd_pair else None)
            og, lg = bf16(f["out"]), f["lse"].astype(np.float32).astype(np.float64)
            w = head_bwd(*a, inp["do"][b, h], og, lg, L, kp, c["p"])
            for rev in (False, True):
                o, l = restate_fwd(*a, L, kp, c["p"], points=False, reverse=rev, block=128 if c["plan"].fwd_pair else None)
                cf = max(cf, _units(o, f["out"], f["out_f32"]), _units(l, f["lse"], f["lse_f32"]))
                g = restate_bwd(*a, inp["do"][b, h], og, lg, L, kp, c["p"], points=False, reverse=rev)
                cb = max(cb, max(_units(g[n], w[n], w[n + "_f32"]) for n in ("dq", "dk", "dv", "delta")))
    return cf, cb


def _units(got, want, term):
    nz = term > 0
    assert np.array_equal(got[~nz], want[~nz])
    return float((np.abs(got - want)[nz] / (2.0 ** -24 * term[nz])).max()) if nz.any() else 0.0


# ---- launches (GPU tests only; nothing above touches CUDA) ---------------------------------------------------------------------------------
def _pack(x):
    """[B, H, N, 64] -> [B * N, H * 64]."""
    B, H, N, _ = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(B * N, H * HD)


def _unpack(x, B, N, H):
    return x.reshape(B, N, H, HD).transpose(0, 2, 1, 3)


class Buf:
    """A [rows, cols] block inside a larger allocation: `front` elements before it, ROWS_AFTER rows after it.  Operands: block = the values,
    padding NaN.  Outputs: block NaN, padding PATTERN."""

    def __init__(self, dev, rows, cols, dtype, values=None):
        front = FRONT if dtype == torch.bfloat16 else FRONT_F32
        n = front + (rows + ROWS_AFTER) * cols
        self.rows, self.cols, self.front, self.dtype = rows, cols, front, dtype
        if values is not None:
            flat = torch.full((n,), float("nan"), dtype=dtype)
            flat[front:front + rows * cols] = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).reshape(-1).to(dtype)
        else:
            words = torch.full((n * (2 if dtype == torch.float32 else 1),), PATTERN, dtype=torch.int16)
            flat = words.view(dtype).clone()
            flat[front:front + rows * cols] = float("nan")
        self.flat = flat.to(dev)
        self.block = self.flat[front:front + rows * cols].view(rows, cols)
        assert self.block.data_ptr() % 16 == 0 and self.block.data_ptr() != self.flat.data_ptr()

    def padding_untouched(self):
        w = self.flat.cpu().view(torch.int16)
        per = 2 if self.dtype == torch.float32 else 1
        pad = torch.cat([w[:self.front * per], w[(self.front + self.rows * self.cols) * per:]])
        return bool((pad == PATTERN).all())

    def bits(self):
        return self.block.cpu().contiguous().view(torch.int16 if self.dtype == torch.bfloat16 else torch.int32).numpy().copy()

    def values(self):
        return self.block.double().cpu().numpy()


def qkv_rows(inp, v=None):
    return np.concatenate([_pack(inp["q"]), _pack(inp["k"]), _pack(inp["v"] if v is None else v)], axis=1)      # [B * N, 3 D]: q | k | v


def launch_fwd(c, dev, inp, drop, *, v=None, with_lse=True, B=None):
    """One forward launch through the C ABI (B: only the first B sequences).  Returns the output buffers."""
    B = c["B"] if B is None else B
    N, H = c["N"], c["H"]
    qkv = Buf(dev, c["B"] * N, 3 * H * HD, torch.bfloat16, qkv_rows(inp, v))
    out = Buf(dev, B * N, H * HD, torch.bfloat16)
    lse = Buf(dev, B * H, N, torch.float32) if with_lse else None
    if c["var"]:
        kl = torch.from_numpy(inp["klen"][:B].astype(np.int32)).to(dev) if c["key_len"] is not None else None
        ops.attn_masked_fwd(qkv.block, out.block, lse.block if lse else None, kl, B, N, H, SCALE, drop)
    else:
        ops.attn_fwd(qkv.block, out.block, lse.block if lse else None, B, N, H, SCALE)
    torch.cuda.synchronize()
    return out, lse


def launch_bwd(c, dev, inp, drop, fwd, *, do=None, B=None):
    B = c["B"] if B is None else B
    N, H = c["N"], c["H"]
    qkv = Buf(dev, c["B"] * N, 3 * H * HD, torch.bfloat16, qkv_rows(inp))
    o = Buf(dev, c["B"] * N, H * HD, torch.bfloat16, _pack(fwd["out_given"]))
    d = Buf(dev, c["B"] * N, H * HD, torch.bfloat16, _pack(inp["do"] if do is None else do))
    lse = Buf(dev, c["B"] * H, N, torch.float32, fwd["lse_given"].reshape(c["B"] * H, N))
    dqkv = Buf(dev, B * N, 3 * H * HD, torch.bfloat16)
    delta = Buf(dev, B * H, N, torch.float32)
    if c["var"]:
        kl = torch.from_numpy(inp["klen"][:B].astype(np.int32)).to(dev) if c["key_len"] is not None else None
        ops.attn_masked_bwd(qkv.block, o.block, d.block, lse.block, dqkv.block, delta.block, kl, B, N, H, SCALE, drop)
    else:
        ops.attn_bwd(qkv.block, o.block, d.block, lse.block, dqkv.block, delta.block, B, N, H, SCALE)
    torch.cuda.synchronize()
    return dqkv, delta


def split_dqkv(x, B, N, H):
    D = H * HD
    return {n: _unpack(x[:, i * D:(i + 1) * D], B, N, H) for i, n in enumerate(("dq", "dk", "dv"))}


# ---- the fused block ---------------------------------------------------------------------------------------------------------------------
BLOCK_D, BLOCK_H, BLOCK_CHUNK, BLOCK_READ_HEAD = 384, 6, 64, 2
BLOCK_CASES = tuple(dict(id="block-N%dB%d" % (N, B), N=N, B=B, seed=9000 + 10 * N + B) for N in (257, 197) for B in (1, 3, 9))
BLOCK_BY_ID = {c["id"]: c for c in BLOCK_CASES}


def make_block_inputs(c, readout_window_j=None):
    """xn [B * N, 384] and W [1152, 384] as float64 arrays of bf16 values, bias float64 [1152] of float32 values."""
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    D, N = BLOCK_D, c["N"]
    xn, W = bf16(rng.standard_normal((c["B"] * N, D))), bf16(0.08 * rng.standard_normal((3 * D, D)))
    b = (0.3 * rng.standard_normal(3 * D)).astype(np.float32).astype(np.float64)
    if readout_window_j is not None:
        j, r0 = readout_window_j, 2 * D + BLOCK_READ_HEAD * HD
        xn[:, 320:], W[:, 320:], W[r0:r0 + HD], b[r0:r0 + HD] = 0.0, 0.0, 0.0, 0.0
        W[r0 + np.arange(HD), 320 + np.arange(HD)] = 1.0
        for img in range(c["B"]):
            for kk in range(64 * j, min(64 * j + 64, N)):
                xn[img * N + kk, 320 + kk - 64 * j] = 1.0
    return dict(xn=xn, W=W, b=b)


def block_reference(c, inp, out_scale=None):
    """out [B * N, 384] in float64 from the unrounded projections, with the bound of the fused kernel (tol) and of the unfused pair (tol_pair);
    P [B, N, N] of BLOCK_READ_HEAD."""
    from _gemm_cases import C_ACC
    B, N, D, H = c["B"], c["N"], BLOCK_D, BLOCK_H
    qkv = inp["xn"] @ inp["W"].T + inp["b"]
    eacc = C_ACC * 2.0 ** -24 * (np.abs(inp["xn"]) @ np.abs(inp["W"]).T + np.abs(inp["b"]))
    dqkv = half_ulp_bf16(np.abs(qkv) + eacc) + eacc                   # what the kernel's bf16 q | k | v may differ from the float64 ones by
    r = {n: np.zeros((B * N, D)) for n in ("out", "tol", "tol_pair")}
    r["P"] = np.zeros((B, N, N))
    for img in range(B):
        rows, osc = slice(img * N, (img + 1) * N), 1.0 if out_scale is None else float(out_scale[img])
        for h in range(H):
            q, k, v = (qkv[rows, i * D + h * HD:i * D + (h + 1) * HD] for i in range(3))
            eq, ek, ev = (dqkv[rows, i * D + h * HD:i * D + (h + 1) * HD] for i in range(3))
            ds = SCALE * (eq @ np.abs(k).T + np.abs(q) @ ek.T)
            for name, block in (("tol", BLOCK_CHUNK), ("tol_pair", None)):
                f = head_probs(q, k, N, None, 0.0, block)
                P, A = f["P"], f["P"] @ np.abs(v)
                rel = ds + (P * ds).sum(1, keepdims=True)
                tol = (P * rel) @ np.abs(v) + P @ ev + f["hu"] @ np.abs(v) + F32(C_F32 * (f["aS"].max(1) + 1.0))[:, None] * A + TINY * (A > 0)
                r[name][rows, h * HD:(h + 1) * HD] = abs(osc) * tol
            r["out"][rows, h * HD:(h + 1) * HD] = osc * (P @ v)
            if h == BLOCK_READ_HEAD:
                r["P"][img] = P
    return r


def restate_block(c, inp, out_scale=None):
    """The fused kernel's rounding points in float32 on the CPU: fp32 projections rounded to bf16, the chunked softmax of restate_fwd,
    out_scale [B] applied before the one rounding of the output."""
    B, N, D, H = c["B"], c["N"], BLOCK_D, BLOCK_H
    qkv = bf16((inp["xn"].astype(_f) @ inp["W"].astype(_f).T + inp["b"].astype(_f)).astype(_f))
    out = np.zeros((B * N, D))
    for img in range(B):
        rows = slice(img * N, (img + 1) * N)
        for h in range(H):
            q, k, v = (qkv[rows, i * D + h * HD:i * D + (h + 1) * HD] for i in range(3))
            out[rows, h * HD:(h + 1) * HD] = restate_fwd(q, k, v, N, None, 0.0, block=BLOCK_CHUNK, osc=1.0 if out_scale is None else out_scale[img])[0]
    return out


def where_is_block(c, idx):
    row, col = idx
    tok = row % c["N"]
    return "image %d token %d (tile %d lane l15 %d%s) head %d d %d = d-tile %d lane group g %d" % (
        row // c["N"], tok, tok // 16, tok % 16, ", the extra query" if tok == 256 else "", col // HD, col % HD, (col % HD) // 16, (col % 16) // 4)


def verify_block(kernel, c, got, want, tol):
    return verify(kernel, "out", got, want, tol, where=lambda idx: where_is_block(c, idx))


# out_scale.  The kernel stores bf16(o * (osc / sum)) where the unscaled launch stores bf16(o * (1 / sum)): with x the unrounded fp32 value and
# out = bf16(x) what the unscaled launch returned, |x - out| <= half_ulp_bf16(out), so the scaled launch is held against s * out, the UNSCALED
# LAUNCH of the same operands -- not against float64, whose bound carries the q / k / v rounding and is ten times wider:
#   |outs - s out| <= s half_ulp_bf16(out) + OSC_F32 2^-24 |s out| + half_ulp_bf16(|s out| + the two terms before)
# OSC_F32 = 8: the scaled launch makes two fp32 roundings (osc / sum, the product) where the unscaled one makes two of its own.  A scale off
# by 1 % is outside everywhere (the bound is at most 2 * 2^-8 = 0.8 % of the value).  A scale applied AFTER the rounding, bf16(s * out), is the
# centre of that bound and cannot be told apart element by element; it shows in how many elements differ from bf16(s * out): x - out is
# spread over +- half_ulp(out), the result's half ulp hu' is that or twice that, so a once-rounded result differs from bf16(s * out) with
# probability s E|x - out| / (2 hu') >= s / 8 = 0.147 at s = 1 / 0.85, and a twice-rounded one never.  ONCE_ROUNDED_MIN = 0.05, a third of that.
OSC_F32, ONCE_ROUNDED_MIN = 8.0, 0.05


def verify_out_scale(kernel, c, outs, out, s):
    """One image's rows: outs (launch with out_scale = s) against out (launch without), both float64 arrays of the bf16 results, s != 0, 1.
    Returns (headroom, fraction of the non-zero elements that differ from bf16(s * out))."""
    want = s * out
    tol = abs(s) * half_ulp_bf16(out) + OSC_F32 * 2.0 ** -24 * np.abs(want)
    r = verify(kernel, "out", outs, want, tol, where=lambda idx: where_is_block(c, idx))
    nz = out != 0
    frac = float((outs[nz] != bf16(want)[nz]).mean())
    assert frac >= ONCE_ROUNDED_MIN, "%s: only %.3f of the scaled elements differ from bf16(s * out): out_scale is applied after the bf16 rounding" % (
        kernel, frac)
    return r, frac


# ---- what the norm tests let through ----------------------------------------------------------------------------------------------------
# Planted faults whose whole-tensor rel-L2 stays under the thresholds of the norm tests (6e-3 output, 1.5e-2 gradients) at those tests' shapes
# and Gaussian inputs -- tests/test_cpu_attn_cases.py::test_what_the_norm_thresholds_let_pass computes every figure and asserts this list.
NORM_BLIND = ("row sum taken after the bf16 rounding", "dV of padded keys left unwritten")
