"""Per-kernel parity of libsrhip (through the C ABI) against fp32 references / the CPU oracle.  Needs a MI355X."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import hooks_ref as H          # noqa: E402
from oracle import optim_ref as O          # noqa: E402
from oracle import semireward_ref as S     # noqa: E402
from oracle import vit_ref as V            # noqa: E402
from semireward_amd import ops             # noqa: E402
from semireward_amd.utils import synth     # noqa: E402
import _gemm_cases as GC                   # noqa: E402

DEV = "cuda:0"


def rnd(*shape, seed=0, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((scale * g.standard_normal(shape)).astype(np.float32)).to(DEV)


def bf(x):
    return x.to(torch.bfloat16).contiguous()


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(16, 128, 64), (300, 256, 128), (24 * 257, 1152, 384), (4112, 384, 1536), (384, 1536, 4160), (130, 4, 64),
                                   (70001, 1152, 384),         # persistent 256x256 kernel, ragged last column tile and row
                                   (2061, 768, 3072), (2300, 3072, 768),    # D = 768 legs (BERT / Wav2Vec2 MLP products)
                                   (13952, 768, 768), (9001, 2304, 1536)])  # two-wave-group 256 x 256 x 64 kernel, ragged last row tile
def test_gemm_epilogues(M, N, K):
    # the 64 x 64 kernel's threshold is a process-wide run-time setting that a training step flips: pinned here, so that the kernels this test runs
    # do not depend on what ran before it (tests/test_gpu_gemm_cases.py holds every kernel to a per-element bound)
    prev = ops._small_max_grid
    ops.gemm_small_max_grid(ops.GEMM_SMALL_ALONE)
    try:
        _gemm_epilogues(M, N, K)
    finally:
        ops.gemm_small_max_grid(prev if prev is not None else ops.GEMM_SMALL_ALONE)


def _gemm_epilogues(M, N, K):
    A, B = bf(rnd(M, K, seed=1)), bf(rnd(N, K, seed=2, scale=0.1))
    bias = rnd(N, seed=3)
    ref = A.double().cpu() @ B.double().cpu().t()          # transposition-detecting: A, B are asymmetric random
    refb = ref + bias.double().cpu()
    # bf16 + bias
    C = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    ops.gemm_nt(ops.EPI_BF16, A, B, C, M, N, K, bias=bias)
    assert relerr(C, refb) < 4e-3
    # GELU (+ pre-activation save)
    pre = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    ops.gemm_nt(ops.EPI_GELU_BF16, A, B, C, M, N, K, bias=bias, aux_out=pre, ldaux=N)
    assert relerr(C, gelu(refb)) < 5e-3 and relerr(pre, refb) < 4e-3
    # residual + per-sample scale
    rps = 4 if M % 4 == 0 else 1
    sc = (torch.arange(M // rps, device=DEV) % 3).float() * 0.625
    X0 = rnd(M, N, seed=4)
    X = X0.clone()
    ops.gemm_nt(ops.EPI_RESID_F32, A, B, X, M, N, K, bias=bias, row_scale=sc, rows_per_sample=rps)
    want = X0.double().cpu() + sc.double().cpu().repeat_interleave(rps)[:, None] * refb
    assert relerr(X, want) < 1e-5 + 2e-3 * float(refb.norm() / want.norm())
    # residual, out-of-place source
    X2 = torch.empty_like(X0)
    ops.gemm_nt(ops.EPI_RESID_F32, A, B, X2, M, N, K, bias=bias, aux_in=X0, ldaux=N)
    assert relerr(X2, X0.double().cpu() + refb) < 1e-5 + 2e-3 * float(refb.norm() / (X0.double().cpu() + refb).norm())
    # dGELU
    pin = bf(rnd(M, N, seed=5))
    ops.gemm_nt(ops.EPI_DGELU_BF16, A, B, C, M, N, K, aux_in=pin, ldaux=N)
    p = pin.double().cpu().requires_grad_(True)
    gelu(p).sum().backward()
    assert relerr(C, ref * p.grad) < 5e-3
    # fp32 accumulate
    G0 = rnd(M, N, seed=6)
    G = G0.clone()
    ops.gemm_nt(ops.EPI_F32, A, B, G, M, N, K, alpha=0.5, beta=1.0)
    assert relerr(G, G0.double().cpu() + 0.5 * ref) < 1e-5
    ops.gemm_nt(ops.EPI_F32, A, B, G, M, N, K, alpha=1.0, beta=0.0)
    assert relerr(G, ref) < 1e-5


@pytest.mark.parametrize("M,rows_per_sample", [(128, 0), (257 * 3, 257), (1000, 0), (257 * 40 + 5, 257)])
def test_mlp_fused(M, rows_per_sample):
    """Fused LN2 + fc1 + GELU + fc2 + residual (srhip_mlp_fused) against (a) the fp32 torch formula of vit.py:165 / 69-75 on
    the bf16-rounded weights and (b) the three unfused libsrhip launches it replaces (same rounding points).
    (tests/test_gpu_mlp_fused_cases.py holds every output of the kernel to a per-element bound.)"""
    D, Hd = 384, 1536
    x0 = rnd(M, D, seed=1)
    x0[:, 7] += 3.0                                            # non-zero mean / uneven columns: transposed fragments would show
    g, b = rnd(D, seed=2, scale=0.2) + 1.0, rnd(D, seed=3, scale=0.1)
    W1, W2 = bf(rnd(Hd, D, seed=4, scale=0.05)), bf(rnd(D, Hd, seed=5, scale=0.03))
    b1, b2 = rnd(Hd, seed=6, scale=0.1), rnd(D, seed=7, scale=0.1)
    rs = None
    if rows_per_sample:
        ns = (M + rows_per_sample - 1) // rows_per_sample
        rs = torch.from_numpy(np.random.Generator(np.random.PCG64(8)).choice([0.0, 1.0 / 0.9], size=ns).astype(np.float32)).to(DEV)
    # (a) fp32 reference
    xn = torch.nn.functional.layer_norm(x0, (D,), g, b, 1e-6)
    y = gelu(xn @ W1.float().T + b1) @ W2.float().T + b2
    scale = rs.repeat_interleave(rows_per_sample)[:M, None] if rs is not None else 1.0
    want = x0 + scale * y
    # (b) unfused HIP path
    xu = x0.clone()
    ln = torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
    h = torch.empty(M, Hd, dtype=torch.bfloat16, device=DEV)
    ops.layernorm_fwd(xu, g, b, 1e-6, ln, None, None, M, D)
    ops.gemm_nt(ops.EPI_GELU_BF16, ln, W1, h, M, Hd, D, bias=b1)
    ops.gemm_nt(ops.EPI_RESID_F32, h, W2, xu, M, D, Hd, bias=b2, row_scale=rs, rows_per_sample=rows_per_sample)
    xf = x0.clone()
    ops.mlp_fused(xf, g, b, 1e-6, W1, b1, W2, b2, rs, rows_per_sample, M, D, Hd)
    torch.cuda.synchronize()
    assert relerr(xf - x0, want - x0) < 6e-3                   # bf16 activations (2^-9) through two products
    assert relerr(xf - x0, xu - x0) < 1.5e-3                   # same rounding points; LN mean/var summation order differs
    if rs is not None:                                         # dropped samples are untouched, bit for bit
        dropped = (rs.repeat_interleave(rows_per_sample)[:M] == 0)
        assert torch.equal(xf[dropped], x0[dropped])
    # out-of-place call with the backward operands of the leading rows (mixed batch: gradient rows first)
    R = min(M, 200) if rows_per_sample == 0 else min(M, 2 * rows_per_sample)
    xo = torch.zeros_like(x0)
    s_ln2 = torch.zeros(R, D, dtype=torch.bfloat16, device=DEV)
    s_pre, s_h = torch.zeros(R, Hd, dtype=torch.bfloat16, device=DEV), torch.zeros(R, Hd, dtype=torch.bfloat16, device=DEV)
    s_mu, s_rs = torch.zeros(R, device=DEV), torch.zeros(R, device=DEV)
    ops.mlp_fused(x0, g, b, 1e-6, W1, b1, W2, b2, rs, rows_per_sample, M, D, Hd, x_out=xo, save=(R, s_ln2, s_pre, s_h, s_mu, s_rs))
    pre_u = torch.empty(M, Hd, dtype=torch.bfloat16, device=DEV)
    mu_u, rs_u = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    ops.layernorm_fwd(x0, g, b, 1e-6, ln, mu_u, rs_u, M, D)
    ops.gemm_nt(ops.EPI_GELU_BF16, ln, W1, h, M, Hd, D, bias=b1, aux_out=pre_u, ldaux=Hd)
    torch.cuda.synchronize()
    assert torch.equal(xo, xf)                                 # same arithmetic, other destination
    assert relerr(s_ln2.float(), ln[:R].float()) < 1e-3 and relerr(s_pre.float(), pre_u[:R].float()) < 2e-3
    assert relerr(s_h.float(), h[:R].float()) < 2e-3
    np.testing.assert_allclose(s_mu.cpu().numpy(), mu_u[:R].cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(s_rs.cpu().numpy(), rs_u[:R].cpu().numpy(), rtol=1e-5)


def test_gemm_tn_grouped():
    """dW = dY^T X (+ db = colsum dY) from row-major operands (srhip_gemm_tn_grouped_f32, LDS transpose reads) against fp32
    torch on the same bf16 operands; ragged K (not a multiple of 32), partial tiles, accumulate into C, several problems."""
    shapes = [(300, 384, 1536), (64, 128, 128), (1028, 1152, 384), (33, 136, 72), (4112, 384, 384)]     # (K, M, N)
    problems, refs = [], []
    for i, (K, M, N) in enumerate(shapes):
        A, Bm = bf(rnd(K, M, seed=10 + i)), bf(rnd(K, N, seed=20 + i))
        A[:, 3] += 1.0                                             # asymmetric: a transposed / permuted fragment would show
        C0, db0 = rnd(M, N, seed=30 + i), rnd(M, seed=40 + i)
        C, db = C0.clone(), (db0.clone() if i != 1 else None)
        problems.append((A, Bm, C, db, M, N, K))
        refs.append((C0 + 0.5 * (A.float().T @ Bm.float()), None if db is None else db0 + A.float().sum(0)))
    desc, npb, ntiles, _, _ = ops.make_group_tn_desc(problems, DEV)
    ops.gemm_tn_grouped_f32(desc, npb, ntiles, alpha=0.5, beta=1.0)
    torch.cuda.synchronize()
    for (A, Bm, C, db, M, N, K), (Cr, dbr) in zip(problems, refs):
        assert relerr(C, Cr) < 2e-6, (K, M, N, relerr(C, Cr))
        if db is not None:
            assert relerr(db, dbr) < 2e-6, (K, M, N)


def _tn_problems(shapes, with_bias=True, seed0=0):
    problems, refs = [], []
    for i, (K, M, N) in enumerate(shapes):
        A, Bm = bf(rnd(K, M, seed=seed0 + 10 + i)), bf(rnd(K, N, seed=seed0 + 20 + i))
        A[:, 3] += 1.0                                             # asymmetric: a transposed / permuted fragment would show
        Bm[:, 5] -= 0.5
        C0, db0 = rnd(M, N, seed=seed0 + 30 + i), rnd(M, seed=seed0 + 40 + i)
        C, db = C0.clone(), (db0.clone() if (with_bias and i != 1) else None)
        problems.append((A, Bm, C, db, M, N, K))
        refs.append((C0, A.float().T @ Bm.float(), None if db is None else db0 + A.float().sum(0)))
    return problems, refs


def test_residual_gemm_applies_the_layernorm_it_is_owed():
    """srhip_gemm_nt_resid_ln_dropout (C = LayerNorm(C) + dropout(A B^T + bias) in place, C = pre-LayerNorm sums) + srhip_postln_fwd(x = NULL)
    against the two launches with the materialised LayerNorm output, on every tile kernel the plan picks for these shapes (64 x 64, 128 x 128,
    256 x 256 persistent), with and without dropout; ragged M."""
    D = 768
    for M, K in ((300, 768), (4100, 3072), (34816, 768)):
        for drop in (None, ops.Drop(77, 3, 0.1)):
            y = rnd(M, D, seed=M) * 1.5 + 0.2
            g, b = 1.0 + 0.1 * rnd(D, seed=1), 0.1 * rnd(D, seed=2)
            A, W, bias = bf(rnd(M, K, seed=3)), bf(rnd(D, K, seed=4) * 0.03), 0.1 * rnd(D, seed=5)
            # reference: materialise x = LN(y), then x += dropout(A W^T + bias)
            x_ref = torch.empty_like(y)
            xb_ref = torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
            mu_r, rs_r = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
            ops.postln_fwd(y, g, b, 1e-12, x_ref, xb_ref, mu_r, rs_r, M, D)
            ops.gemm_nt_resid_dropout(A, W, x_ref, M, D, K, bias, None, drop)
            # lazy: statistics + bf16 operand only, the residual GEMM normalises what it reads
            y2 = y.clone()
            xb = torch.empty_like(xb_ref)
            mu, rs = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
            ops.postln_fwd(y2, g, b, 1e-12, None, xb, mu, rs, M, D)
            assert torch.equal(y2, y) and torch.equal(xb, xb_ref) and torch.equal(mu, mu_r) and torch.equal(rs, rs_r)
            ops.gemm_nt_resid_ln_dropout(A, W, y2, M, D, K, bias, mu, rs, g, b, drop)
            torch.cuda.synchronize()
            assert relerr(y2, x_ref) < 1e-6, (M, K, drop is not None, relerr(y2, x_ref))
    with pytest.raises(RuntimeError):
        ops.postln_fwd(y, g, b, 1e-12, None, xb, None, None, M, D)          # no fp32 output AND no statistics: nothing could apply the LayerNorm later
    # where the plan says a lockstep 256-row kernel (pinned here with the test hook; in production: operands past 2 GiB) the product takes the
    # 128 x 128 tiles instead of refusing
    import subprocess
    import sys
    code = ("import sys, torch; sys.path.insert(0, %r); from semireward_amd import ops; torch.manual_seed(0); dev = 'cuda:0'; M, D, K = 4100, 768, 768;"
            "y = torch.randn(M, D, device=dev); g = torch.rand(D, device=dev) + 0.5; b = torch.randn(D, device=dev) * 0.1;"
            "A = torch.randn(M, K, device=dev).to(torch.bfloat16); W = (torch.randn(D, K, device=dev) * 0.03).to(torch.bfloat16); bias = torch.randn(D, device=dev) * 0.1;"
            "x = torch.empty_like(y); xb = torch.empty(M, D, dtype=torch.bfloat16, device=dev); mu = torch.empty(M, device=dev); rs = torch.empty(M, device=dev);"
            "ops.postln_fwd(y, g, b, 1e-12, x, xb, mu, rs, M, D); ops.gemm_nt_resid_dropout(A, W, x, M, D, K, bias, None, None);"
            "y2 = y.clone(); ops.gemm_nt_resid_ln_dropout(A, W, y2, M, D, K, bias, mu, rs, g, b, None); torch.cuda.synchronize();"
            "e = float((y2 - x).norm() / x.norm()); assert e < 1e-6, e; print('ok', e)") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SRHIP_GEMM="bigoldf"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])


def test_gemm_nt_grouped_narrow_columns():
    """srhip_gemm_nt_grouped_n64_f32 (128 x 64 tiles: the grouped positional convolution, 48 output channels per group) against fp32 torch and against
    the 128 x 128 grouped kernel on the same table: overlapping-row A operands (lda < K: a sliding window over a staging copy, as the convolution
    reads it), N = 48 / 64 / 40 / 72 (two column tiles), ragged M, overwrite and accumulate."""
    rng = np.random.Generator(np.random.PCG64(7))
    for alpha, beta in ((1.0, 0.0), (0.5, 1.0)):
        probs, probs128, refs, outs, outs128, pads, bounds = [], [], [], [], [], [], []
        for (M, N, K, lda) in ((300, 48, 6144, 48), (129, 64, 256, 256), (1000, 40, 384, 16), (64, 72, 128, 128), (5, 48, 96, 96)):
            rows = (M - 1) * lda + K
            Abuf = bf(torch.from_numpy(rng.standard_normal(rows).astype(np.float32)).to(DEV))
            Bm = bf(torch.from_numpy((rng.standard_normal((N, K)) * 0.1).astype(np.float32)).to(DEV))
            Bm[3] += 0.25
            C0 = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32)).to(DEV)
            A = torch.as_strided(Abuf, (M, K), (lda, 1))
            refs.append(beta * C0 + alpha * (A.float() @ Bm.float().t()))
            # the 128 x 128 kernel's output with a pitch (ldc = N + 4) between padding that must come back bit for bit
            C, (C2buf, C2) = C0.clone(), GC.arena2(M, N, N + 4, torch.float32, DEV, False, C0)
            outs.append(C); outs128.append(C2); pads.append((C2buf, C2buf.clone(), M, N))
            probs.append((Abuf.data_ptr(), lda, Bm.data_ptr(), K, C.data_ptr(), N, M, N, K))
            probs128.append((Abuf.data_ptr(), lda, Bm.data_ptr(), K, C2.data_ptr(), N + 4, M, N, K))
            probs[-1] = probs[-1] + (Abuf, Bm)            # keep the operands alive
            # float64 expectation and the per-element fp32 bound of tests/_gemm_cases.py
            A64, B64 = A.double(), Bm.double()
            want = beta * C0.double() + alpha * (A64 @ B64.t())
            bounds.append((want, GC.C_ACC * 2.0 ** -24 * (abs(alpha) * (A64.abs() @ B64.abs().t()) + abs(beta) * C0.double().abs()) + 2.0 ** -23 * want.abs()))
        d64 = ops.make_group_desc_ld([pr[:9] for pr in probs], DEV, bn=64)
        d128 = ops.make_group_desc_ld(probs128, DEV)
        assert d64[2] == 3 + 2 + 8 + 2 + 1 and d128[2] == 3 + 2 + 8 + 1 + 1
        ops.gemm_nt_grouped_f32(d64[0], d64[1], d64[2], alpha=alpha, beta=beta, n64=True)
        ops.gemm_nt_grouped_f32(d128[0], d128[1], d128[2], alpha=alpha, beta=beta)
        torch.cuda.synchronize()
        for C, C2, R, (want, tol), (buf, was, M, N) in zip(outs, outs128, refs, bounds, pads):
            assert relerr(C, R) < 2e-6, relerr(C, R)
            assert torch.equal(C, C2)                        # same k order, same fp32 accumulation: the two tilings agree bit for bit
            print("headroom grouped_n64-%dx%d-a%g_b%g %.4f" % (M, N, alpha, beta, GC.assert_within("grouped %d x %d" % (M, N), C, want, tol)))
            now = buf.clone()
            torch.as_strided(now, (M, N), (N + 4, 1), GC.FRONT).copy_(torch.as_strided(was, (M, N), (N + 4, 1), GC.FRONT))
            assert torch.equal(now.view(torch.int32), was.view(torch.int32))


def test_table_stager_uploads_survive_ring_reuse():
    """ops.TableStager (descriptor tables built inside a step: pinned staging ring + stream-ordered asynchronous copies).  With the stream kept busy
    the copies lag behind the host by milliseconds; a staging slot must not be rewritten before its copy has run: 40 tables through a ring of 4,
    each checked after the fact; a table larger than the ring's slots takes the blocking path."""
    st = ops.TableStager(4096, depth=4)
    big = torch.randn(2048, 2048, device=DEV)
    outs = []
    for i in range(40):
        for _ in range(3):
            big = (big @ big) * 1e-2                       # ~100 us of queued work per product: the uploads queue up behind it
        outs.append((st.upload(np.full(1000 + i, i % 251, dtype=np.uint8), DEV), i))
    outs.append((st.upload(np.full(5000, 77, dtype=np.uint8), DEV), 77))
    torch.cuda.synchronize()
    for t, i in outs[:-1]:
        assert t.numel() == 1000 + i and bool((t == i % 251).all()), i
    assert outs[-1][0].numel() == 5000 and bool((outs[-1][0] == 77).all())


def test_gemm_tn_token_slices_through_slabs():
    """Token slices that write scratch slabs of their own (SRHIP_TN_OVERWRITE) + srhip_slab_reduce_f32, on both weight-gradient kernels: C +=
    product and dbias += column sums as with the atomic slices, unsliced problems of the same table untouched by the second phase, ragged
    last slice, a bias vector whose length is not a multiple of 1024."""
    shapes = [(1100, 32, 288), (64, 128, 128), (4112, 384, 384), (700, 136, 72), (2100, 1160, 384)]     # (K, M, N)
    for tile in (128, 256):
        problems, refs = _tn_problems(shapes, seed0=400 + tile)
        desc, npb, ntiles, _, _ = ops.make_group_tn_desc(problems, DEV, split_k=256, tile=tile, slabs=True)
        assert npb == 5 + 1 + 17 + 3 + 9 and desc.reduce[1] == 4 + 4 and desc.slab.numel() >= 5 * 32 * 288
        ops.gemm_tn_grouped_f32(desc, npb, ntiles, alpha=1.0, beta=1.0, pp=tile == 256)
        torch.cuda.synchronize()
        for (A, Bm, C, db, M, N, K), (C0, P, dbr) in zip(problems, refs):
            assert relerr(C, C0 + P) < 2e-6, (tile, K, M, N, relerr(C, C0 + P))
            if db is not None:
                assert relerr(db, dbr) < 2e-6, (tile, K, M, N)


def test_gemm_tn_grouped_pp():
    """The 256 x 256 persistent weight-gradient kernel (srhip_gemm_tn_grouped_pp_f32) against fp32 torch on the same bf16 operands: ragged K
    (not a multiple of the 64-token K-tile, shorter than one), partial tiles in both directions (384 = 256 + 128, 136, 72), bias sums, accumulate
    and overwrite, token slices through atomics, and a table of more tiles than workgroups (the cursor crosses tiles and entries)."""
    shapes = [(1100, 768, 512), (64, 256, 256), (4112, 384, 384), (300, 384, 1536), (33, 136, 72), (640, 1152, 384), (200, 256, 768)]     # (K, M, N)
    for alpha, beta in ((0.5, 1.0), (1.0, 0.0)):
        problems, refs = _tn_problems(shapes)
        desc, npb, ntiles, _, _ = ops.make_group_tn_desc(problems, DEV, tile=256)
        assert ntiles == sum(((M + 255) // 256) * ((N + 255) // 256) for K, M, N in shapes)
        ops.gemm_tn_grouped_f32(desc, npb, ntiles, alpha=alpha, beta=beta, pp=True)
        torch.cuda.synchronize()
        for (A, Bm, C, db, M, N, K), (C0, P, dbr) in zip(problems, refs):
            Cr = beta * C0 + alpha * P
            assert relerr(C, Cr) < 2e-6, (K, M, N, alpha, beta, relerr(C, Cr))
            if db is not None:
                assert relerr(db, dbr) < 2e-6, (K, M, N)
    # token slices (SRHIP_TN_ATOMIC entries): the order of the fp32 atomic adds is free, the sum is not
    problems, refs = _tn_problems([(1100, 768, 512), (640, 384, 640)], seed0=100)
    desc, npb, ntiles, _, _ = ops.make_group_tn_desc(problems, DEV, split_k=256, tile=256)
    assert npb == 5 + 3
    ops.gemm_tn_grouped_f32(desc, npb, ntiles, alpha=1.0, beta=1.0, pp=True)
    torch.cuda.synchronize()
    for (A, Bm, C, db, M, N, K), (C0, P, dbr) in zip(problems, refs):
        assert relerr(C, C0 + P) < 2e-6, (K, M, N, relerr(C, C0 + P))
        if db is not None:
            assert relerr(db, dbr) < 2e-6
    # more tiles than workgroups + the planner's sliced tail: 7 x (9 + 9 + 9 + 12) = 273 tiles -> 17 past the first round
    shapes = [(1088, 768, 768), (1088, 768, 768), (1088, 768, 768), (1088, 768, 1024)] * 7
    problems, refs = _tn_problems(shapes, seed0=200)
    plan = ops.tn_pp_plan(problems)
    assert any(sl > 0 for _, sl in plan) and all(sl % 64 == 0 for _, sl in plan)
    for slabs in (False, True):                        # the planner's slices through atomics, and through slabs + the reduce launch (the encoders' form)
        problems, refs = _tn_problems(shapes, seed0=200)
        desc, npb, ntiles, _, _ = ops.make_group_tn_desc(problems, DEV, tile=256, slabs=slabs)
        assert ntiles > 273 and npb > len(shapes) and hasattr(desc, "reduce") == slabs
        ops.gemm_tn_grouped_f32(desc, npb, ntiles, alpha=1.0, beta=1.0, pp=True)
        torch.cuda.synchronize()
        for (A, Bm, C, db, M, N, K), (C0, P, dbr) in zip(problems, refs):
            assert relerr(C, C0 + P) < 2e-6, (K, M, N, relerr(C, C0 + P))
            if db is not None:
                assert relerr(db, dbr) < 2e-6


def test_gemm_identity_asymmetric():
    """A = I against an asymmetric B: catches a swapped row/col C write that random-norm checks could hide."""
    K = 128
    A = torch.zeros(K, K, device=DEV)
    A[torch.arange(K), torch.arange(K)] = 1
    Bm = (torch.arange(256 * K, device=DEV).reshape(256, K) % 251).float() / 8
    C = torch.empty(K, 256, dtype=torch.float32, device=DEV)
    ops.gemm_nt(ops.EPI_F32, bf(A), bf(Bm), C, K, 256, K)
    assert torch.equal(C.cpu(), bf(Bm).float().cpu().t())
    with pytest.raises(RuntimeError):
        ops.gemm_nt(ops.EPI_F32, bf(A), bf(Bm), C, K, 256, 100)      # K % 64 != 0 -> error code, not a crash


# ------------------------------------------------------------------------------------------------
def attn_ref(qkv, B, N, H, scale):
    q, k, v = qkv.reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    a = torch.softmax((q @ k.transpose(-2, -1)) * scale, dim=-1)
    return (a @ v).transpose(1, 2).reshape(B * N, H * 64), torch.logsumexp((q @ k.transpose(-2, -1)) * scale, dim=-1)


@pytest.mark.parametrize("M,rows_per_sample", [(128, 0), (257 * 3, 257), (1000, 0), (257 * 40 + 5, 257), (257 * 127, 257), (257 * 300, 257)])
def test_mlp_fused_proj(M, rows_per_sample):
    """Attention projection + first residual + LN2 + fc1 + GELU + fc2 + second residual in ONE launch (srhip_mlp_fused_proj, vit.py:105-106,
    :163-165) against (a) the fp32 torch formula on the
    bf16-rounded operands and (b) the two launches it replaces (srhip_gemm_nt with the residual epilogue + srhip_mlp_fused), incl. per-sample
    DropPath scales on both branches and in-place operation.  (257 * 300 rows = 603 tiles: workgroups that loop over several tiles.)
    (tests/test_gpu_mlp_fused_cases.py holds every output of the kernel, its strided and its planned form to a per-element bound.)"""
    D, Hd = 384, 1536
    x0 = rnd(M, D, seed=1)
    x0[:, 7] += 3.0
    ao32 = rnd(M, D, seed=11, scale=0.7)
    ao32[:, 300] += 2.0                                        # uneven columns: a wrong fragment transpose would show
    ao = bf(ao32)
    Wp, bp = bf(rnd(D, D, seed=12, scale=0.06)), rnd(D, seed=13, scale=0.2)
    g, b = rnd(D, seed=2, scale=0.2) + 1.0, rnd(D, seed=3, scale=0.1)
    W1, W2 = bf(rnd(Hd, D, seed=4, scale=0.05)), bf(rnd(D, Hd, seed=5, scale=0.03))
    b1, b2 = rnd(Hd, seed=6, scale=0.1), rnd(D, seed=7, scale=0.1)
    rs1 = rs2 = None
    if rows_per_sample:
        ns = (M + rows_per_sample - 1) // rows_per_sample
        rng = np.random.Generator(np.random.PCG64(8))
        rs1 = torch.from_numpy(rng.choice([0.0, 1.0 / 0.95], size=ns, p=[0.3, 0.7]).astype(np.float32)).to(DEV)
        rs2 = torch.from_numpy(rng.choice([0.0, 1.0 / 0.9], size=ns).astype(np.float32)).to(DEV)
    sc = lambda r: r.repeat_interleave(rows_per_sample)[:M, None] if r is not None else 1.0   # noqa: E731
    # (a) fp32 reference
    x1 = x0 + sc(rs1) * (ao.float() @ Wp.float().T + bp)
    xn = torch.nn.functional.layer_norm(x1, (D,), g, b, 1e-6)
    want = x1 + sc(rs2) * (gelu(xn @ W1.float().T + b1) @ W2.float().T + b2)
    # (b) the two launches it replaces
    xu = x0.clone()
    ops.gemm_nt(ops.EPI_RESID_F32, ao, Wp, xu, M, D, D, bias=bp, row_scale=rs1, rows_per_sample=rows_per_sample)
    x1u = xu.clone()
    ops.mlp_fused(xu, g, b, 1e-6, W1, b1, W2, b2, rs2, rows_per_sample, M, D, Hd)
    # fused, in place
    xf = x0.clone()
    ops.mlp_fused_proj(xf, ao, Wp, bp, rs1, g, b, 1e-6, W1, b1, W2, b2, rs2, rows_per_sample, M, D, Hd)
    # fused, out of place
    xo = torch.zeros_like(x0)
    ops.mlp_fused_proj(x0, ao, Wp, bp, rs1, g, b, 1e-6, W1, b1, W2, b2, rs2, rows_per_sample, M, D, Hd, x_out=xo)
    # ... and with the next block's norm1 output written by the same launch
    gn, bn = rnd(D, seed=21, scale=0.3) + 1.0, rnd(D, seed=22, scale=0.2)
    xo2 = torch.zeros_like(x0)
    lnn = torch.full((M, D), 9.0, dtype=torch.bfloat16, device=DEV)
    ops.mlp_fused_proj(x0, ao, Wp, bp, rs1, g, b, 1e-6, W1, b1, W2, b2, rs2, rows_per_sample, M, D, Hd, x_out=xo2, ln_next=lnn, next_gamma=gn,
                       next_beta=bn)
    lnu = torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
    ops.layernorm_fwd(xf, gn, bn, 1e-6, lnu, None, None, M, D)
    torch.cuda.synchronize()
    assert torch.equal(xo2, xf)
    # LayerNorm of identical fp32 rows by two kernels with different summation orders: bf16 outputs agree except where a value sits on a
    # rounding boundary (one bf16 ulp = 2^-8 relative)
    dl = (lnn.float() - lnu.float()).abs()
    assert float(dl.max()) <= 2.0 ** -7 * float(lnu.float().abs().max()) and float((dl > 0).float().mean()) < 0.02
    assert relerr(lnn.float(), torch.nn.functional.layer_norm(xf, (D,), gn, bn, 1e-6)) < 3e-3
    assert torch.equal(xo, xf)
    assert relerr(xf - x0, want - x0) < 6e-3
    # same rounding points (accumulation / LN summation order differs) unless a DropPath factor is in play: the fused launch applies it to
    # the bf16 B operand of the product (one rounding of rs * value instead of value), the unfused pair to the fp32 result
    assert relerr(xf - x0, xu - x0) < (1.5e-3 if rs1 is None else 4e-3)
    assert relerr(xf, xu) < (2e-4 if rs1 is None else 3e-3), relerr(xf, xu)
    if rs1 is not None:
        # the form the backbone uses: the attention launch applied rs1 BEFORE rounding its output (srhip_attn_block_fused out_scale) -> one
        # rounding per operand as in the unfused pair, and no further from the fp32 formula than that pair
        xs = x0.clone()
        ops.mlp_fused_proj(xs, bf(sc(rs1) * ao32), Wp, bp, rs1, g, b, 1e-6, W1, b1, W2, b2, rs2, rows_per_sample, M, D, Hd, ao_scaled=True)
        torch.cuda.synchronize()
        want32 = x0 + sc(rs1) * (ao32 @ Wp.float().T + bp)
        want32 = want32 + sc(rs2) * (gelu(torch.nn.functional.layer_norm(want32, (D,), g, b, 1e-6) @ W1.float().T + b1) @ W2.float().T + b2)
        e_f, e_u = relerr(xs - x0, want32 - x0), relerr(xu - x0, want32 - x0)
        assert e_f < 1.1 * e_u + 1e-4, (e_f, e_u)
    if rs1 is not None:                                        # rows whose both branches are dropped are untouched, bit for bit
        dead = (rs1.repeat_interleave(rows_per_sample)[:M] == 0) & (rs2.repeat_interleave(rows_per_sample)[:M] == 0)
        assert (M < 257 * 20 or bool(dead.any())) and torch.equal(xf[dead], x0[dead])
        only2 = (rs1.repeat_interleave(rows_per_sample)[:M] != 0) & (rs2.repeat_interleave(rows_per_sample)[:M] == 0)
        if bool(only2.any()):                                  # MLP branch dropped: the projection residual alone (rs1 on the bf16 operand)
            assert relerr(xf[only2] - x0[only2], x1u[only2] - x0[only2]) < 4e-3
        only1 = (rs1.repeat_interleave(rows_per_sample)[:M] == 0) & (rs2.repeat_interleave(rows_per_sample)[:M] != 0)
        if bool(only1.any()):                                  # projection dropped: LN + MLP of the untouched rows
            assert relerr(xf[only1] - x0[only1], xu[only1] - x0[only1]) < 4e-3


def test_gelu_forms_against_exact_erf():
    """The library's two GELU evaluations against nn.GELU() (exact erf, vit.py:63) in float64: gelu_erf (every path with a backward, every
    unfused epilogue) to 1e-6; gelu_poly2 (inside srhip_mlp_fused_proj, no transcendentals) to max(7e-5, 5e-6 |x|) over |x| <= 30 and below
    half a bf16 quantum of the result wherever |GELU| >= 0.03 -- its result is rounded to bf16 right away."""
    x = torch.cat([torch.linspace(-30, 30, 600001), torch.linspace(-4.3, -4.2, 20001), torch.tensor([0.0, -0.0, 1e-30, -1e-30, 4.252893, -4.252893])]).to(DEV)
    ye, yp = torch.empty_like(x), torch.empty_like(x)
    ops.gelu_eval(x, ye, yp)
    xd = x.double().cpu()
    want = 0.5 * xd * (1 + torch.erf(xd / 2 ** 0.5))
    assert float((ye.double().cpu() - want).abs().max()) < 1e-6
    ep = (yp.double().cpu() - want).abs()
    assert (GC.GELU_POLY2_ABS, GC.GELU_POLY2_REL) == (7e-5, 5e-6)                # (tests/_mlp_fused_cases.py builds its bound on this figure)
    assert bool((ep <= torch.maximum(torch.full_like(ep, GC.GELU_POLY2_ABS), GC.GELU_POLY2_REL * xd.abs())).all()), float(ep.max())
    big = want.abs() >= 0.03
    assert bool((ep[big] <= 0.5 * 2.0 ** -8 * want.abs()[big]).all())          # < half a bf16 quantum (2^-8 relative at worst)
    assert bool(torch.isfinite(yp).all()) and float(yp[x == 0].abs().max()) == 0.0


@pytest.mark.parametrize("B,N,H", [(3, 17, 2), (2, 197, 6), (4, 257, 6), (1, 64, 1), (2, 33, 3), (2, 320, 2), (1, 512, 3), (2, 401, 1)])
def test_attention_fwd_bwd(B, N, H):
    D = H * 64
    qkv = bf(rnd(B * N, 3 * D, seed=7, scale=1.5))
    out = torch.empty(B * N, D, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B, H, N, device=DEV)
    ops.attn_fwd(qkv, out, lse, B, N, H, 0.125)
    x = qkv.double().cpu().requires_grad_(True)
    ro, rl = attn_ref(x, B, N, H, 0.125)
    assert relerr(out, ro) < 6e-3
    assert float((lse.double().cpu() - rl).abs().max()) < 2e-3
    d_out = bf(rnd(B * N, D, seed=8))
    ro.backward(d_out.double().cpu())
    dqkv = torch.zeros(B * N, 3 * D, dtype=torch.bfloat16, device=DEV)
    delta = torch.empty(B, H, N, device=DEV)
    ops.attn_bwd(qkv, out, d_out, lse, dqkv, delta, B, N, H, 0.125)
    g = x.grad
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        assert relerr(dqkv[:, sl], g[:, sl]) < 1.5e-2, name


def test_attention_forced_large_scores():
    """Spiked key: exercises the max-subtraction path with raw scores >> the rest (guide rule 26)."""
    B, N, H = 1, 257, 1
    qkv = bf(rnd(N, 192, seed=9))
    qkv[5, :64] = 6.0
    qkv[200, 64:128] = 6.0
    out = torch.empty(N, 64, dtype=torch.bfloat16, device=DEV)
    ops.attn_fwd(qkv, out, None, B, N, H, 0.125)
    ro, _ = attn_ref(qkv.double().cpu(), B, N, H, 0.125)
    assert torch.isfinite(out.float()).all() and relerr(out, ro) < 6e-3


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D", [(7, 128), (4112, 384), (1000, 768)])
def test_layernorm_fwd_bwd(M, D):
    x, g, b = rnd(M, D, seed=10, scale=2.0) + 0.5, 1 + 0.1 * rnd(D, seed=11), 0.1 * rnd(D, seed=12)
    out = torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    ops.layernorm_fwd(x, g, b, 1e-6, out, mean, rstd, M, D)
    xc = x.double().cpu().requires_grad_(True)
    gc, bc = g.double().cpu().requires_grad_(True), b.double().cpu().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xc, (D,), gc, bc, 1e-6)
    assert relerr(out, ref) < 3e-3
    assert float((mean.double().cpu() - xc.detach().mean(-1)).abs().max()) < 1e-5
    dy = bf(rnd(M, D, seed=13))
    ref.backward(dy.double().cpu())
    dx0 = rnd(M, D, seed=14)
    dx, dg, db = dx0.clone(), torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    ops.layernorm_bwd(dy, x, mean, rstd, g, dx, dg, db, M, D)
    assert relerr(dx - dx0, xc.grad) < 2e-5
    assert relerr(dg, gc.grad) < 2e-5 and relerr(db, bc.grad) < 2e-5


@pytest.mark.parametrize("cfgd", [V.VIT_TINY_TEST, V.VIT_SMALL_P2_32])
def test_patch_embed_and_head(cfgd):
    cfg = V.VitCfg(num_classes=10, **cfgd)
    D, N, ps, HW = cfg.embed_dim, cfg.num_tokens, cfg.patch_size, cfg.img_size
    P = {k: torch.from_numpy(v).to(DEV) for k, v in synth.synth_params(V.param_shapes(cfg), 21).items()}
    nimg, B = 5, 7
    img = rnd(nimg, 3, HW, HW, seed=15)
    idx = torch.tensor([0, 3, 1, 4, 4, 2, 0], dtype=torch.int32, device=DEV)
    x = torch.empty(B, N, D, device=DEV)
    ops.patch_embed_fwd(img, idx, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], P["cls_token"], P["pos_embed"], x,
                        B, 3, HW, ps, D)
    Pc = {k: v.double().cpu().requires_grad_(True) for k, v in P.items()}
    sel = img.double().cpu()[idx.cpu().long()]
    t = V.patchify(sel, ps) @ Pc["patch_embed.proj.weight"].reshape(D, -1).t() + Pc["patch_embed.proj.bias"]
    t = torch.cat((Pc["cls_token"].expand(B, -1, -1), t), dim=1) + Pc["pos_embed"]
    assert relerr(x, t) < 1e-6
    dx = rnd(B, N, D, seed=16)
    t.backward(dx.double().cpu())
    dW, dbp = torch.zeros_like(P["patch_embed.proj.weight"]), torch.zeros(D, device=DEV)
    dcls, dpos = torch.zeros(D, device=DEV), torch.zeros(N, D, device=DEV)
    ops.patch_embed_bwd(dx, img, idx, dW, dbp, dcls, dpos, B, 3, HW, ps, D)
    assert relerr(dW, Pc["patch_embed.proj.weight"].grad) < 1e-5 and relerr(dbp, Pc["patch_embed.proj.bias"].grad) < 1e-5
    assert relerr(dcls, Pc["cls_token"].grad.reshape(-1)) < 1e-5 and relerr(dpos, Pc["pos_embed"].grad[0]) < 1e-5
    # cls head
    C = cfg.num_classes
    feat, logits = torch.empty(B, D, device=DEV), torch.empty(B, C, device=DEV)
    xhat, rstd = torch.empty(B, D, device=DEV), torch.empty(B, device=DEV)
    ops.cls_head_fwd(x, P["norm.weight"], P["norm.bias"], 1e-6, P["head.weight"], P["head.bias"], feat, logits, xhat, rstd, B, N, D, C)
    xc = x.double().cpu().requires_grad_(True)
    f = torch.nn.functional.layer_norm(xc[:, 0], (D,), Pc["norm.weight"], Pc["norm.bias"], 1e-6)
    lg = f @ Pc["head.weight"].t() + Pc["head.bias"]
    assert relerr(feat, f) < 1e-6 and relerr(logits, lg) < 1e-6
    # the scattering form: image b's outputs at row rows[b] of larger tables, with and without the dense copies
    rows = torch.tensor([(7 * b + 3) % (2 * B + 5) for b in range(B)], dtype=torch.int64, device=DEV)
    assert len(set(rows.tolist())) == B
    fa, la = torch.full((2 * B + 5, D), 5.0, device=DEV), torch.full((2 * B + 5, C), 5.0, device=DEV)
    f2, l2 = torch.empty_like(feat), torch.empty_like(logits)
    ops.cls_head_fwd_scatter(x, P["norm.weight"], P["norm.bias"], 1e-6, P["head.weight"], P["head.bias"], f2, l2, None, None, fa, la, rows,
                             B, N, D, C)
    assert torch.equal(f2, feat) and torch.equal(l2, logits) and torch.equal(fa[rows], feat) and torch.equal(la[rows], logits)
    untouched = torch.ones(2 * B + 5, dtype=torch.bool, device=DEV)
    untouched[rows] = False
    assert bool((fa[untouched] == 5.0).all()) and bool((la[untouched] == 5.0).all())
    fb_, lb_ = torch.zeros_like(fa), torch.zeros_like(la)
    ops.cls_head_fwd_scatter(x, P["norm.weight"], P["norm.bias"], 1e-6, P["head.weight"], P["head.bias"], None, None, None, None, fb_, lb_,
                             rows, B, N, D, C)
    assert torch.equal(fb_[rows], feat) and torch.equal(lb_[rows], logits)
    dl = rnd(B, C, seed=17)
    lg.backward(dl.double().cpu())
    dxh = torch.zeros(B, N, D, device=DEV)
    dWh, dbh = torch.zeros(C, D, device=DEV), torch.zeros(C, device=DEV)
    dgn, dbn = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    ops.cls_head_bwd(dl, P["head.weight"], P["norm.weight"], feat, xhat, rstd, dxh, dWh, dbh, dgn, dbn, B, N, D, C)
    assert relerr(dxh, xc.grad) < 2e-5 and relerr(dWh, Pc["head.weight"].grad) < 1e-5 and relerr(dbh, Pc["head.bias"].grad) < 1e-5
    assert relerr(dgn, Pc["norm.weight"].grad) < 1e-5 and relerr(dbn, Pc["norm.bias"].grad) < 1e-5


def test_glue_kernels():
    M, D, rps = 4112, 384, 257
    x = rnd(M, D, seed=18)
    sc = rnd(M // rps, seed=19)
    out = torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
    ops.cast_scale_rows(x, sc, rps, out, M, D)
    assert torch.equal(out, (x * sc.repeat_interleave(rps)[:, None]).to(torch.bfloat16))
    Mp = 4160
    t = torch.full((D, Mp), 7.0, dtype=torch.bfloat16, device=DEV)
    cs = torch.zeros(D, device=DEV)
    ops.transpose_to_bf16(out, False, D, t, Mp, M, Mp, D, colsum=cs)
    assert torch.equal(t[:, :M], out.t()) and float(t[:, M:].float().abs().max()) == 0.0
    assert relerr(cs, out.float().sum(0)) < 1e-5
    ops.transpose_to_bf16(out, False, D, t, Mp, M, Mp, D, apply_gelu=True)
    assert relerr(t[:, :M], gelu(out.float().double()).t()) < 3e-3
    w = rnd(384, 1536, seed=20)
    wt = torch.empty(1536, 384, dtype=torch.bfloat16, device=DEV)
    ops.transpose_to_bf16(w, True, 1536, wt, 384, 384, 384, 1536)
    assert torch.equal(wt, w.t().to(torch.bfloat16))
    flat = rnd(100003, seed=22)
    fb = torch.empty(100003, dtype=torch.bfloat16, device=DEV)
    ops.cast_f32_bf16(flat, fb, flat.numel())
    assert torch.equal(fb, flat.to(torch.bfloat16))
    probs = torch.tensor(V.drop_path_probs(V.VitCfg(**V.VIT_SMALL_P2_32)), device=DEV)
    dp = torch.empty(12, 2, 4096, device=DEV)
    ops.droppath_fill(dp, probs, 12, 4096, 1234)
    # any selection / order of the columns of the same draw in one launch (the step's launch trains take slices of it)
    cols = torch.tensor([4095, 0, 17, 17, 2048, 1], dtype=torch.int64, device=DEV)
    dpc = torch.empty(12, 2, cols.numel(), device=DEV)
    ops.droppath_fill(dpc, probs, 12, 4096, 1234, cols=cols)
    assert torch.equal(dpc, dp.index_select(2, cols))
    keep = 1 - probs.cpu().numpy()
    vals = dp.cpu().numpy()
    assert np.all(vals[0] == 1.0)
    for l in range(1, 12):
        nz = vals[l] != 0
        assert np.allclose(vals[l][nz], 1 / keep[l]) and abs(nz.mean() - keep[l]) < 0.03


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["c10_w", "c100_w", "c10_nw", "c100_b256", "c100_rej", "c100_rej_nw"])
def test_flexmatch_score_filter_bit_exact(golden, tag):
    """Golden probabilities from the reference -> masks / classwise_acc / selected_label must be bit-identical."""
    g = golden("hooks")
    C, U, Bu, steps, warm, seed = [int(v) for v in g[f"{tag}/meta"]]
    sel = torch.full((U,), -1, dtype=torch.int64, device=DEV)
    hist = torch.zeros(C + 1, dtype=torch.int32, device=DEV)
    acc = torch.zeros(C, device=DEV)
    ops.flexmatch_rebuild_hist(sel, hist, U, C)
    mp, mi, mask, fm = torch.empty(Bu, device=DEV), torch.empty(Bu, dtype=torch.int64, device=DEV), torch.empty(Bu, device=DEV), torch.empty(Bu, device=DEV)
    for t in range(steps):
        probs = torch.from_numpy(g[f"{tag}/probs"][t]).to(DEV)
        idx = torch.from_numpy(g[f"{tag}/idx"][t]).to(DEV)
        ops.row_max(probs, True, None, mp, mi, Bu, C)
        assert np.array_equal(mi.cpu().numpy(), g[f"{tag}/pseudo_label"][t])
        ops.fixed_mask(mp, 0.95, fm, Bu)
        assert np.array_equal(fm.cpu().numpy(), g[f"{tag}/fixed_mask"][t])
        ops.flexmatch_mask(mp, mi, idx, 0.95, sel, hist, acc, mask, Bu, C, U, bool(warm))
        assert np.array_equal(mask.cpu().numpy(), g[f"{tag}/mask"][t]), (tag, t)
        assert np.array_equal(acc.cpu().numpy().view(np.uint32), g[f"{tag}/classwise_acc"][t].view(np.uint32)), (tag, t)
    s = sel.cpu().numpy()
    nz = np.nonzero(s != -1)[0]
    assert np.array_equal(nz, g[f"{tag}/sel_idx"]) and np.array_equal(s[nz], g[f"{tag}/sel_val"])
    h2 = torch.zeros_like(hist)
    ops.flexmatch_rebuild_hist(sel, h2, U, C)
    assert torch.equal(hist, h2)                      # incremental histogram == recount
    # fused-softmax mode on logits: same argmax, max-prob within 2 ulp of the reference softmax
    lg = torch.from_numpy(g[f"{tag}/logits"][0]).to(DEV)
    po = torch.empty(Bu, C, device=DEV)
    ops.row_max(lg, False, po, mp, mi, Bu, C)
    # rows read in place from a [groups, rows, C] table (the weak rows of every pass inside the step's logits): same bits, no gathered copy
    if Bu % 4 == 0:
        rpg, grows, first = Bu // 4, Bu // 4 + 3, 2
        table = torch.full((4 * grows + first, C), -7.0, device=DEV)
        for gi in range(4):
            table[first + gi * grows:first + gi * grows + rpg] = lg[gi * rpg:(gi + 1) * rpg]
        mp2, mi2 = torch.empty_like(mp), torch.empty_like(mi)
        ops.row_max_strided(table, first, False, None, mp2, mi2, Bu, C, rpg, grows)
        assert torch.equal(mp2, mp) and torch.equal(mi2, mi)
    ref = g[f"{tag}/probs"][0]
    assert np.array_equal(mi.cpu().numpy(), ref.argmax(-1))
    np.testing.assert_allclose(mp.cpu().numpy(), ref.max(-1), rtol=3e-7)
    np.testing.assert_allclose(po.cpu().numpy(), ref, rtol=2e-6, atol=1e-12)


@pytest.mark.parametrize("tag", ["b8_c100", "b64_c10", "b256_c100"])
def test_masked_ce(golden, tag):
    g = golden("losses")
    lg = torch.from_numpy(g[f"{tag}/logits"]).to(DEV)
    y = torch.from_numpy(g[f"{tag}/y"]).to(DEV)
    m, m2 = torch.from_numpy(g[f"{tag}/mask"]).to(DEV), torch.from_numpy(g[f"{tag}/mask2"]).to(DEV)
    B, C = lg.shape
    loss, dl = torch.empty(1, device=DEV), torch.empty(B, C, device=DEV)
    ops.masked_ce(lg, y, None, None, 1.0, loss, dl, B, C)
    assert abs(float(loss) - float(g[f"{tag}/sup"])) < 2e-6
    np.testing.assert_allclose(dl.cpu().numpy(), g[f"{tag}/sup_grad"], rtol=2e-5, atol=1e-8)
    ops.masked_ce(lg, y, m, m2, 1.0, loss, dl, B, C)
    assert abs(float(loss) - float(g[f"{tag}/unsup"])) < 2e-6
    np.testing.assert_allclose(dl.cpu().numpy(), g[f"{tag}/unsup_grad"], rtol=2e-5, atol=1e-8)
    ops.masked_ce(lg, y, m, None, 1.0, loss, None, B, C)
    assert abs(float(loss) - float(g[f"{tag}/unsup_mask1"])) < 2e-6


# ------------------------------------------------------------------------------------------------
def flat_params(d, keys):
    return torch.cat([torch.from_numpy(np.ascontiguousarray(d[k])).reshape(-1) for k in keys]).to(DEV)


def unflat(flat, shapes):
    out, o = {}, 0
    for k, s in shapes.items():
        n = int(np.prod(s))
        out[k] = flat[o:o + n].reshape(s).cpu()
        o += n
    return out


@pytest.mark.parametrize("tag", ["f384_b8", "f128_b64", "f768_b16_c200"])
def test_rewarder_generator(golden, tag):
    g = golden("rewarder")
    Fd, C, B, seed = [int(v) for v in g[f"{tag}/meta"]]
    L = S.label_dim(C)
    shapes = S.rewarder_shapes(Fd, C)
    rp_np = synth.synth_params(shapes, seed)
    gp_np = synth.synth_params(S.generator_shapes(Fd), seed + 100)
    gp_np["fc_layers.6.bias"] = gp_np["fc_layers.6.bias"] + np.float32(2.6)
    rp, gp = flat_params(rp_np, S.REWARDER_KEYS), flat_params(gp_np, S.GENERATOR_KEYS)
    assert rp.numel() == ops.rewarder_param_count(Fd, L) and gp.numel() == ops.generator_param_count(Fd)
    rng = np.random.Generator(np.random.PCG64(seed + 200))
    feats = torch.from_numpy(rng.standard_normal((B, Fd)).astype(np.float32)).to(DEV)
    labels = torch.from_numpy(rng.integers(0, C, size=(B,), dtype=np.int64)).to(DEV)
    ws = torch.empty(ops.rewarder_ws_floats(1, B), device=DEV)
    r = torch.empty(B, device=DEV)
    rpt, gpt = torch.empty(ops.rewarder_t_floats(Fd), device=DEV), torch.empty(ops.generator_t_floats(Fd), device=DEV)
    ops.rewarder_prepare(rp, rpt, Fd, L)
    ops.generator_prepare(gp, gpt, Fd)
    ops.rewarder_fwd(rp, rpt, feats, labels, r, ws, 1, B, Fd, L)
    np.testing.assert_allclose(r.cpu().numpy(), g[f"{tag}/reward"][:, 0], rtol=1e-5, atol=1e-6)   # stated fp tolerance for rewards
    # mask2: bit-exact on the REFERENCE's rewards (integer thresholding parity)
    m2, mean = torch.empty(B, device=DEV), torch.empty(1, device=DEV)
    ops.reward_mask2(torch.from_numpy(g[f"{tag}/reward"][:, 0]).to(DEV), m2, mean, 1, B)
    assert np.array_equal(m2.cpu().numpy(), g[f"{tag}/mask2"])
    # grouped launch == per-group launches
    G = 3
    fe3 = torch.cat([feats, feats.flip(0), feats * 0.5])
    lb3 = torch.cat([labels, labels.flip(0), labels])
    ws3 = torch.empty(ops.rewarder_ws_floats(G, B), device=DEV)
    r3 = torch.empty(G * B, device=DEV)
    ops.rewarder_fwd(rp, rpt, fe3, lb3, r3, ws3, G, B, Fd, L)
    for gi in range(G):
        ops.rewarder_fwd(rp, rpt, fe3[gi * B:(gi + 1) * B].contiguous(), lb3[gi * B:(gi + 1) * B].contiguous(), r, ws, 1, B, Fd, L)
        assert torch.equal(r, r3[gi * B:(gi + 1) * B])
    # ... == the groups read in place from a [passes, batch, F] table (group g = rows first + g * group_rows .. + B), as the step does
    Bt, first = B + 5, 3
    table = torch.full((G + 1, Bt, Fd), 99.0, device=DEV)
    for gi in range(G):
        table[gi + 1, first:first + B] = fe3[gi * B:(gi + 1) * B]
    r3s = torch.empty(G * B, device=DEV)
    ops.rewarder_fwd(rp, rpt, table, lb3, r3s, ws3, G, B, Fd, L, feats_first_row=Bt + first, group_rows=Bt)
    assert torch.equal(r3s, r3)
    # a group of one row tile (B <= 8) runs as ONE launch, larger groups as two: same arithmetic, same bits
    for Bs in (8, 5):
        rs_, ws_ = torch.empty(Bs, device=DEV), torch.empty(ops.rewarder_ws_floats(1, Bs), device=DEV)
        ops.rewarder_fwd(rp, rpt, feats[:Bs].contiguous(), labels[:Bs].contiguous(), rs_, ws_, 1, Bs, Fd, L)
        assert bool(torch.isfinite(rs_).all()) and float(rs_.min()) > 0.0 and float(rs_.max()) < 1.0
    # generator
    go, gl = torch.empty(B, device=DEV), torch.empty(B, dtype=torch.int64, device=DEV)
    ops.generator_fwd(gp, gpt, feats, go, gl, B, Fd)
    np.testing.assert_allclose(go.cpu().numpy(), g[f"{tag}/gen_out"][:, 0], rtol=1e-5, atol=2e-6)
    assert np.array_equal(gl.cpu().numpy(), g[f"{tag}/gen_label"][:, 0])
    # SR update: target, losses, grads, two Adam steps
    tgt = torch.empty(B, device=DEV)
    ops.sr_target(gl, labels, tgt, B)
    assert np.array_equal(tgt.cpu().numpy(), g[f"{tag}/upd_target"][:, 0])
    grads, m, v = torch.empty_like(rp), torch.zeros_like(rp), torch.zeros_like(rp)
    losses = torch.empty(2, device=DEV)
    for step in (1, 2):
        ops.rewarder_prepare(rp, rpt, Fd, L)
        ops.rewarder_fwd(rp, rpt, feats, gl, r, ws, 1, B, Fd, L, save_for_bwd=True)
        ops.rewarder_bwd(rp, feats, gl, tgt, ws, grads, losses, B, Fd, L)
        if step == 1:
            np.testing.assert_allclose(r.cpu().numpy(), g[f"{tag}/upd_reward"][:, 0], rtol=1e-5, atol=1e-6)
            assert abs(float(losses[0]) - float(g[f"{tag}/generator_loss"])) < 2e-6
            assert abs(float(losses[1]) - float(g[f"{tag}/rewarder_loss"])) < 2e-6
            gd = unflat(grads, shapes)
            for k in S.REWARDER_KEYS:
                if k == "cross_attention_fc.bias":
                    assert float(gd[k].abs().max()) == 0.0           # analytically zero; see test_oracle_golden
                    continue
                gs = g.samp(f"{tag}/grad/{k}")
                a = gd[k].numpy().ravel()[::gs["stride"]]
                np.testing.assert_allclose(a, gs["sample"], rtol=5e-4, atol=1e-7 + 1e-4 * float(np.abs(gs["sample"]).max()), err_msg=k)
        ops.adam_flat(rp, grads, m, v, rp.numel(), 5e-4, step)
        pd = unflat(rp, shapes)
        for k in S.REWARDER_KEYS:
            if k == "cross_attention_fc.bias":
                continue
            gs = g.samp(f"{tag}/after{step}/{k}")
            np.testing.assert_allclose(pd[k].numpy().ravel()[::gs["stride"]], gs["sample"], rtol=1e-5, atol=3e-5, err_msg=k)


def test_adamw_flat_matches_oracle():
    cfg = V.VitCfg(num_classes=10, **V.VIT_TINY_TEST)
    from semireward_amd.optim import build_chunk_table
    shapes = V.param_shapes(cfg)
    P = synth.synth_params(shapes, 61)
    hp = O.vit_param_hparams(shapes, cfg.depth, 5e-4, 5e-4, 0.5)
    names = [n for n, _ in shapes]
    flat = torch.cat([torch.from_numpy(P[n]).reshape(-1) for n in names]).to(DEV)
    sizes = [int(np.prod(s)) for _, s in shapes]
    table = build_chunk_table(sizes).to(DEV)
    lr_t = torch.tensor([hp[n][0] for n in names], dtype=torch.float32, device=DEV)
    wd_t = torch.tensor([hp[n][1] for n in names], dtype=torch.float32, device=DEV)
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    pb, ema = torch.empty(flat.numel(), dtype=torch.bfloat16, device=DEV), flat.clone()
    Pt = {k: torch.from_numpy(v_.copy()) for k, v_ in P.items()}
    mo = {k: torch.zeros_like(v_) for k, v_ in Pt.items()}
    vo = {k: torch.zeros_like(v_) for k, v_ in Pt.items()}
    for step in range(4):
        gr = synth.synth_params(shapes, 70 + step)
        gflat = torch.cat([torch.from_numpy(gr[n]).reshape(-1) * 0.1 for n in names]).to(DEV)
        fac = O.cosine_warmup_factor(step, 10, 2)
        ops.adamw_flat(flat, gflat, m, v, pb, ema, table, table.shape[0], lr_t, wd_t, fac, step + 1, ema_m=0.9, zero_grad=True)
        assert float(gflat.abs().max()) == 0.0
        for k in names:
            O.adamw_step(Pt[k], torch.from_numpy(gr[k]) * 0.1, mo[k], vo[k], step + 1, hp[k][0] * fac, hp[k][1])
    want = torch.cat([Pt[n].reshape(-1) for n in names])
    np.testing.assert_allclose(flat.cpu().numpy(), want.numpy(), rtol=2e-6, atol=1e-8)
    assert torch.equal(pb, flat.to(torch.bfloat16))


@pytest.mark.parametrize("tag", ["c10_q", "c100_mean", "c100_q"])
def test_freematch_hook_and_entropy(golden, tag):
    """FreeMatch thresholds + fairness loss on device against the reference's own sequences (tests/golden/freematch_hook.npz)."""
    g = golden("freematch_hook")
    C, Bu, steps, uq, clip, seed = [int(v) for v in g[f"{tag}/meta"]]
    m = float(g[f"{tag}/momentum"])
    time_p = torch.full((1,), 1.0 / C, device=DEV)
    p_model, label_hist = torch.full((C,), 1.0 / C, device=DEV), torch.full((C,), 1.0 / C, device=DEV)
    colsum, hist = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    mp, mi, mask = torch.empty(Bu, device=DEV), torch.empty(Bu, dtype=torch.int64, device=DEV), torch.empty(Bu, device=DEV)
    loss, ws = torch.empty(1, device=DEV), torch.empty(Bu * C, device=DEV)
    for t in range(steps):
        probs = torch.from_numpy(g[f"{tag}/probs"][t]).to(DEV)
        ops.row_max(probs, True, None, mp, mi, Bu, C)
        ops.freematch_stats(probs, mi, colsum, hist, Bu, C)
        ops.freematch_update(mp, Bu, colsum, hist, mp, mi, time_p, p_model, label_hist, mask, Bu, C, m, bool(uq), bool(clip))
        assert np.array_equal(mask.cpu().numpy(), g[f"{tag}/mask"][t]), (tag, t)          # identical masks on identical probabilities
        assert float(time_p) == pytest.approx(float(g[f"{tag}/time_p"][t]), rel=3e-7)
        np.testing.assert_allclose(p_model.cpu().numpy(), g[f"{tag}/p_model"][t], rtol=1e-6)
        np.testing.assert_allclose(label_hist.cpu().numpy(), g[f"{tag}/label_hist"][t], rtol=1e-6)
        ls = torch.from_numpy(g[f"{tag}/logits_s"][t]).to(DEV)
        dl = torch.full((Bu, C), 7.0, device=DEV)
        ops.freematch_entropy(ls, mask, p_model, label_hist, 1.0, loss, dl, ws, Bu, C)
        assert float(loss) == pytest.approx(float(g[f"{tag}/ent"][t]), rel=2e-5, abs=1e-6)
        np.testing.assert_allclose(dl.cpu().numpy(), g[f"{tag}/ent_grad"][t], rtol=2e-4, atol=1e-8)
        d2 = torch.ones(Bu, C, device=DEV)
        ops.freematch_entropy(ls, mask, p_model, label_hist, 0.5, loss, d2, ws, Bu, C, accumulate=True)
        np.testing.assert_allclose(d2.cpu().numpy(), 1.0 + 0.5 * g[f"{tag}/ent_grad"][t], rtol=2e-4, atol=1e-7)
    # empty mask: zero loss, zero / untouched gradient (srfreematch.py:216-219)
    z = torch.zeros(Bu, device=DEV)
    dl = torch.full((Bu, C), 7.0, device=DEV)
    ops.freematch_entropy(ls, z, p_model, label_hist, 1.0, loss, dl, ws, Bu, C)
    assert float(loss) == 0.0 and float(dl.abs().max()) == 0.0


@pytest.mark.parametrize("tag", ["c10_uniform", "c100_model", "c10_model_s3"])
def test_softmatch_and_distalign(golden, tag):
    """DistAlign EMA + aligned probabilities and the SoftMatch Gaussian weight on device against the reference's own sequences
    (tests/golden/softmatch_hook.npz): EMA state to fp32 round-off (reduction order differs), weights to 2e-6."""
    g = golden("softmatch_hook")
    C, Bu, Bl, steps, ns, model_t, seed = [int(v) for v in g[f"{tag}/meta"]]
    m = float(g[f"{tag}/momentum"])
    p_model, p_target = torch.zeros(C, device=DEV), torch.ones(C, device=DEV) / C
    inited = torch.zeros(1, dtype=torch.int32, device=DEV)
    mu_var = torch.tensor([1.0 / C, 1.0], device=DEV)
    cs_u, cs_l, hist = torch.empty(C, device=DEV), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    zi = torch.zeros(max(Bu, Bl), dtype=torch.int64, device=DEV)
    for t in range(steps):
        lu, ll = torch.from_numpy(g[f"{tag}/logits_ulb"][t]).to(DEV), torch.from_numpy(g[f"{tag}/logits_lb"][t]).to(DEV)
        pu, plb = torch.empty(Bu, C, device=DEV), torch.empty(Bl, C, device=DEV)
        mp, mi = torch.empty(Bu, device=DEV), torch.empty(Bu, dtype=torch.int64, device=DEV)
        mpl, mil = torch.empty(Bl, device=DEV), torch.empty(Bl, dtype=torch.int64, device=DEV)
        ops.row_max(lu, False, pu, mp, mi, Bu, C)
        ops.row_max(ll, False, plb, mpl, mil, Bl, C)
        ops.freematch_stats(pu, zi, cs_u, hist, Bu, C)
        ops.freematch_stats(plb, zi, cs_l, hist, Bl, C)
        al, amp, ami = torch.empty(Bu, C, device=DEV), torch.empty(Bu, device=DEV), torch.empty(Bu, dtype=torch.int64, device=DEV)
        ops.distalign(pu, cs_u, Bu, cs_l if model_t else None, Bl, p_model, p_target, inited, m, al, amp, ami, Bu, C)
        ma, mk = torch.empty(Bu, device=DEV), torch.empty(Bu, device=DEV)
        ops.softmatch_mask(amp, Bu, amp, mu_var, m, ns, ma, Bu)
        mu_a = mu_var.clone()
        ops.softmatch_mask(mp, Bu, mp, mu_var, m, ns, mk, Bu)
        torch.cuda.synchronize()
        np.testing.assert_allclose(p_model.cpu().numpy(), g[f"{tag}/p_model"][t], rtol=2e-6, atol=1e-9)
        np.testing.assert_allclose(p_target.cpu().numpy(), g[f"{tag}/p_target"][t], rtol=2e-6, atol=1e-9)
        np.testing.assert_allclose(al.cpu().numpy(), g[f"{tag}/aligned"][t], rtol=5e-6, atol=1e-9)
        assert torch.equal(amp, al.max(dim=1)[0]) and torch.equal(ami, al.argmax(dim=1))
        np.testing.assert_allclose(mu_var.cpu().numpy(), [g[f"{tag}/mu"][t], g[f"{tag}/var"][t]], rtol=3e-6)
        # the weights are steep functions of (p - mu) / sigma: compare with the formula on the device's own state, and with the
        # reference within the amplification of the 1e-6 state round-off
        np.testing.assert_allclose(ma.cpu().numpy(), g[f"{tag}/mask_a"][t], rtol=2e-4, atol=1e-6)
        np.testing.assert_allclose(mk.cpu().numpy(), g[f"{tag}/mask_p"][t], rtol=2e-4, atol=1e-6)
        d = torch.clamp(amp - mu_a[0], max=0.0)
        np.testing.assert_allclose(ma.cpu().numpy(), torch.exp(-(d * d) / (2 * mu_a[1] / ns ** 2)).cpu().numpy(), rtol=3e-6, atol=1e-7)
    assert int(inited) == 1


def test_concurrent_stream_is_measured_not_assumed():
    """ops.concurrent_stream / streams_overlap: HIP multiplexes streams onto a few hardware queues; a stream handed out by concurrent_stream has
    been seen to execute beside the current stream, and among a few dozen plain streams at least one pair that does NOT overlap exists on a
    default configuration (which is why the check is needed) -- that part is reported, not required (GPU_MAX_HW_QUEUES may be large)."""
    from semireward_amd import ops
    main = torch.cuda.current_stream()
    s = ops.concurrent_stream(torch.device("cuda", 0))
    assert ops.streams_overlap(main, s) and not ops.streams_overlap(s, s)        # (a stream never overlaps with itself: the probe has power)
    plain = [torch.cuda.Stream() for _ in range(12)]
    aliased = [i for i, p in enumerate(plain) if not ops.streams_overlap(main, p)]
    print("plain streams sharing the current stream's hardware queue: %d of %d" % (len(aliased), len(plain)))
