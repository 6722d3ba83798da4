"""Every tile kernel of csrc/gemm.hip, every epilogue form and every edge of tests/_gemm_cases.py on the MI355X, element by element against float64
(the vendor library's float64 matmul on the device for the product, everything after it restated here): GC.verify is the function
tests/test_cpu_gemm_cases.py shows accepting the float32 restatement of every case and rejecting each planted fault.  Every test asserts which
kernel srhip_gemm_nt_plan names before it launches; the run-time threshold of the 64 x 64 kernel is pinned to GEMM_SMALL_ALONE for the file.
Each test prints 'headroom <id> <max |got - want| / tol>' (profiles/gemm_cases_headroom.txt keeps the largest per kernel and form)."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                   # (the hook children run this file as a script)
    sys.path.insert(0, ROOT)

import _gemm_cases as GC                   # noqa: E402
from semireward_amd import ops             # noqa: E402

DEV = "cuda:0"
PAIRS, IDS = GC.params()
HOOK_PLAN = {"bigold": "big256", "big128": "big128", "big2wg": "big2wg", "big256r8": "pp256"}      # SRHIP_GEMM test hook -> what the plan then names


@pytest.fixture(scope="module", autouse=True)
def small_grid_alone():
    prev = ops._small_max_grid
    ops.gemm_small_max_grid(ops.GEMM_SMALL_ALONE)
    yield
    ops.gemm_small_max_grid(prev if prev is not None else ops.GEMM_SMALL_ALONE)


def R(t):
    """the first element of a (pitched) view as a bare pointer argument"""
    return None if t is None else ops.RawRows(t, 0)


def run_hip(L, plan_M=None):
    f, M, N, K = L.f, L.M, L.N, L.K
    A, B, C = R(L.A), R(L.B), R(L.C)
    aux_in = L.preact if f["epi"] == ops.EPI_DGELU_BF16 else (L.resid if f["resid"] == "aux" else None)
    if f["api"] == "nt":
        ops.gemm_nt(f["epi"], A, B, C, M, N, K, lda=L.lda, ldb=L.ldb, ldc=L.ldc, bias=L.bias, row_scale=L.row_scale,
                    rows_per_sample=GC.RPS if L.row_scale is not None else 0, aux_in=R(aux_in), aux_out=R(L.aux_out),
                    ldaux=L.ldaux if (aux_in is not None or L.aux_out is not None) else 0, alpha=f["alpha"], beta=f["beta"], plan_M=plan_M)
    elif f["api"] == "dropout":
        assert L.ldc == N
        ops.gemm_nt_dropout(f["epi"], A, B, C, M, N, K, L.drop(), lda=L.lda, ldb=L.ldb, bias=L.bias, aux_in=R(aux_in), aux_out=R(L.aux_out), ldaux=L.ldaux)
    elif f["api"] == "resid_dropout":
        assert L.ldc == N and L.ldaux == N
        ops.gemm_nt_resid_dropout(A, B, C, M, N, K, L.bias, R(L.resid), L.drop(), lda=L.lda, ldb=L.ldb)
    else:
        assert L.ldc == N
        ops.gemm_nt_resid_ln_dropout(A, B, C, M, N, K, L.bias, *L.ln, L.drop(), lda=L.lda, ldb=L.ldb)


@pytest.mark.parametrize("c,f", PAIRS, ids=IDS)
def test_gemm_case(c, f):
    assert ops.gemm_nt_plan(f["epi"], c["M"], c["N"], c["K"], f["beta"]) == c["plan"]
    L = GC.Launch(c, f, DEV)
    run_hip(L)
    torch.cuda.synchronize()
    ratio = GC.verify(L)
    print("headroom %s-%s %.4f" % (c["id"], f["name"], ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("cid", ["pp256-39173x1152x128", "tile128-11009x384x128"])
def test_rows_split_off_a_larger_launch_keep_its_kernel(cid):
    """srhip_gemm_nt_planned: 300 rows with plan_M = the full launch equal the first 300 rows of that launch bit for bit, within the bound, padding
    untouched; plan_M < M and the accumulating EPI_F32 (split-K: an order no row count pins) are refused."""
    c, m = GC.by_id(cid), 300
    N, K = c["N"], c["K"]
    for name in ("bf16", "resid_aux"):
        f = GC.form(name)
        assert ops.gemm_nt_plan(f["epi"], c["M"], N, K) == c["plan"] and ops.gemm_nt_plan(f["epi"], m, N, K) != c["plan"]
        L = GC.Launch(c, f, DEV)
        run_hip(L)
        ex = GC.expect(L)
        buf, out = GC.arena2(m, N, N, L.C.dtype, DEV, False)
        was = buf.clone()
        ops.gemm_nt(f["epi"], R(L.A), R(L.B), R(out), m, N, K, bias=L.bias, aux_in=R(L.resid) if f["resid"] else None,
                    ldaux=L.ldaux if f["resid"] else 0, plan_M=c["M"])
        torch.cuda.synchronize()
        assert torch.equal(GC._bits(out), GC._bits(L.C[:m]))
        ratio = GC.assert_within("%s-%s planned" % (cid, name), out, ex["want"][:m], ex["tol"][:m], GC.TILE[c["plan"]])
        print("headroom %s-%s-planned %.4f" % (cid, name, ratio))
        now = buf.clone()
        torch.as_strided(now, (m, N), (N, 1), GC.FRONT).copy_(torch.as_strided(was, (m, N), (N, 1), GC.FRONT))
        assert torch.equal(GC._bits(now), GC._bits(was))
        with pytest.raises(RuntimeError):
            ops.gemm_nt(f["epi"], R(L.A), R(L.B), R(out), m, N, K, bias=L.bias, aux_in=R(L.resid) if f["resid"] else None,
                        ldaux=L.ldaux if f["resid"] else 0, plan_M=m - 1)
    G = torch.zeros(m, N, device=DEV)
    with pytest.raises(RuntimeError):
        ops.gemm_nt(ops.EPI_F32, R(L.A), R(L.B), G, m, N, K, alpha=1.0, beta=1.0, plan_M=c["M"])
    torch.cuda.synchronize()
    assert float(G.abs().max()) == 0.0


def test_argument_errors_leave_the_output_alone():
    c = GC.by_id("small64-65x132x192")
    M, N, K = c["M"], c["N"], c["K"]
    Lb, Lr, Ld = (GC.Launch(c, GC.form(n), DEV) for n in ("bf16", "resid_inplace", "dgelu"))
    s = torch.cuda.current_stream().cuda_stream

    def nt(L, epi, **o):
        a = dict(A=L.A.data_ptr(), lda=L.lda, B=L.B.data_ptr(), ldb=L.ldb, C=L.C.data_ptr(), ldc=L.ldc, M=M, N=N, K=K, bias=None, row_scale=None,
                 rps=0, aux_in=None, aux_out=None, ldaux=0)
        a.update(o)
        ops._call("srhip_gemm_nt", epi, a["A"], a["lda"], a["B"], a["ldb"], a["C"], a["ldc"], a["M"], a["N"], a["K"], a["bias"], a["row_scale"],
                  a["rps"], a["aux_in"], a["aux_out"], a["ldaux"], 1.0, 0.0, s)
    nt(Lb, ops.EPI_BF16)                                     # (the arguments as they stand are accepted)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(Lb.C.float()).all())
    Lb = GC.Launch(c, GC.form("bf16"), DEV)
    bad = [
        ("K % 32 != 0", lambda: nt(Lb, ops.EPI_BF16, K=100)),
        ("N % 4 != 0", lambda: nt(Lb, ops.EPI_BF16, N=130)),
        ("lda % 8 != 0", lambda: nt(Lb, ops.EPI_BF16, lda=K + 4)),
        ("ldb % 8 != 0", lambda: nt(Lb, ops.EPI_BF16, ldb=K + 4)),
        ("ldc % 4 != 0", lambda: nt(Lb, ops.EPI_BF16, ldc=N + 2)),
        ("C 4 bytes off a 16-byte boundary", lambda: nt(Lb, ops.EPI_BF16, C=Lb.C.data_ptr() + 4)),
        ("A 4 bytes off a 16-byte boundary", lambda: nt(Lb, ops.EPI_BF16, A=Lb.A.data_ptr() + 4)),
        ("DGELU without aux_in", lambda: nt(Ld, ops.EPI_DGELU_BF16)),
        ("row_scale with rows_per_sample = 0", lambda: nt(Lr, ops.EPI_RESID_F32, row_scale=GC.arena1(GC.row_scale_of(M), DEV)[1].data_ptr(), rps=0)),
        ("dropout with ldc != N (GELU)", lambda: ops._call(
            "srhip_gemm_nt_dropout", ops.EPI_GELU_BF16, Lb.A.data_ptr(), K, Lb.B.data_ptr(), K, Lb.C.data_ptr(), N + 4, M, N, K, None, None, None, 0,
            *ops.Drop(GC.DROP_SEED, GC.DROP_SITE, GC.DROP_P).args(), s)),
        ("dropout with ldc != N (residual)", lambda: ops._call(
            "srhip_gemm_nt_resid_dropout", Lr.A.data_ptr(), K, Lr.B.data_ptr(), K, Lr.C.data_ptr(), N + 4, M, N, K, None, None, N,
            *ops.Drop(GC.DROP_SEED, GC.DROP_SITE, GC.DROP_P).args(), s)),
    ]
    ln = [GC.arena1(t, DEV)[1] for t in GC.ln_of(GC.resid_of(M, N), N)]
    for i in range(4):
        args = list(ln)
        args[i] = None
        bad.append(("LayerNorm form without statistic %d" % i,
                    lambda args=args: ops.gemm_nt_resid_ln_dropout(R(Lr.A), R(Lr.B), R(Lr.C), M, N, K, None, *args, None)))
    for what, call in bad:
        with pytest.raises(RuntimeError):
            call()
        print("refused:", what)
    torch.cuda.synchronize()
    for L in (Lb, Lr, Ld):
        for buf, was in L.before:
            assert torch.equal(GC._bits(buf), GC._bits(was))


# ---- kernels only the SRHIP_GEMM test hook reaches ---------------------------------------------------------------------------------------------
def _child(mode):
    """runs in a fresh process with SRHIP_GEMM=mode (read once per process): the pp256 cases through the same check, one JSON line of results"""
    ops.gemm_small_max_grid(ops.GEMM_SMALL_ALONE)
    ratios, failures = {}, {}
    for (c, f), cid in zip(PAIRS, IDS):
        if c["plan"] != "pp256":
            continue
        if mode != "big256r8" and (f["ln"] or f["overlap"]):       # (the LayerNorm-owing residual and sliding rows exist for the two-wave-group kernel only)
            continue
        plan = ops.gemm_nt_plan(f["epi"], c["M"], c["N"], c["K"], f["beta"])
        if plan != HOOK_PLAN[mode]:
            failures[cid] = "plan %s" % plan
            continue
        L = GC.Launch(c, f, DEV)
        run_hip(L)
        torch.cuda.synchronize()
        try:
            ratios[cid] = GC.verify(L)
        except AssertionError as e:
            failures[cid] = str(e)
    print(json.dumps(dict(mode=mode, ran=len(ratios) + len(failures), worst=max(ratios.values(), default=0.0), failures=failures, ratios=ratios)))


def test_hook_only_kernels():
    """SRHIP_GEMM = bigold (the lockstep kernel on K % 64 == 0), big128, big2wg (the 256 x 128 tiles) and big256r8 (the 8-slot ring of the
    two-wave-group kernel): tools/ decides dispatch rules with them, so they compute what the shipped kernels compute.  One fresh child per
    mode, one at a time; a child that ends on a signal, an error or its time limit ends the loop -- nothing more is started on the GPU."""
    for mode in HOOK_PLAN:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode], env=dict(os.environ, SRHIP_GEMM=mode), cwd=ROOT,
                               capture_output=True, text=True, timeout=600)
        except subprocess.TimeoutExpired as e:
            pytest.fail("SRHIP_GEMM=%s: time limit; no further mode started\n%s\n%s" % (mode, str(e.stdout)[-2000:], str(e.stderr)[-2000:]))
        if r.returncode != 0:
            pytest.fail("SRHIP_GEMM=%s: exit status %d; no further mode started\n%s\n%s" % (mode, r.returncode, r.stdout[-2000:], r.stderr[-3000:]))
        res = json.loads(r.stdout.strip().splitlines()[-1])
        for cid, ratio in sorted(res["ratios"].items()):
            print("headroom %s:%s %.4f" % (mode, cid, ratio))
        assert res["mode"] == mode and res["ran"] >= 20 and not res["failures"], (mode, res["failures"])
        assert res["worst"] <= 1.0


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child(sys.argv[2])
