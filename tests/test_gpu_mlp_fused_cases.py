"""Every shipped instantiation of csrc/mlp_fused.hip against float64, element by element: the cases, references, bounds and verify() are
tests/_mlp_fused_cases.py (tests/test_cpu_mlp_fused_cases.py shows what verify() accepts and rejects without a GPU).  Per case: one ordinary
launch into poisoned arenas, every element of every output checked, then the bit-for-bit conditions -- the in-place launch equals the
out-of-place one, the strided and the planned launch equal srhip_mlp_fused_proj on the same operands.  (A launch that equals a verified one bit
for bit is verified with it: verify() runs once per case.)  Each test prints the worst |got - want| / bound per output."""
import numpy as np
import pytest
import torch

import _mlp_fused_cases as C
from _gemm_cases import GELU_E
from semireward_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ids = lambda c: c["id"]      # noqa: E731


def _check(c, twin=False):
    L = C.run_gpu(C.Launch(c), DEV)
    ratios = C.verify(L)
    print("%s: worst |got - want| / bound: %s" % (c["id"], ", ".join("%s %.3f" % kv for kv in ratios.items())))
    assert max(ratios.values()) <= 1.0
    Li = C.run_gpu(C.Launch(c, inplace=True), DEV)
    touched = Li.pad_touched()
    assert not touched, "%s in place: padding overwritten %s" % (c["id"], touched)
    C.same_bits(L, Li, c["id"] + ": out of place vs in place")
    if twin:
        Ld = C.run_gpu(C.Launch(C.dense_twin(c)), DEV)
        assert not Ld.pad_touched()
        C.same_bits(L, Ld, c["id"] + " vs srhip_mlp_fused_proj")


@pytest.mark.parametrize("c", C.DENSE, ids=ids)
def test_mlp_fused(c):
    _check(c)


@pytest.mark.parametrize("c", C.PROJ, ids=ids)
def test_mlp_fused_proj(c):
    _check(c)


@pytest.mark.parametrize("c", C.STRIDED, ids=ids)
def test_mlp_fused_proj_strided(c):
    _check(c, twin=True)


@pytest.mark.parametrize("c", C.PLANNED, ids=ids)
def test_mlp_fused_proj_planned(c):
    _check(c, twin=True)


@pytest.mark.parametrize("n", [1, 2, 511, 512, 513, 100001])
def test_gelu_eval(n):
    """srhip_gelu_eval per element: gelu_erf to GELU_E, gelu_poly2 to the figure test_gelu_forms_against_exact_erf pins, odd and even counts (the
    kernel takes two values per thread), outputs between untouched padding"""
    x = np.random.Generator(np.random.PCG64([n, 9])).uniform(-8.0, 8.0, n).astype(np.float32)
    x[0] = 4.252893
    bufs = {k: C._arena(1, n, n, np.float32, k == "x", x if k == "x" else None) for k in ("x", "erf", "poly")}
    t = {k: torch.from_numpy(b).to(DEV) for k, (b, _) in bufs.items()}
    assert _lib.lib().srhip_gelu_eval(*(t[k][C.FRONT:].data_ptr() for k in ("x", "erf", "poly")), n, None) == 0
    torch.cuda.synchronize()
    want = C.gelu64(x.astype(np.float64))
    for k, tol in (("erf", np.full(n, GELU_E)), ("poly", C.gelu_poly2_err(x.astype(np.float64)))):
        got = t[k].cpu().numpy()
        blk = got[C.FRONT:C.FRONT + n]
        err = np.abs(blk.astype(np.float64) - want)
        assert (err <= tol).all(), (k, int(np.argmax(err - tol)), float(err.max()))
        got[C.FRONT:C.FRONT + n] = np.nan
        assert np.array_equal(got.view(np.uint32), bufs[k][0].view(np.uint32)), k + ": padding overwritten"
        print("gelu_eval n=%d %s: worst |got - want| / bound %.3f" % (n, k, float((err / tol).max())))


# ---- refused calls ---------------------------------------------------------------------------------------------------------------------------
DENSE_ARGS = ("x", "xo", "gam", "bet", "eps", "W1", "b1", "W2", "b2", "r2", "rps", "save", "s_ln2", "s_pre", "s_h", "s_mean", "s_rstd", "M", "D", "Hd")
PROJ_ARGS = ("x", "xo", "ao", "Wp", "bp", "r1", "ao_scaled", "gam", "bet", "eps", "W1", "b1", "W2", "b2", "r2", "rps", "ln", "gn", "bn", "M", "D", "Hd")


def _args(L, t, names):
    c = L.c
    scal = dict(eps=C.EPS, rps=c["rps"], save=c["save"], M=c["M"], D=C.D, Hd=c["Hd"], ao_scaled=int(c["ao_scaled"]), pitch=c["pitch"], B=c.get("B"))
    return {k: scal[k] if k in scal else (t[k].data_ptr() + C.FRONT * t[k].element_size() if k in t else None) for k in names}


def _refused(fn, args, names, what, **change):
    a = dict(args, **change)
    assert fn(*(a[k] for k in names), None) == -1, "%s: %s was accepted" % (fn.__name__, what)


def _untouched(L, t):
    C.download(L, t)
    for k in L.outputs:
        assert np.array_equal(C._bits(L.buf[k]), C._bits(L.init[k])), "a refused call wrote to " + k


def test_refused_calls_return_the_error_code_and_write_nothing():
    lib = _lib.lib()
    # srhip_mlp_fused
    L = C.Launch(C._dense(17, 128, 5, True, 15))
    t, _ = C.upload(L, DEV)
    a, n, f = _args(L, t, DENSE_ARGS), DENSE_ARGS, lib.srhip_mlp_fused
    _refused(f, a, n, "D = 256", D=256)
    for hd in (64, 192, 4224):
        _refused(f, a, n, "Hd = %d" % hd, Hd=hd)
    for k in ("x", "xo", "W1", "W2", "gam", "bet", "s_ln2", "s_pre", "s_h"):
        _refused(f, a, n, k + " off by 4 bytes", **{k: a[k] + 4})
    _refused(f, a, n, "save_rows > M", save=18)
    _refused(f, a, n, "save_rows < 0", save=-1)
    for k in ("s_ln2", "s_pre", "s_h", "s_mean", "s_rstd"):
        _refused(f, a, n, "save_rows > 0 without " + k, **{k: None})
    _refused(f, a, n, "row_scale without rows_per_sample", rps=0)
    _refused(f, a, n, "M = 0", M=0)
    _untouched(L, t)
    # srhip_mlp_fused_proj and its two forms
    c = C._planned(5, 6, 128, 3, "kernel")
    L = C.Launch(c)
    t, _ = C.upload(L, DEV)
    forms = ((lib.srhip_mlp_fused_proj, PROJ_ARGS), (lib.srhip_mlp_fused_proj_strided, PROJ_ARGS + ("pitch",)),
             (lib.srhip_mlp_fused_proj_planned, PROJ_ARGS + ("plan", "B")))
    for f, n in forms:
        a = _args(L, t, n)
        _refused(f, a, n, "D = 256", D=256)
        for hd in (64, 192, 4224):
            _refused(f, a, n, "Hd = %d" % hd, Hd=hd)
        for k in ("x", "xo", "ao", "Wp", "W1", "W2", "gam", "bet", "ln"):
            _refused(f, a, n, k + " off by 4 bytes", **{k: a[k] + 4})
        _refused(f, a, n, "row_scale2 without rows_per_sample", rps=0)
        _refused(f, a, n, "row_scale1 without rows_per_sample", rps=0, r2=None)
        _refused(f, a, n, "ln_next without its gamma", gn=None)
        _refused(f, a, n, "ln_next without its beta", bn=None)
        _refused(f, a, n, "M = 0", M=0)
    f, n = forms[1]
    a = _args(L, t, n)
    _refused(f, a, n, "pitch < D", pitch=C.D - 8, ln=None)
    _refused(f, a, n, "pitch not a multiple of 8", pitch=C.D + 4, ln=None)
    _refused(f, a, n, "ln_next with pitch != D", pitch=C.D + 8)
    f, n = forms[2]
    a = _args(L, t, n)
    _refused(f, a, n, "B * rows_per_sample != M", B=7)
    _refused(f, a, n, "B * rows_per_sample != M", rps=4)
    _refused(f, a, n, "B = 0", B=0)
    _refused(f, a, n, "no row_scale2", r2=None)
    _refused(f, a, n, "no plan", plan=None)
    _refused(f, a, n, "plan off by 2 bytes", plan=a["plan"] + 2)
    _untouched(L, t)
    # ... and the same arguments unchanged are accepted by all three (the refusals above are not an accident of the argument list)
    for f, n in forms:
        a = _args(L, t, n)
        assert f(*(a[k] for k in n), None) == 0
    torch.cuda.synchronize()
