"""The criterion surface (soft targets, 'mse' / 'l1', per-row losses) without a GPU: the C ABI and its wrappers, argument validation, the
register budget of csrc/criterions.hip, the reference fixture against a float64 restatement, and the unchanged hard-label path."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _criterions_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("srhip_ce_hard", "srhip_ce_soft", "srhip_consistency_mse", "srhip_consistency_l1")

# fp32 reference (the fixture) against the float64 restatement, measured by test_fixture_is_self_consistent over all 578 cases:
# largest loss error 1.75e-7 (mse/B8_C2_g1/mean_prob_mask2), largest gradient error 4.34e-7 (soft/B1_C2_g1/sum_raw_nomask); rel-L2 at
# gain 1, max-abs over the case's largest gradient at gain 24, denominators as floors() explains.  Below 5e-6, so the GPU tests hold the
# kernels to 1e-5 against this fixture.
REF_FP32_ERR = 1e-6


def rel(a, b, floor=0.0):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    d = float(np.linalg.norm(a - b))
    return 0.0 if d == 0.0 else d / (max(float(np.linalg.norm(b)), floor) + 1e-30)


def floors(c):
    """(loss floor, gradient floor) of a case's error denominators.  Only gain 24 against probability targets ('mse', and the gradient
    of soft 'ce' with 'prob' targets) has any: there softmax(z) and the targets are both saturated, p - t is a difference of fp32 numbers
    next to 1 and 0, and where the two agree the float64 value is ~1e-10 or less -- far below the 2^-24 spacing of the operands that form
    it, so no fp32 evaluation (the reference's included: it is off by 100 % on 'mse/B1_C2_g24') has any relative accuracy.  Such a case
    is held to the bound relative to the value the quantity has when p and t differ by O(1): mean_c (p - t)^2 ~ 1 / C for the 'mse' loss,
    (2 / C) / B for an element of its gradient, r = 1 / B (1 for reduction='none') for an element of the soft 'ce' gradient r (p sum t - t)."""
    if c["kind"] == "mse" and c["gain"] == 24:
        return 1.0 / c["C"], 2.0 / (c["C"] * c["B"])
    if c["kind"] == "soft" and c["tkind"] == "prob" and c["gain"] == 24:
        return 0.0, 1.0 if c["reduction"] == "none" else 1.0 / c["B"]
    return 0.0, 0.0


def loss_err(c, got, want):
    return rel(got, want, floors(c)[0] * np.sqrt(np.size(want)))


def grad_err(c, got_sample, want_sample, gmax):
    """rel-L2 at gain 1; at gain 24 (rows can be ~0) the largest absolute error over the largest reference gradient of the case."""
    if c["gain"] == 1:
        return rel(got_sample, want_sample)
    d = np.abs(np.asarray(got_sample, np.float64) - np.asarray(want_sample, np.float64))
    return 0.0 if d.size == 0 or d.max() == 0.0 else float(d.max()) / (max(gmax, floors(c)[1]) + 1e-30)


def test_header_declares_the_criterion_entries_and_ops_wraps_them():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srhip.h")).read(), flags=re.S)
    for n in ENTRIES + ("SRHIP_REDUCE_NONE", "SRHIP_REDUCE_MEAN", "SRHIP_REDUCE_SUM"):
        assert re.search(r"\b%s\b" % n, src), n
    from semireward_amd import _lib, ops
    for n in ENTRIES:
        assert n in _lib.SIGNATURES, n
        assert len(_lib.SIGNATURES[n][1]) == len(re.search(r"\b%s\s*\(([^)]*)\)" % n, src).group(1).split(",")), n
    for n in ("ce_hard", "ce_soft", "consistency_mse", "consistency_l1"):
        assert callable(getattr(ops, n)), n
    assert (ops.REDUCE_NONE, ops.REDUCE_MEAN, ops.REDUCE_SUM) == (0, 1, 2)
    for n, v in (("NONE", 0), ("MEAN", 1), ("SUM", 2)):
        assert re.search(r"#define\s+SRHIP_REDUCE_%s\s+%d\b" % (n, v), src)


def test_invalid_criterion_arguments_return_error_codes_without_gpu():
    """The guards reject before any launch; the pointers are host addresses that are never dereferenced."""
    from semireward_amd import _lib
    lib = _lib.lib()
    a, E = 0x10000, -1
    soft = (lib.srhip_ce_soft, lib.srhip_consistency_mse, lib.srhip_consistency_l1)
    for fn in soft:
        assert fn(a, 10, a, 10, None, None, 1.0, 1, None, a, a, 10, 0, 10, None) == E            # B = 0
        assert fn(a, 10, a, 10, None, None, 1.0, 1, None, a, a, 10, 8, 0, None) == E             # C = 0
        assert fn(None, 10, a, 10, None, None, 1.0, 1, None, a, a, 10, 8, 10, None) == E         # no logits
        assert fn(a, 10, None, 10, None, None, 1.0, 1, None, a, a, 10, 8, 10, None) == E         # no targets
        assert fn(a, 9, a, 10, None, None, 1.0, 1, None, a, a, 10, 8, 10, None) == E             # logits row stride < C
        assert fn(a, 10, a, 9, None, None, 1.0, 1, None, a, a, 10, 8, 10, None) == E             # targets row stride < C
        assert fn(a, 10, a, 10, None, None, 1.0, 1, None, a, a, 9, 8, 10, None) == E             # dlogits row stride < C
        assert fn(a, 10, a, 10, None, None, 1.0, 3, None, a, a, 10, 8, 10, None) == E            # unknown reduction
        assert fn(a, 10, a, 10, None, None, 1.0, -1, None, a, a, 10, 8, 10, None) == E
        assert fn(a, 10, a, 10, None, None, 1.0, 0, None, None, None, 0, 8, 10, None) == E       # nothing asked for
    fn = lib.srhip_ce_hard
    assert fn(a, 10, a, None, None, 1.0, 1, None, a, a, 10, 0, 10, None) == E
    assert fn(a, 10, a, None, None, 1.0, 1, None, a, a, 10, 8, -3, None) == E
    assert fn(None, 10, a, None, None, 1.0, 1, None, a, a, 10, 8, 10, None) == E
    assert fn(a, 10, None, None, None, 1.0, 1, None, a, a, 10, 8, 10, None) == E
    assert fn(a, 9, a, None, None, 1.0, 1, None, a, a, 10, 8, 10, None) == E
    assert fn(a, 10, a, None, None, 1.0, 1, None, a, a, 9, 8, 10, None) == E
    assert fn(a, 10, a, None, None, 1.0, 7, None, a, a, 10, 8, 10, None) == E
    assert fn(a, 10, a, None, None, 1.0, 0, None, None, None, 0, 8, 10, None) == E


def test_python_surface_validates_before_any_launch():
    from semireward_amd.core.criterions import CELoss, ConsistencyLoss
    z, y, t = torch.zeros(4, 5), torch.zeros(4, dtype=torch.int64), torch.zeros(4, 5)
    with pytest.raises(ValueError, match="'ce', 'mse', 'l1'"):
        ConsistencyLoss()(z, t, name="kl")
    with pytest.raises(ValueError, match="'none', 'mean', 'sum'"):
        CELoss()(z, y, reduction="batchmean")
    with pytest.raises(ValueError, match="'none', 'mean', 'sum'"):
        CELoss()(z, t, reduction="batchmean")
    with pytest.raises(ValueError, match="shape"):
        ConsistencyLoss()(z, y, name="mse")


def test_criterion_kernels_use_no_scratch(tmp_path):
    """Compiled with the resource remarks on (as test_precise_kernels_keep_their_register_budget does): every kernel of the translation
    unit -- 4 kinds x {16-byte, scalar access} x {register-resident row, re-read row} and the reduction -- has no scratch and no spill."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "semireward_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-c",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "o.o"), os.path.join(csrc, "criterions.hip")],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    assert len([k for k in out if "criterion_kernel" in k]) == 16 and len([k for k in out if "criterion_reduce_kernel" in k]) == 1, sorted(out)
    for k, v in out.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["Occupancy [waves/SIMD]"] >= 4, (k, v)


def test_fixture_covers_the_cases_and_is_small(golden):
    g = CC.load(golden("criterions"))
    cases = CC.cases()
    assert sorted(g) == sorted(c["id"] for c in cases) and len(g) == len(cases) == 4 * 4 * 2 * 18 + 2
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "criterions.npz")) < 1 << 20
    for c in cases:
        n = c["B"] * c["C"]
        assert g[c["id"]]["stride"] == CC.grad_stride(n) and g[c["id"]]["grad"].size == len(range(0, n, CC.grad_stride(n)))
        assert g[c["id"]]["loss"].size == (c["B"] if c["reduction"] == "none" else 1)
    l1 = [c for c in cases if c["kind"] == "l1" and c["B"] * c["C"] >= 10]
    for c in l1[:4]:
        i = CC.inputs(c)
        assert int((i["logits"] == i["targets"]).sum()) == 5                      # the exact ties are there
    m = CC.inputs(next(c for c in cases if c["mkind"] == "mask2" and c["B"] == 67))
    assert (m["mask"] == 0).any() and (m["mask2"] == 0).any() and (m["mask"] * m["mask2"] > 0).any()
    assert not CC.inputs(next(c for c in cases if c["mkind"] == "allzero"))["mask"].any()


def test_fixture_is_self_consistent(golden):
    """The float64 restatement reproduces what the reference computed in fp32, case by case, to REF_FP32_ERR."""
    g = CC.load(golden("criterions"))
    worst_l, worst_g = (0.0, ""), (0.0, "")
    for c in CC.cases():
        inp, ref = CC.inputs(c), g[c["id"]]
        loss, grad = CC.restate64(c, inp)
        el = loss_err(c, ref["loss"], loss)
        eg = grad_err(c, ref["grad"], grad.reshape(-1)[::ref["stride"]], float(np.abs(grad).max()))
        worst_l, worst_g = max(worst_l, (el, c["id"])), max(worst_g, (eg, c["id"]))
        if c["mkind"] == "allzero":
            assert not ref["loss"].any() and not ref["grad"].any()
    print("fixture vs float64: worst loss %.3g (%s), worst gradient %.3g (%s)" % (worst_l + worst_g))
    assert worst_l[0] <= REF_FP32_ERR and worst_g[0] <= REF_FP32_ERR, (worst_l, worst_g)


def test_hard_label_mean_path_still_calls_masked_ce(monkeypatch):
    """ConsistencyLoss(name='ce') and CELoss(reduction='mean') with integer targets: the ONE ops.masked_ce call with the arguments of
    old, and none of the new launches."""
    from semireward_amd import ops
    from semireward_amd.core import criterions
    calls = []
    monkeypatch.setattr(ops, "masked_ce", lambda *a: calls.append(a))
    for n in ("ce_hard", "ce_soft", "consistency_mse", "consistency_l1"):
        monkeypatch.setattr(ops, n, lambda *a, n=n: pytest.fail("%s called on the hard-label mean path" % n))
    z, y = torch.zeros(6, 10), torch.arange(6)
    m, m2, out = torch.ones(6), torch.ones(6), torch.empty(6, 10)
    loss, dl = criterions.ConsistencyLoss()(z, y, "ce", m, m2, grad_scale=0.5, dl_out=out)
    a = calls.pop()
    assert len(a) == 9 and a[2] is m and a[3] is m2 and a[4] == 0.5 and a[6] is out and dl is out and a[7:] == (6, 10) and loss.shape == ()
    loss, dl = criterions.ConsistencyLoss()(z, y, mask=m, want_grad=False)
    a = calls.pop()
    assert a[2] is m and a[3] is None and a[6] is None and dl is None
    loss, dl = criterions.CELoss()(z, y)
    a = calls.pop()
    assert a[2] is None and a[3] is None and a[4] == 1.0 and a[6] is dl and tuple(dl.shape) == (6, 10) and not calls
    src = open(os.path.join(ROOT, "semireward_amd", "core", "criterions.py")).read()
    assert src.count("ops.masked_ce(") == 2 and "assert reduction ==" not in src and "assert name ==" not in src
