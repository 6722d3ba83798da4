"""What tests/_mlp_fused_cases.py promises, stated without a GPU: its two new constants are 8 times what the float32 LayerNorm restatements
measure; its inputs are what its docstring says (clearly non-zero GELU outputs in every hidden chunk, every factor combination, valid plans);
the float32 restatement of every case passes the very verify() the GPU tests hold the kernels to, with no element excused (the large-M cases
whole: no row sample is drawn); verify() rejects every planted fault in every case the fault changes; and the whole-tensor norms of
test_mlp_fused / test_mlp_fused_proj, at those tests' own largest common shape, let the faults of NORM_BLIND pass."""
import numpy as np
import pytest
import torch

import _mlp_fused_cases as C

ids = lambda c: c["id"]      # noqa: E731


def test_import_did_not_touch_the_device():
    assert not torch.cuda.is_initialized()


def test_committed_constants_are_eight_times_the_measurement():
    c_stat, c_norm = C.measure_constants()
    print("C_STAT: measured %.4f committed %.4f x 8 = %.3f;  C_NORM: measured %.4f committed %.4f x 8 = %.3f" % (
        c_stat, C.C_STAT_MEASURED, C.C_STAT, c_norm, C.C_NORM_MEASURED, C.C_NORM))
    assert C.C_STAT == 8.0 * C.C_STAT_MEASURED and C.C_NORM == 8.0 * C.C_NORM_MEASURED
    assert 4.0 * c_stat <= C.C_STAT <= 16.0 * c_stat
    assert 4.0 * c_norm <= C.C_NORM <= 16.0 * c_norm
    # any order of the 384 additions of a row sum is within 383 u sum|x| to first order: the bound asks for less
    assert C.C_STAT < C.D - 1 and C.C_NORM < C.D - 1


def test_number_format_helpers():
    v = np.array([1.0, 1.00390625, 1.01171875, -3.0e-5, 255.5, 0.0], np.float32)        # 1 + 2^-8: a tie, to even (down); 1 + 3 * 2^-8: a tie, up
    want = torch.from_numpy(v).to(torch.bfloat16).float().numpy()
    assert np.array_equal(C.bf16_round(v), want) and np.array_equal(C.bf16_round64(v.astype(np.float64)), want.astype(np.float64))
    r = np.random.Generator(np.random.PCG64(3)).standard_normal(100000).astype(np.float32)
    assert np.array_equal(C.bf16_round(r), torch.from_numpy(r).to(torch.bfloat16).float().numpy())
    assert np.array_equal(C.from_bits(C.to_bits(C.bf16_round(r))), C.bf16_round(r))
    assert np.array_equal(C.half_ulp_bf16(np.array([1.0, 1.99, 2.0, 0.75, 0.0])), np.array([2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 2.0 ** -134]))
    # flip_bf16: 1 + 2^-8 is the first rounding boundary of [1, 2), 1 - 2^-9 the last one below it
    assert C.flip_bf16(np.array([1.0 + 2.0 ** -9]), np.array([2.0 ** -11]))[0] == 0.0
    assert C.flip_bf16(np.array([1.0 + 2.0 ** -8 - 2.0 ** -12]), np.array([2.0 ** -11]))[0] > 2.0 ** -7
    assert C.flip_bf16(np.array([1.0 + 2.0 ** -20]), np.array([2.0 ** -11]))[0] == 0.0              # 1.0 itself is no boundary ...
    assert C.flip_bf16(np.array([1.0 + 2.0 ** -20]), np.array([2.0 ** -9 + 2.0 ** -19]))[0] > 0.0  # ... 1 - 2^-9 is one
    assert C.flip_bf16(np.array([0.0, 1e-7]), np.array([1e-6, 1e-6])).min() > 0.0                  # (a sign change counts)


@pytest.mark.parametrize("c", C.CASES, ids=ids)
def test_inputs_are_what_the_cases_say(c):
    share = C.share_clear(c)
    assert share.shape == (c["Hd"] // C.CH,) and float(share.min()) >= 0.3, share      # |GELU| >= 0.25 on at least 30 % of every chunk
    L = C.Launch(c)
    o = L.o
    assert abs(float(o["x"][:, 7].mean()) - 3.0) < 1.5 and (o["x"] != 0).all()
    r1, r2 = L.r1, L.r2
    if c["entry"] == "dense":
        assert (r2 is not None) == c["scale"]
        if r2 is not None:
            assert set(np.unique(r2)) <= set(C.FACTORS.tolist()) and r2[0] != 0 and (len(r2) == 1 or r2[1] == 0)
        return
    assert (r1 is not None) == (r2 is not None) == c["fac"]
    if not c["fac"]:
        return
    assert set(np.unique(r1)) | set(np.unique(r2)) <= set(C.FACTORS.tolist())
    combos = set(zip((r1 != 0).tolist(), (r2 != 0).tolist()))
    if c["entry"] != "planned":
        assert combos == {(False, False), (False, True), (True, False), (True, True)}, combos
        if c["ao_scaled"]:
            assert (L.ao[L.rows(r1) == 0] == 0).all()
    else:
        B, n = c["B"], c["n_mlp"]
        assert sorted(L.plan[1:].tolist()) == list(range(B)) and L.plan[0] == n == int((r2 != 0).sum())
        assert (r2[L.plan[1:1 + n]] != 0).all() and (r2[L.plan[1 + n:]] == 0).all()
        vrow = L.vrow()
        assert sorted(vrow.tolist()) == list(range(c["M"]))
        # a tile that straddles the boundary is heavy as a whole; every light row's MLP branch is dropped
        assert (L.rows(r2)[L.light()] == 0).all()


def test_planned_cases_cover_every_factor_combination_and_both_kinds_of_tile():
    for N, B in ((257, 3), (5, 30), (1, 130), (257, 130)):
        cs = [c for c in C.PLANNED if (c["rps"], c["B"]) == (N, B)]
        combos, straddle, light2 = set(), False, False
        for c in cs:
            L = C.Launch(c)
            combos |= set(zip((L.r1 != 0).tolist(), (L.r2 != 0).tolist()))
            edge = c["n_mlp"] * N
            straddle |= edge % C.FBM != 0 and 0 < edge < c["M"]
            light2 |= bool((L.light() & (L.vrow() >= C.GRID * C.FBM)).any())
        assert straddle, (N, B)
        if N * B < C.GRID * C.FBM:
            assert combos == {(False, False), (False, True), (True, False), (True, True)} and {c["n_mlp"] for c in cs} >= {0, 1, B - 1, B}, (N, B)
        assert light2 == (N * B > C.GRID * C.FBM)


@pytest.mark.parametrize("c", C.CASES, ids=ids)
def test_float32_restatement_is_within_the_bound(c):
    for reverse in ((False, True) if c["M"] < 1000 else (False,)):
        ratios = C.verify(C.restate(C.Launch(c), reverse=reverse))
        print("%s%s: max |restatement - float64| / bound: %s" % (c["id"], " reversed" if reverse else "", ", ".join("%s %.3f" % kv for kv in ratios.items())))
        assert max(ratios.values()) <= 1.0


# ---- planted faults ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.CASES, ids=ids)
def test_checker_rejects_each_planted_fault(c):
    for fault in C.FAULTS:
        if not C.fault_applies(fault, c):
            continue
        with pytest.raises(AssertionError) as e:
            C.verify(C.restate(C.Launch(c), fault))
        print("%s -> %s" % (fault, str(e.value)[:260]))


def test_every_planted_fault_meets_a_case_of_every_entry_point_it_can_occur_in():
    where = {f: {c["entry"] for c in C.CASES if C.fault_applies(f, c)} for f in C.FAULTS}
    every, projs = {"dense", "proj", "strided", "planned"}, {"proj", "strided", "planned"}
    assert where == {"chunk_dropped": every, "b1_of_next_chunk": every, "b2_unscaled": every, "bp_unscaled": projs, "factor_one_row_early": every - {"planned"},
                     "stale_ring_slot": every, "permlane_pairing": projs, "save_rows_off_by_one": {"dense"}, "s_pre_holds_gelu": {"dense"},
                     "light_tile_adds_b2": {"planned"}, "plan_on_x_not_ao": {"planned"}, "ln_next_at_virtual_row": {"planned"},
                     "clamped_row_stored_twice": every, "xn_truncated_in_one_wave": {"dense"}}, where
    assert len(C.UNDETECTABLE) == 2          # named, with the reasons, beside FAULTS


# ---- what the whole-tensor norms of tests/test_gpu_kernels.py read ------------------------------------------------------------------------------
def _relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def _formula64(L):
    """the float64 formula without any rounding point (what those tests call the fp32 torch reference)"""
    o = {k: v.astype(np.float64) for k, v in L.o.items()}
    r1, r2 = L.rows(L.r1).astype(np.float64)[:, None], L.rows(L.r2).astype(np.float64)[:, None]
    x1 = o["x"] + r1 * (L.ao.astype(np.float64) @ o["Wp"].T + o["bp"]) if L.proj else o["x"]
    _, _, xhat = C.ln64(x1)
    return x1 + r2 * (C.gelu64((xhat * o["gam"] + o["bet"]) @ o["W1"].T + o["b1"]) @ o["W2"].T + o["b2"])


def _old_criteria(Lf, Lc, want):
    """{criterion: (figure, limit)} of test_mlp_fused / test_mlp_fused_proj for the outputs in Lf, with the clean restatement Lc standing for the
    unfused launches those tests compare with (same rounding points); a criterion holds when figure < limit"""
    x0, xf, xu = Lf.o["x"], Lf.got("xo"), Lc.got("xo")
    out = {"vs formula": (_relerr(xf - x0, want - x0), 6e-3)}
    dead = (Lf.rows(Lf.r2) == 0) & (Lf.rows(Lf.r1) == 0)
    out["dropped rows exact"] = (float(not np.array_equal(xf[dead], x0[dead])), 0.5)
    if not Lf.proj:
        out["vs unfused"] = (_relerr(xf - x0, xu - x0), 1.5e-3)
        for k, lim in (("s_ln2", 1e-3), ("s_pre", 2e-3), ("s_h", 2e-3)):
            g = Lf.got(k)
            out[k] = (_relerr(np.where(np.isnan(g), 0.0, g), Lc.got(k)), lim)                  # (those buffers start as zeros there)
        for k in ("s_mean", "s_rstd"):
            g, w = np.nan_to_num(Lf.got(k)[0]), Lc.got(k)[0]
            out[k] = (float((np.abs(g - w) / (1e-6 + 1e-5 * np.abs(w))).max()), 1.0)
        return out
    out["vs unfused"] = (_relerr(xf - x0, xu - x0), 4e-3)
    out["x vs unfused"] = (_relerr(xf, xu), 3e-3)
    lf, lu = Lf.got("ln"), Lc.got("ln")
    dl = np.abs(lf - lu)
    out["ln_next max"] = (float(dl.max() / (2.0 ** -7 * np.abs(lu).max())), 1.0 + 1e-9)
    out["ln_next share"] = (float((dl > 0).mean()), 0.02)
    r1, r2 = Lf.rows(Lf.r1), Lf.rows(Lf.r2)
    for k, m in (("only MLP dropped", (r1 != 0) & (r2 == 0)), ("only attention dropped", (r1 == 0) & (r2 != 0))):
        out[k] = (_relerr(xf[m] - x0[m], xu[m] - x0[m]), 4e-3)
    return out


def _their_inputs(M, Hd, rps, proj):
    """the operands and factors of test_mlp_fused / test_mlp_fused_proj (tests/test_gpu_kernels.py), seed by seed"""
    def rnd(*shape, seed, scale=1.0):
        return (scale * np.random.Generator(np.random.PCG64(seed)).standard_normal(shape)).astype(np.float32)
    x, ao32 = rnd(M, C.D, seed=1), rnd(M, C.D, seed=11, scale=0.7)
    x[:, 7] += 3.0
    ao32[:, 300] += 2.0
    o = dict(x=x, ao32=ao32, Wp=C.bf16_round(rnd(C.D, C.D, seed=12, scale=0.06)), bp=rnd(C.D, seed=13, scale=0.2),
             gam=rnd(C.D, seed=2, scale=0.2) + np.float32(1.0), bet=rnd(C.D, seed=3, scale=0.1), W1=C.bf16_round(rnd(Hd, C.D, seed=4, scale=0.05)),
             W2=C.bf16_round(rnd(C.D, Hd, seed=5, scale=0.03)), b1=rnd(Hd, seed=6, scale=0.1), b2=rnd(C.D, seed=7, scale=0.1),
             gn=rnd(C.D, seed=21, scale=0.3) + np.float32(1.0), bn=rnd(C.D, seed=22, scale=0.2))
    ns = (M + rps - 1) // rps
    rng = np.random.Generator(np.random.PCG64(8))
    if not proj:
        return o, (None, rng.choice([0.0, 1.0 / 0.9], size=ns).astype(np.float32))
    return o, (rng.choice([0.0, 1.0 / 0.95], size=ns, p=[0.3, 0.7]).astype(np.float32), rng.choice([0.0, 1.0 / 0.9], size=ns).astype(np.float32))


def test_whole_tensor_norms_are_blind_to_some_of_the_faults():
    """At M = 257 * 40 + 5 = 10285, Hd = 1536, rows_per_sample = 257 -- the largest shape test_mlp_fused runs and one test_mlp_fused_proj runs
    (its larger ones move a norm by less still) -- on those tests' own inputs and with save_rows = 2 * 257 as there: every criterion of those
    tests, fault by fault.  The faults all of them let pass are NORM_BLIND of _mlp_fused_cases.py; test_checker_rejects_each_planted_fault
    rejects every one of them in every case."""
    M, Hd, rps = 257 * 40 + 5, 1536, 257
    blind = []
    for c in (C._dense(M, Hd, rps, True, 2 * rps), C._proj(M, Hd, rps, True, False, True)):
        o, factors = _their_inputs(M, Hd, rps, c["entry"] == "proj")
        new = lambda: C.Launch(c, o=o, factors=factors)      # noqa: E731
        clean = C.restate(new())
        want = _formula64(clean)
        ok = _old_criteria(clean, clean, want)
        print("%s clean: %s" % (c["entry"], ", ".join("%s %.2e" % (k, v) for k, (v, _) in ok.items())))
        assert all(v < lim for v, lim in ok.values()), ok
        for fault in C.FAULTS:
            if not C.fault_applies(fault, c, new()) or fault == "clamped_row_stored_twice":     # (those tests allocate no padding to look at)
                continue
            res = _old_criteria(C.restate(new(), fault), clean, want)
            failed = [k for k, (v, lim) in res.items() if not v < lim]
            print("%s %-22s %s -> %s" % (c["entry"], fault, ", ".join("%s %.2e" % (k, v) for k, (v, _) in res.items()),
                                          "caught by " + ", ".join(failed) if failed else "PASSES"))
            if not failed:
                blind.append("%s:%s" % (c["entry"], fault))
    assert tuple(blind) == C.NORM_BLIND, blind
