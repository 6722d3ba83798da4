"""What tests/_enc_cases.py promises, stated without a GPU: every kernel and dispatcher branch of csrc/enc_ops.hip and csrc/optim.hip is named by a
case; the float64 references agree with float64 autograd (embedding, post-LN, mean pool, GELU) and with oracle/optim_ref.py (AdamW);
ops.site_key / ops.Drop reproduce oracle.bert_ref.keep_mask; the float32 restatement of every case, in both summation orders, passes the very
verify functions the GPU tests hold the kernels to; the committed constants are eight times a fresh measurement; and each of thirteen planted
faults is rejected -- with what test_embed_postln_meanpool / test_adamw_flat_matches_oracle would have read of it (NORM_BLIND)."""
import numpy as np
import pytest
import torch

import _enc_cases as E
from oracle import bert_ref as BR
from oracle import optim_ref as OR
from semireward_amd import ops

f8 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))          # noqa: E731


# ---- 1. coverage -----------------------------------------------------------------------------------------------------------------------------------
def test_every_kernel_and_dispatcher_branch_is_named_by_a_case():
    named = " | ".join(c["kernel"] for _, c in E.all_cases())
    for nv in (1, 3, 6):
        for k in ("embed_ln_fwd_kernel<%d>", "embed_ln_bwd_kernel<%d>", "postln_fwd_kernel<%d>", "postln_bwd_kernel<%d, 2>"):
            assert k % nv in named, k % nv
    for k in ("postln_bwd_kernel<1, 8>", "postln_bwd_kernel<1, 8> part", "postln_bwd_kernel<6, 2> part", "meanpool_fwd_kernel", "meanpool_bwd_kernel", "gelu_f32_kernel",
              "gelu_bwd_f32_kernel", "dropout_cast_kernel", "mask_len_kernel", "adamw_flat_kernel dyn", "adamw_flat_kernel by-value", "sumsq_part_kernel",
              "clip_coef_kernel"):
        assert k in named, k
    # the dispatcher of postln_bwd: RPW = 8 from 16384 rows on, and no smaller case claims it
    assert all((c["M"] >= 16384) == (c["rpw"] == 8) for c in E.PLN_BWD_CASES) and min(c["M"] for c in E.PLN_BWD_CASES if c["rpw"] == 8) == 16384 + 5
    for D in (128, 384, 768):
        cs = [c for c in E.PLN_BWD_CASES if c["D"] == D and c["rpw"] == 2]
        assert {c["M"] for c in cs} == {1, 9, 69} and {c["n_rep"] for c in cs} == {0, 1, 16} and {c["p"] for c in cs} == {0.0, 0.1} and {c["alias"] for c in cs} == {False, True}
        assert any(c["M"] == 9 and c["n_rep"] == 16 for c in cs)                           # 2 workgroups, 16 copies
        cs = [c for c in E.PLN_FWD_CASES if c["D"] == D]
        assert {c["M"] for c in cs} == {1, 7, 8, 9, 69} and {c["form"] for c in cs} == set(E.FORMS) and {c["eps"] for c in cs} == {1e-12, 1e-5}
        cs = [c for c in E.EMBED_CASES if c["D"] == D]
        assert {(c["B"], c["L"]) for c in cs} == {(1, 1), (3, 23), (2, 33)} and {(c["gather"], c["p"]) for c in cs} == {(False, 0.0), (True, 0.1), (False, 0.1), (True, 0.0)}
    for M in (1, 7, 8, 9, 69):
        assert {c["form"] for c in E.PLN_FWD_CASES if c["M"] == M} == set(E.FORMS)
    fams = set()
    for c in E.PLN_FWD_CASES:
        fams |= {(c["D"], int(f)) for f in E.PlnFwdLaunch(c, "cpu").fam}
    assert fams == {(D, f) for D in (128, 384, 768) for f in range(4)}
    L = E.EmbedLaunch(E.EMBED_CASES[5], "cpu")
    assert (L.row_id == E.PAD_ID).sum() >= 3 and len(set(L.row_id.tolist())) < len(L.row_id) and L.ids_base.shape[1] > L.c["L"] and L.pos.shape[0] > L.c["L"]
    assert {c["L"] for c in E.POOL_CASES} == {1, 3, 4, 16, 17, 19, 35} and {c["D"] for c in E.POOL_CASES} == {64, 128, 768}
    assert {(c["seq_len"], c["p"] > 0) for c in E.POOL_CASES} == {(a, b) for a in (False, True) for b in (False, True)}
    assert any((c["B"] * c["L"] * c["D"]) % 256 for c in E.POOL_CASES)
    assert {c["n"] for c in E.GELU_CASES} == {1, 255, 257, 4099} and {(c["n"], c["p"]) for c in E.CAST_CASES} == {(n, p) for n in (2, 510, 514) for p in (0.0, 0.1, 0.5)}
    assert {c["L"] for c in E.MASK_CASES} == {1, 63, 64, 65, 512}
    for key, vals in (("table", {"dense", "gaps"}), ("step", {1, 2, 1000}), ("zero_grad", {False, True}), ("grad_scale", {1.0, 0.25}), ("clip", {False, True}),
                      ("ema_m", {0.9, 0.999}), ("dyn", {False, True})):
        assert {c[key] for c in E.ADAM_CASES} == vals, key
    assert {(c["pb"], c["ema"]) for c in E.ADAM_CASES} == {(a, b) for a in (False, True) for b in (False, True)}
    assert set(E.SIZES) == {1, 255, 256, 257, 4096, 4097, 5000} and (0.0, 0.0) in set(zip(E.LR_T, E.WD_T)) and any(w == 0.0 and l > 0 for l, w in zip(E.LR_T, E.WD_T))
    assert {c["n"] for c in E.CLIP_CASES} == {1, 1023, 1024, 1025, 300001} and {(c["pre"], c["below"]) for c in E.CLIP_CASES} == {(a, b) for a in (1.0, 0.5) for b in (False, True)}
    assert any(c["dominant"] for c in E.CLIP_CASES)


# ---- 2. references ---------------------------------------------------------------------------------------------------------------------------------
def test_site_key_and_drop_reproduce_the_oracle_keep_mask():
    for seed, site, p, shape in (((3 << 32) + 9, 1, 0.1, (5, 19, 128)), (E.SEED, E.SITE_LN, 0.1, (69, 384)), (0xFEDCBA9876543210, 4 * 11 + 2, 0.5, (514,)),
                                 (1, 0, 0.25, (7, 6))):
        assert ops.site_key(seed, site) == BR.site_key(seed, site)
        d = ops.Drop(seed, site, p)
        n = int(np.prod(shape))
        idx = np.arange(n, dtype=np.uint64)
        h = np.array([ops._fmix32((int(i >> 1) * 0x9E3779B1 + d.key) & 0xFFFFFFFF) for i in idx[::2]], dtype=np.uint64).repeat(2)[:n]       # drop_keep of csrc/common.h
        keep = np.where(idx & 1, h >> 16, h & 0xFFFF) >= (d.thresh >> 16)
        assert np.array_equal(keep.reshape(shape), BR.keep_mask(seed, site, shape, p)) and d.scale == 1.0 / (1.0 - p)
        assert 0.6 * p < 1.0 - keep.mean() < 1.4 * p


def test_float64_references_agree_with_float64_autograd():
    rng = np.random.default_rng(3)
    # LayerNorm forward / backward as functions
    M, D = 7, 128
    y, g, b, dy = (torch.from_numpy(rng.standard_normal(s)).requires_grad_() for s in ((M, D), (D,), (D,), (M, D)))
    r = torch.nn.functional.layer_norm(y, (D,), g, b, 1e-5)
    r.backward(dy.detach())
    R = E.ln_fwd_ref(y.detach().numpy(), np.zeros((M, D)), np.abs(y.detach().numpy()), g.detach().numpy(), b.detach().numpy(), 1e-5)
    assert np.abs(R["o"] - r.detach().numpy()).max() < 1e-12
    dx, _ = E.ln_bwd_ref(dy.detach().numpy(), R["xh"], R["rs"], g.detach().numpy())
    assert np.abs(dx - y.grad.numpy()).max() < 1e-12
    # the embedding launch: forward to 1e-12; the backward reads fp32-rounded statistics, so it agrees to a few 2^-24
    for c in (E.EMBED_CASES[4], E.EMBED_CASES[5], E.EMBED_CASES[10]):
        L = E.EmbedLaunch(c, "cpu")
        word, pos, typ, g, b = (f8(a).requires_grad_() for a in (L.word, L.pos, L.typ, L.g, L.b))
        rows = torch.from_numpy(L.ids[L.idx if L.idx is not None else np.arange(c["B"])])
        e = torch.nn.functional.embedding(rows, word, padding_idx=E.PAD_ID) + pos[:c["L"]][None] + typ[0]
        r = torch.nn.functional.layer_norm(e, (c["D"],), g, b, L.eps).reshape(L.M, c["D"]) * f8(L.keep) * float(L.scale)
        assert np.abs(L.ex["x"][0] - r.detach().numpy()).max() < 1e-12
        r.backward(f8(L.dy))
        for k, t in (("dword", word), ("dpos", pos), ("dtype0", typ), ("dgamma", g), ("dbeta", b)):
            want = t.grad.numpy()[0] if k == "dtype0" else t.grad.numpy()
            got = L.ex[k][0] - L.pre[k].astype(np.float64)
            assert np.abs(got - want).max() < 2e-6 * (1.0 + np.abs(want).max()), (c["id"], k, np.abs(got - want).max())
        assert not word.grad[E.PAD_ID].any()
    # post-LN backward launch, direct and through the partial copies
    for c in (E.PLN_BWD_CASES[20], E.PLN_BWD_CASES[22]):
        L = E.PlnBwdLaunch(c, "cpu")
        y, g = f8(L.y).requires_grad_(), f8(L.g).requires_grad_()
        torch.nn.functional.layer_norm(y, (c["D"],), g, torch.zeros(c["D"], dtype=torch.float64), 1e-12).backward(f8(L.dy))
        assert np.abs(L.ex["dx"][0] - y.grad.numpy()).max() < 2e-6 * (1.0 + y.grad.abs().max().item())
        got = (L.ex["part"][0] - L.pre)[:, 0].sum(0) if c["n_rep"] else L.ex["dgamma"][0] - L.pre[0]
        assert np.abs(got - g.grad.numpy()).max() < 2e-6 * (1.0 + g.grad.abs().max().item())
    # mean pool
    for c in E.POOL_CASES[20:24]:
        L = E.PoolLaunch(c, "cpu")
        x = f8(L.x).requires_grad_()
        r = (x * f8(L.keep & L.valid) * float(L.scale)).sum(1) / f8(L.Ls)[:, None]
        r.backward(f8(L.df))
        assert np.abs(L.ex["feat"][0] - r.detach().numpy()).max() < 1e-12 and np.abs(L.ex["dx"][0] - x.grad.numpy()).max() < 1e-12
    # GELU
    L = E.GeluLaunch(E.GELU_CASES[2], "cpu")
    v = f8(L.v).requires_grad_()
    r = torch.nn.functional.gelu(v)
    r.backward(f8(L.dout))
    assert np.abs(L.ex["out"][0] - r.detach().numpy()).max() < 1e-9 and np.abs(L.ex["dpre"][0] - v.grad.numpy()).max() < 1e-12


def test_adamw_reference_agrees_with_the_oracle():
    rng = np.random.default_rng(4)
    for step, lr, wd in ((1, 5e-4, 5e-4), (2, 1e-3, 0.0), (1000, 2.5e-4, 0.05)):
        p, g, m, v = (rng.standard_normal(300) * s for s in (0.05, 0.1, 0.01, 1.0))
        v = 1e-4 * np.abs(v)
        P, Mo, Vo = f8(p).clone(), f8(m).clone(), f8(v).clone()
        OR.adamw_step(P, f8(g), Mo, Vo, step, lr, wd)
        R = E.adamw_ref(p, g, m, v, 1.0 - lr * wd, lr / (1.0 - 0.9 ** step), 0.9, 1.0 - 0.9, 0.999, 1.0 - 0.999, np.sqrt(1.0 - 0.999 ** step), 1e-8)
        for got, want in ((R["p"], P), (R["m"], Mo), (R["v"], Vo)):
            assert np.abs(got - want.numpy()).max() < 1e-13
        assert (R["U"] >= np.abs(R["pi"] - R["p"]) * (1 - 1e-12)).all()
    # the bias corrections the references use are the library's own fp32 ones
    bc1, bc2s = ops.adam_bias_corrections(0.9, 0.999, 1000)
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))            # (the powers are taken of the fp32 betas)
    assert abs(bc1 - (1 - b1 ** 1000)) < 2e-7 and abs(bc2s - np.sqrt(1 - b2 ** 1000)) < 2e-7 and bc1 == float(np.float32(bc1))


# ---- 3. the restatement of every case passes ---------------------------------------------------------------------------------------------------------
def check(H):
    assert all(v <= 1.0 for v in H.values()), H
    return H


@pytest.mark.parametrize("cls,c", E.all_cases(), ids=[c["id"] for _, c in E.all_cases()])
def test_restatement_passes_verify(cls, c):
    for order in E.ORDERS:
        L = cls(c, "cpu")
        L.restate(order=order)
        H = check(L.verify())
        print("restatement %s %s %s" % (c["id"], order, {k: round(v, 4) for k, v in H.items()} or "same bits"))


# ---- 4. constants --------------------------------------------------------------------------------------------------------------------------------------
def test_committed_constants_are_eight_times_the_measurement():
    got = dict(E.measure_constants(), **E.measure_intrinsics())
    assert set(got) == set(E.NAMES)
    for k in E.NAMES:
        v, committed, measured = got[k], getattr(E, k), getattr(E, k + "_MEASURED")
        print("%s: measured %.4f committed %.4f x 8 = %.3f" % (k, v, measured, committed))
        assert committed == 8.0 * measured and 4.0 * v <= committed <= 16.0 * v, k


# ---- 5. planted faults -----------------------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def case(cs, **kw):
    return next(c for c in cs if all(c[k] == v for k, v in kw.items()))


EMB_T = dict(x=2e-6, xb=4e-3, dword=1e-5, dpos=1e-5, dtype0=1e-5, dgamma=1e-5, dbeta=1e-5)
# fault -> (launch class, the case verify() must reject it on, the old test's shape / form (None: the old tests never launch the path or read the
# output -- the reason follows), the thresholds the old test reads its outputs with)
FAULTS = {
    "one_pass_variance": (E.PlnFwdLaunch, case(E.PLN_FWD_CASES, D=768, M=69, form="out_of_place"), E.OLD_PLN_FWD, dict(x=2e-6, xb=4e-3)),
    "meanpool_divides_by_L": (E.PoolLaunch, case(E.POOL_CASES, L=19, seq_len=True), E.OLD_POOL, dict(feat=2e-6, dx=2e-6)),
    "dropout_scale_left_off_bf16_branch": (E.PlnBwdLaunch, case(E.PLN_BWD_CASES, M=69, D=384, n_rep=0, p=0.1), E.OLD_PLN_BWD, dict(dx=1e-5, dxb=4e-3, dgamma=1e-5, dbeta=1e-5)),
    "dropout_pair_swapped": (E.EmbedLaunch, case(E.EMBED_CASES, D=384, B=3, p=0.1, gather=True), E.OLD_EMBED, EMB_T),
    "pad_receives_gradient": (E.EmbedLaunch, case(E.EMBED_CASES, D=128, B=3, p=0.0, gather=False), E.OLD_EMBED, EMB_T),
    "last_partial_workgroup_missing_from_dgamma": (E.EmbedLaunch, case(E.EMBED_CASES, D=768, B=3, p=0.1, gather=False), E.OLD_EMBED, EMB_T),
    "part_copy_overwritten": (E.PlnBwdLaunch, case(E.PLN_BWD_CASES, M=9, D=128, n_rep=16), None, "no test launches srhip_postln_bwd_part against a reference"),
    "second_row_of_odd_pair_written": (E.PlnFwdLaunch, case(E.PLN_FWD_CASES, D=128, M=69, form="x_none"), None,
                                       "M = 95 is odd there, but the buffers end at row M: nothing reads what lands behind them"),
    "chunk_tail_skipped": (E.AdamLaunch, E.ADAM_CASES[0], E.OLD_ADAM, dict(p=2e-6)),
    "weight_decay_after_the_update": (E.AdamLaunch, E.ADAM_CASES[2], E.OLD_ADAM, dict(p=2e-6)),
    "bc1_and_bc2_swapped": (E.AdamLaunch, E.ADAM_CASES[1], E.OLD_ADAM, dict(p=2e-6)),
    "ema_one_minus_m_in_float32": (E.AdamLaunch, E.ADAM_CASES[5], None, "the test hands the launch an ema buffer and never reads it"),
    "clip_norm_misses_the_last_partition": (E.ClipLaunch, case(E.CLIP_CASES, n=300001, below=True), None,
                                            "srhip_clip_grad_coef is reached only through a whole-algorithm golden trace"),
}


@pytest.mark.parametrize("fault", list(FAULTS), ids=list(FAULTS))
def test_verify_rejects_each_planted_fault(fault):
    cls, c = FAULTS[fault][:2]
    G = cls(c, "cpu")
    G.restate()
    check(G.verify())
    L = cls(c, "cpu")
    L.restate(fault=fault)
    with pytest.raises(AssertionError) as e:
        L.verify()
    print("%s at %s -> %s" % (fault, c["id"], str(e.value)[:240]))


def old_test_reading(fault):
    """(True when the old test would have passed the fault, one line of figures)"""
    cls, _, old, thr = FAULTS[fault]
    if old is None:
        return True, "not read: " + thr
    L = cls(old, "cpu")
    L.restate(fault=fault)
    G, figs, ok = L.got(), [], True
    for k, t in thr.items():
        want, got = L.ex[k][0], G[k]
        if cls is E.AdamLaunch:                                   # np.testing.assert_allclose(rtol=2e-6, atol=1e-8)
            excess = float((np.abs(got - want) - (1e-8 + t * np.abs(want))).max())
            figs.append("p: largest |diff| - (1e-8 + 2e-6 |want|) = %.2e" % excess)
            ok &= excess <= 0.0
        else:
            pre = 0.0
            if cls is E.EmbedLaunch and k in L.pre:
                pre = L.pre[k].astype(np.float64)
            elif cls is E.PlnBwdLaunch and k in ("dgamma", "dbeta"):
                pre = L.pre[("dgamma", "dbeta").index(k)].astype(np.float64)
            r = rel(got - pre, want - pre)                        # (the old test starts its accumulators from zero)
            figs.append("%s %.2e (< %.0e)" % (k, r, t))
            ok &= r < t
    if cls is E.EmbedLaunch:                                      # ``assert float(dw[0].abs().max()) == 0.0``
        z = not G["dword"][E.PAD_ID].any()
        figs.append("dword[pad] %s" % ("zero" if z else "NOT zero"))
        ok &= z
    return bool(ok), ", ".join(figs)


def test_what_the_old_tests_let_pass():
    blind = []
    for fault in FAULTS:
        passes, line = old_test_reading(fault)
        print("%-45s %s -> %s" % (fault, line, "PASSES the old test" if passes else "caught by the old test"))
        if passes:
            blind.append(fault)
    assert tuple(blind) == E.NORM_BLIND, blind
