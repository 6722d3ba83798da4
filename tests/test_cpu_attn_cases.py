"""What tests/_attn_cases.py rests on, checked without a GPU: the committed fp32 constants are 8 x their measurement; the float32 restatement
of every case lies inside the bound; the backward formula equals float64 autograd; every key carries DECISIVE of some row and the spikes stand
>= 40 above their rows; every case reaches the plan it names; no dropout mask is trivial on a tile; verify() rejects each planted fault; and
which of those faults the whole-tensor thresholds of the norm tests let pass."""
import numpy as np
import pytest
import torch

import _attn_cases as A
from semireward_amd import ops

IDS = [c["id"] for c in A.CASES]


def test_committed_constants_are_eight_times_their_measurement():
    cf, cb = A.measure_constants()
    print("measured C_F32 %.3f C_BWD %.3f (committed %.3f %.3f)" % (cf, cb, A.C_F32_MEASURED, A.C_BWD_MEASURED))
    assert A.C_F32 == 8.0 * A.C_F32_MEASURED and A.C_BWD == 8.0 * A.C_BWD_MEASURED
    assert 4.0 * cf <= A.C_F32 <= 16.0 * cf, (cf, A.C_F32)
    assert 4.0 * cb <= A.C_BWD <= 16.0 * cb, (cb, A.C_BWD)


@pytest.mark.parametrize("cid", IDS)
def test_case_inputs_plan_and_restatement(cid):
    """Per case: the plan it names; the decisive-key and spike conditions on its inputs, every head; the float32 restatement with the kernels'
    rounding points, both accumulation orders, inside the bound on the sampled heads."""
    c = A.BY_ID[cid]
    assert ops.attn_plan(c["B"], c["N"], c["H"]) == c["plan"], cid
    inp = A.make_inputs(c)
    if c["key_len"] is not None:
        assert inp["klen"][0] == c["N"] and all(1 <= x <= c["N"] for x in inp["klen"])          # the key_len contract of srhip_attn_masked_fwd
    least, margin = A.decisive_mass(c, inp)
    assert least >= A.DECISIVE, (cid, least)
    assert margin >= 40.0, (cid, margin)
    for b in range(c["B"]):                                   # pi is a permutation of the valid keys: every key is some row's decisive key
        for h in range(c["H"]):
            assert sorted(set(inp["pi"][b, h])) == list(range(int(inp["klen"][b])))
    keep, _ = A.keep_of(c)
    heads = A.sample_heads(c)
    sub = dict(c, B=1, H=1)
    for b, h in heads:
        one = {n: inp[n][b:b + 1, h:h + 1] for n in ("q", "k", "v", "do")}
        one["klen"] = inp["klen"][b:b + 1]
        kp = None if keep is None else keep[b:b + 1, h:h + 1]
        fwd = A.reference_fwd(sub, one, kp)
        bwd = A.reference_bwd(sub, one, kp, fwd)
        for rev in (False, True):
            r = A.restate_case(sub, one, kp, fwd, reverse=rev)
            A.verify_fwd("restatement", r["out"], r["lse"], fwd)
            A.verify_bwd("restatement", r, bwd)


@pytest.mark.parametrize("cid", [c["id"] for c in A.CASES if "readout" in c["forms"]])
def test_readout_restatement(cid):
    """The probability read-out on the float32 restatement, every window, sampled heads: each element of the matrix inside its own bound (the
    paired forward rounds against the running maximum: the bound's rounding term sits there), dropped and masked entries exactly zero."""
    c = A.BY_ID[cid]
    inp = A.make_inputs(c)
    keep, _ = A.keep_of(c)
    sub = dict(c, B=1, H=1)
    for b, h in A.sample_heads(c, 3):
        one = {n: inp[n][b:b + 1, h:h + 1] for n in ("q", "k", "v", "do")}
        one["klen"] = inp["klen"][b:b + 1]
        kp = keep[b:b + 1, h:h + 1]
        fwd = A.reference_fwd(sub, one, kp)
        R = A.readout_reference(sub, one, kp, fwd)
        L = int(one["klen"][0])
        for j in range((c["N"] + 63) // 64):
            o, _ = A.restate_fwd(one["q"][0, 0], one["k"][0, 0], A.readout_v(sub, one, j)[0, 0], L, kp[0, 0], c["p"],
                                 block=128 if c["plan"].fwd_pair else None)
            A.verify("restatement", "P(out)", o[None, None], A.readout_window(R["fwd"], j), A.readout_window(R["fwd_tol"], j))
            g = A.restate_bwd(one["q"][0, 0], one["k"][0, 0], one["v"][0, 0], A.readout_do(sub, one, j)[0, 0], fwd["out_given"][0, 0],
                              fwd["lse_given"][0, 0], L, kp[0, 0], c["p"])
            A.verify("restatement", "P(dv)", g["dv"][None, None], A.readout_window(R["bwd"], j, True), A.readout_window(R["bwd_tol"], j, True))
            assert np.array_equal(o[None, None] == 0, A.readout_window(R["fwd"], j) == 0)
            assert np.array_equal(g["dv"][None, None] == 0, A.readout_window(R["bwd"], j, True) == 0)


@pytest.mark.parametrize("cid", [c["id"] for c in A.BLOCK_CASES])
def test_fused_block_restatement_inside_bound(cid):
    """The fused block's rounding points restated in float32 (projections rounded to bf16, softmax in chunks of 64 keys) inside the bound of
    the block reference, every element; a wrong extra query (row 256 computed from token 240's q) is rejected and named."""
    c = A.BLOCK_BY_ID[cid]
    inp = A.make_block_inputs(c)
    ref = A.block_reference(c, inp)
    got = A.restate_block(c, inp)
    A.verify_block("restatement", c, got, ref["out"], ref["tol"])
    if c["N"] == 257:
        got[256, 64:128] = got[240, 64:128]
        with pytest.raises(AssertionError) as e:
            A.verify_block("restatement", c, got, ref["out"], ref["tol"])
        assert "the extra query" in str(e.value) and "head 1" in str(e.value)


@pytest.mark.parametrize("cid", ["block-N257B1", "block-N197B3"])
def test_out_scale_is_held_against_the_unscaled_result(cid):
    """verify_out_scale on the restatement: the scaled result (scale before the one rounding) passes; a scale off by 1 % and a scale applied
    after the rounding are rejected -- both lie inside the float64 bound of the block, which is why out_scale is not held to that one."""
    c = A.BLOCK_BY_ID[cid]
    inp = A.make_block_inputs(c)
    s = float(np.float32(1.0 / 0.85))
    out = A.restate_block(c, inp)
    outs = A.restate_block(c, inp, out_scale=[s] * c["B"])
    r, frac = A.verify_out_scale("restatement", c, outs, out, s)
    print("headroom %.3f, %.3f of the elements differ from bf16(s * out)" % (r, frac))
    assert frac >= 1.0 / 0.85 / 8.0                                         # the figure ONCE_ROUNDED_MIN is a third of
    off = A.restate_block(c, inp, out_scale=[1.01 * s] * c["B"])
    twice = A.bf16(s * out)
    ref = A.block_reference(c, inp, out_scale=[s] * c["B"])
    for bad in (off, twice):
        A.verify_block("restatement", c, bad, ref["out"], ref["tol"])       # the float64 bound lets both pass
        with pytest.raises(AssertionError):
            A.verify_out_scale("restatement", c, bad, out, s)
    with pytest.raises(AssertionError) as e:
        A.verify_out_scale("restatement", c, twice, out, s)
    assert "after the bf16 rounding" in str(e.value)


def test_backward_formula_equals_float64_autograd():
    """head_bwd on unrounded out and lse against torch autograd of the float64 forward, key mask and dropout on: 1e-12 relative."""
    c = A.BY_ID["drop-B6N64H1-kl-p0.5-s2"]
    inp = A.make_inputs(c)
    keep, _ = A.keep_of(c)
    for b in range(c["B"]):
        L = int(inp["klen"][b])
        q, k, v = (torch.from_numpy(inp[n][b, 0]).requires_grad_(True) for n in ("q", "k", "v"))
        neg = torch.where(torch.arange(c["N"]) < L, 0.0, float("-inf")).double()
        P = torch.softmax(A.SCALE * (q @ k.T) + neg, -1) * torch.from_numpy(keep[b, 0] / (1.0 - c["p"]))
        out = P @ v
        out.backward(torch.from_numpy(inp["do"][b, 0]))
        f = A.head_fwd(inp["q"][b, 0], inp["k"][b, 0], inp["v"][b, 0], L, keep[b, 0], c["p"])
        assert np.abs(f["out"] - out.detach().numpy()).max() <= 1e-12 * np.abs(f["out"]).max()
        w = A.head_bwd(inp["q"][b, 0], inp["k"][b, 0], inp["v"][b, 0], inp["do"][b, 0], f["out"], f["lse"], L, keep[b, 0], c["p"])
        for n, t in (("dq", q), ("dk", k), ("dv", v)):
            g = t.grad.numpy()
            assert np.abs(w[n] - g).max() <= 1e-12 * np.abs(g).max(), (b, n)
            if n != "dq":
                assert not g[L:].any() and not w[n][L:].any()


@pytest.mark.parametrize("cid", [c["id"] for c in A.CASES if c["p"]])
def test_no_dropout_mask_is_trivial_on_a_tile(cid):
    """Every whole 16 x 16 tile of every head's keep mask holds both a kept and a dropped element (ragged edge tiles of one row or column can
    be all-kept at p = 0.1 and are not counted); both rates and both seeds are in use."""
    c = A.BY_ID[cid]
    keep, _ = A.keep_of(c)
    n = c["N"] // 16 * 16
    if n:
        t = keep[:, :, :n, :n].reshape(c["B"], c["H"], n // 16, 16, n // 16, 16).sum((3, 5))
        assert t.min() > 0 and t.max() < 256, (cid, t.min(), t.max())
    assert abs(keep.mean() - (1 - c["p"])) < 0.02
    assert {(x["p"], x["dseed"] >> 32) for x in A.CASES if x["p"]} >= {(0.1, 77), (0.5, 77)}
    assert len({x["dseed"] for x in A.CASES if x["p"] and x["N"] == c["N"]}) >= 2


# ---- planted faults --------------------------------------------------------------------------------------------------------------------------
class Ctx:
    """A case with its inputs, references and the clean restatement of every head."""

    def __init__(self, c, gaussian=None):
        self.c, self.inp = c, A.make_inputs(c, gaussian=gaussian)
        self.keep, _ = A.keep_of(c)
        self.fwd = A.reference_fwd(c, self.inp, self.keep)
        self.bwd = A.reference_bwd(c, self.inp, self.keep, self.fwd)
        self.block = 128 if c["plan"].fwd_pair else None

    def clean(self):
        return A.restate_case(self.c, self.inp, self.keep, self.fwd)

    def head(self, b, h):
        i = self.inp
        return dict(q=i["q"][b, h], k=i["k"][b, h], v=i["v"][b, h], do=i["do"][b, h], L=int(i["klen"][b]),
                    keep=None if self.keep is None else self.keep[b, h], og=self.fwd["out_given"][b, h], lg=self.fwd["lse_given"][b, h])

    def rfwd(self, b, h, L=None, keep="same", **kw):
        a = self.head(b, h)
        o, l = A.restate_fwd(a["q"], a["k"], a["v"], a["L"] if L is None else L, a["keep"] if isinstance(keep, str) else keep, self.c["p"],
                             block=self.block, **kw)
        return dict(out=o, lse=l)

    def rbwd(self, b, h, **kw):
        a = self.head(b, h)
        return A.restate_bwd(a["q"], a["k"], a["v"], a["do"], a["og"], a["lg"], a["L"], a["keep"], self.c["p"], **kw)


def _short(x):
    """A sequence of the case whose key length is inside the sequence (the last such one)."""
    return max(b for b in range(x.c["B"]) if 17 < x.inp["klen"][b] < x.c["N"] - 1)


def f_drop_key(x, init):
    P = A.head_probs(x.inp["q"][0, 0], x.inp["k"][0, 0], int(x.inp["klen"][0]), None, 0.0)["P"]
    return (0, 0), x.rfwd(0, 0, fault=("drop_key", 37, int(P[37].argmax())))


def f_swap_v(x, init):
    return (0, 0), x.rfwd(0, 0, fault=("swap_v", 3, 100))


def f_mask_plus(x, init):
    b = _short(x)
    return (b, 0), x.rfwd(b, 0, L=int(x.inp["klen"][b]) + 1)


def f_mask_minus(x, init):
    b = _short(x)
    return (b, 0), x.rfwd(b, 0, L=int(x.inp["klen"][b]) - 1)


def f_drop_parity(x, init):
    kp = x.keep[0, 0].copy()
    kp[36] = x.keep[0, 0][37]                      # the pairs of row 36 decided with the pair indices of the odd row beside it
    return (0, 0), x.rfwd(0, 0, keep=kp)


def f_sum_after_rounding(x, init):
    return (0, 0), x.rfwd(0, 0, fault=("sum_after_rounding",))


def f_block_max_lse(x, init):
    return (0, 0), x.rfwd(0, 0, fault=("block_max_lse",))


def f_last_row_from_previous_tile(x, init):
    r = x.rfwd(0, 0)
    n = x.c["N"] - 1
    r["out"][n], r["lse"][n] = r["out"][n - 16], r["lse"][n - 16]
    return (0, 0), r


def f_ragged_row_zero(x, init):
    r = x.rfwd(0, 0)
    r["out"][x.c["N"] - 1] = 0.0
    return (0, 0), dict(out=r["out"])


def f_padded_dv_unwritten(x, init):
    b = _short(x)
    r = x.rbwd(b, 0)
    r["dv"][int(x.inp["klen"][b]):] = init
    return (b, 0), dict(dv=r["dv"])


def f_delta_wrong_head(x, init):
    other = x.rbwd(x.c["B"] - 1, x.c["H"] - 1)["delta"]
    r = x.rbwd(0, 0, fault=("delta", other))
    return (0, 0), r


def f_dq_no_scale(x, init):
    return (0, 0), dict(dq=x.rbwd(0, 0, fault=("no_scale",))["dq"])


def f_split_slice_not_stored(x, init):
    r = x.rbwd(0, 0)
    r["dq"][128:256] = init                       # blockIdx.y = 1 of a split of three: query tiles 8 .. 15
    return (0, 0), dict(dq=r["dq"])


# fault: (function, the case verify() is shown it on, the shape and inputs of the norm test it is measured at)
MASKED, PAIRED = "drop-B9N257H1-kl-p0.1-s2", "nkt32-B1N384H2"
FAULTS = {
    "one key dropped from one query's softmax": (f_drop_key, MASKED, "plain"),
    "two V rows swapped": (f_swap_v, MASKED, "plain"),
    "mask one key too long at key_len": (f_mask_plus, MASKED, "masked"),
    "mask one key too short at key_len": (f_mask_minus, MASKED, "masked"),
    "dropout pairs of a row decided with the pair index of the other row parity": (f_drop_parity, MASKED, "masked"),
    "row sum taken after the bf16 rounding": (f_sum_after_rounding, MASKED, "plain"),
    "lse built from the last block's maximum": (f_block_max_lse, PAIRED, "paired"),
    "row 256 of a head computed from the previous tile's rows": (f_last_row_from_previous_tile, MASKED, "plain"),
    "ragged-tile row stored as zeros": (f_ragged_row_zero, MASKED, "plain"),
    "dV of padded keys left unwritten": (f_padded_dv_unwritten, MASKED, "masked"),
    "delta taken from another head": (f_delta_wrong_head, MASKED, "plain"),
    "dQ missing scale": (f_dq_no_scale, MASKED, "plain"),
    "one bwd_split slice of dQ not stored": (f_split_slice_not_stored, MASKED, "plain"),
}


@pytest.fixture(scope="module")
def contexts():
    return {cid: Ctx(A.BY_ID[cid]) for cid in (MASKED, PAIRED)}


def _head_ref(x, b, h):
    r = {n: x.fwd[n][b, h] for n in A.FWD_KEYS}
    r.update({n: x.bwd[n][b, h] for n in A.BWD_KEYS})
    return r


def _verify_head(x, b, h, got):
    ref = _head_ref(x, b, h)
    for n, g in got.items():
        A.verify("restatement", "delta_ws" if n == "delta" else n, g, ref[n], ref[n + "_tol"], rounded=n not in ("lse", "delta"))


@pytest.mark.parametrize("name", list(FAULTS))
def test_verify_rejects_planted_fault(name, contexts):
    fn, cid, _ = FAULTS[name]
    x = contexts[cid]
    (b, h), got = fn(x, np.nan)
    clean = dict(x.rfwd(b, h), **x.rbwd(b, h))
    _verify_head(x, b, h, clean)                                            # the same head without the fault is inside the bound
    with pytest.raises(AssertionError) as e:
        _verify_head(x, b, h, got)
    assert "restatement" in str(e.value) and "tile" in str(e.value)


def _norm_case(kind):
    """The shapes and inputs of the norm tests: test_attention_fwd_bwd (4, 257, 6) and (2, 320, 2) on N(0, 1.5^2), and
    test_attention_masked_dropout_fwd_bwd (5, 257, 2, p = 0.1) on N(0, 1.2^2) with its key lengths."""
    if kind == "plain":
        return A._case("norm", 4, 257, 6, plan=ops.attn_plan(4, 257, 6)), 1.5
    if kind == "paired":
        return A._case("norm", 2, 320, 2, plan=ops.attn_plan(2, 320, 2)), 1.5
    c = A._case("norm", 5, 257, 2, p=0.1, dseed=9, plan=ops.attn_plan(5, 257, 2))
    kl = np.random.Generator(np.random.PCG64(257)).integers(257 // 3, 258, size=5)
    kl[0] = 257
    return dict(c, key_len=tuple(int(v) for v in kl)), 1.2


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_what_the_norm_thresholds_let_pass():
    """Each planted fault in one head of a clean float32 restatement, measured as the norm tests measure (rel-L2 of out < 6e-3, of dq / dk / dv
    < 1.5e-2, max |lse| difference < 2e-3 where the test reads lse -- the masked one does not --, dqkv starting from zeros) at those tests' shapes and Gaussian inputs.  The faults those thresholds
    let pass are NORM_BLIND of _attn_cases.py; every one of them is rejected by verify() above."""
    ctx, blind, lines = {}, [], []
    for name, (fn, _, kind) in FAULTS.items():
        if kind not in ctx:
            c, s = _norm_case(kind)
            x = Ctx(c, gaussian=s)
            ctx[kind] = (x, x.clean())
        x, base = ctx[kind]
        (b, h), got = fn(x, 0.0)
        r = {n: base[n].copy() for n in base}
        for n, g in got.items():
            r[n][b, h] = g
        fig = {"out": _rel(r["out"], x.fwd["out"]), "lse": float(np.abs(r["lse"] - x.fwd["lse"]).max())}
        fig.update({n: _rel(r[n], x.bwd[n]) for n in ("dq", "dk", "dv")})
        clean = {"out": _rel(base["out"], x.fwd["out"]), "dq": _rel(base["dq"], x.bwd["dq"])}
        assert clean["out"] < 6e-3 and clean["dq"] < 1.5e-2
        passes = fig["out"] < 6e-3 and (fig["lse"] < 2e-3 or kind == "masked") and all(fig[n] < 1.5e-2 for n in ("dq", "dk", "dv"))
        lines.append("%-75s out %.2e lse %.2e dq %.2e dk %.2e dv %.2e -> %s" % (name, fig["out"], fig["lse"], fig["dq"], fig["dk"], fig["dv"],
                                                                                   "PASSES the norm tests" if passes else "caught"))
        if passes:
            blind.append(name)
    print("\n".join(lines))
    assert blind, "the norm thresholds caught every planted fault"
    assert tuple(blind) == A.NORM_BLIND, blind
