"""The kernels of csrc/rewarder.hip one by one against oracle/semireward_ref.py run in float64 on the CPU: rewarder forward (one- and two-launch
form, dense and strided, with every tensor that save_for_bwd leaves in the workspace), the running max_reward, the hand-written backward (every
gradient tensor whole), generator, sr_target and the flat Adam.  Cases, seeded inputs and references: tests/_rewarder_cases.py; what those
inputs exercise is asserted without a GPU by tests/test_cpu_rewarder_cases.py.  Needs a MI355X.

Bounds.  None is chosen and none comes from a kernel's output.  For every compared quantity the float32 oracle (the same torch restatement run
in float32, one thread) is compared with the float64 one over all cases of the test; "floor" is the worst deviation, to three digits, and the
kernel's bound is 8 x floor (a different, still float32, summation order over K <= 1024), at least 1e-7.  tests/test_cpu_rewarder_cases.py
measures the floors afresh and holds this table and _rewarder_cases.FLOORS to them within 1 %, from both sides.

    quantity        floor      bound      measure
    fwd/reward      4.87e-07   3.90e-06   absolute   (ordinary forward cases)
    fwd/z           6.55e-07   5.24e-06   largest element error / largest magnitude of the tensor
    fwd/alpha       1.28e-06   1.02e-05   "
    fwd/ctx         9.20e-07   7.36e-06   "
    fwd/xhat        6.24e-07   4.99e-06   "
    fwd/rstd        1.97e-07   1.58e-06   "
    fwd/u           4.43e-07   3.54e-06   "
    fwd/m1          5.63e-07   4.50e-06   "
    fwd/m2          5.00e-07   4.00e-06   "
    fwd/f1          5.78e-07   4.62e-06   "
    sat/reward      3.81e-07   3.05e-06   absolute   (saturated forward cases)
    sat/z           4.10e-07   3.28e-06   largest element error / largest magnitude of the tensor
    sat/alpha       4.21e-24   1.00e-07   "   (one-hot in float64 and float32 alike: the 1e-7 minimum)
    sat/ctx         5.54e-07   4.43e-06   "
    sat/xhat        3.90e-07   3.12e-06   "
    sat/rstd        1.21e-07   9.68e-07   "
    sat/u           4.04e-07   3.23e-06   "
    sat/m1          6.09e-07   4.87e-06   "
    sat/m2          3.61e-07   2.89e-06   "
    sat/f1          3.51e-07   2.81e-06   "
    max_reward      1.74e-08   1.39e-07   absolute, float32 mean of the rewards against the float64 mean (B = 1, 5, 8)
    bwd/reward      3.24e-07   2.59e-06   absolute
    bwd/loss        7.20e-07   5.76e-06   relative, the worse of the two losses
    bwd/grad_l2     1.92e-06   1.54e-05   relative L2, the worst gradient tensor
    bwd/grad_max    1.76e-06   1.41e-05   largest element error / largest magnitude, the worst gradient tensor
    gen/out         1.53e-06   1.22e-05   absolute
    adam_p          5.04e-07   4.03e-06   |error| / max(|p|, lr), element by element
    adam_m          1.14e-07   9.12e-07   relative, element by element
    adam_v          1.69e-07   1.35e-06   relative, element by element
    adam_p_double   4.82e-07   3.86e-06   as adam_p, both oracles with the hyper-parameters as doubles

Adam's hyper-parameters reach the kernel as float32 (C ABI), so the float64 reference gets those float32 values like every other input
(_rewarder_cases.ADAM_HP).  Against beta2 = 0.999 held as a double, v of any float32-beta Adam deviates by 1.3e-5 relative (rounding of beta2
times 1 / (1 - beta2)); the deviation cancels against the bias correction in the step, so p is held against the reference with double
hyper-parameters as well (adam_p_double): a beta or lr rounded wrongly on the way in would show there.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _rewarder_cases as RC                # noqa: E402
from oracle import semireward_ref as S      # noqa: E402
from semireward_amd import ops              # noqa: E402

DEV = "cuda:0"
E = 128
IDS = lambda cs: [c["id"] for c in cs]  # noqa: E731


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def flat(p, keys):
    return dev(np.concatenate([np.ascontiguousarray(p[k]).ravel() for k in keys]))


def unflat(t, shapes):
    a, out, o = t.cpu().numpy(), {}, 0
    for k, s in shapes.items():
        n = int(np.prod(s))
        out[k] = a[o:o + n].reshape(s)
        o += n
    assert o == a.size
    return out


def ws_layout(B):
    """RewWs of csrc/rewarder.hip for one group of B rows, restated: name -> (offset, shape), in floats."""
    parts = (("z", (2 * B, E)), ("slog", (2 * B,)), ("alpha", (2 * B,)), ("ctx", (E,)), ("xhat", (2 * B, E)), ("rstd", (2 * B,)),
             ("u", (B, E)), ("m1", (B, 256)), ("m2", (B, E)), ("f1", (B, 64)), ("r", (B,)),
             ("dlogit", (B,)), ("df1", (B, 64)), ("dm2", (B, E)), ("dm1", (B, 256)), ("du", (B, E)), ("dz", (2 * B, E)))
    lay, o = {}, 0
    for k, s in parts:
        lay[k] = (o, s)
        o += int(np.prod(s))
    assert o == ops.rewarder_ws_floats(1, B)
    return lay


def ws_read(ws, B, names):
    a, lay = ws.cpu().numpy(), ws_layout(B)
    return {k: a[lay[k][0]:lay[k][0] + int(np.prod(lay[k][1]))].reshape(lay[k][1]) for k in names}


class Rewarder:
    """The device side of a rewarder case: flat parameters, their transposed block, inputs."""

    def __init__(self, c):
        self.c, self.inp = c, RC.rewarder_inputs(c)
        self.F, self.B, self.G, self.L = c["F"], c["B"], c["G"], S.label_dim(c["C"])
        self.shapes = S.rewarder_shapes(self.F, c["C"])
        self.p = flat(self.inp["params"], S.REWARDER_KEYS)
        assert self.p.numel() == ops.rewarder_param_count(self.F, self.L)
        self.pt = torch.empty(ops.rewarder_t_floats(self.F), device=DEV)
        ops.rewarder_prepare(self.p, self.pt, self.F, self.L)
        self.feats, self.labels = dev(self.inp["feats"]), dev(self.inp["labels"])

    def fwd(self, save=False, **kw):
        r = torch.full((self.G * self.B,), -5.0, device=DEV)
        ws = torch.full((ops.rewarder_ws_floats(self.G, self.B),), 7.0, device=DEV)
        ops.rewarder_fwd(self.p, self.pt, kw.pop("feats", self.feats), self.labels, r, ws, self.G, self.B, self.F, self.L, save_for_bwd=save, **kw)
        return r, ws


def check(errors, prefix=""):
    """Print every figure, then hold each against its committed bound."""
    for k, v in errors.items():
        print("    %-14s %.3e   (bound %.1e)" % (prefix + k, v, RC.BOUNDS[prefix + k]))
    bad = {k: v for k, v in errors.items() if not v <= RC.BOUNDS[prefix + k]}          # (not <=: NaN fails)
    assert not bad, bad


# ---- 1. forward, dense -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RC.FORWARD, ids=IDS(RC.FORWARD))
def test_forward_dense(c):
    k = Rewarder(c)
    B, G, pre = k.B, k.G, "sat/" if c["sat"] else "fwd/"
    ref = RC.forward_ref(c, k.inp)
    r, _ = k.fwd()
    r_np = r.cpu().numpy()
    assert np.isfinite(r_np).all()
    for g in range(G):
        print("  %s group %d" % (c["id"], g))
        check(RC.forward_errors(dict(reward=r_np[g * B:(g + 1) * B]), ref[g]), pre)
    r2, _ = k.fwd()
    assert torch.equal(r, r2)                            # fixed reduction order: the same call gives the same bits
    if G == 1:
        rs, ws = k.fwd(save=True)
        assert torch.equal(rs, r)                        # saving changes nothing
        got = ws_read(ws, B, RC.SAVED + ("r",))
        assert all(np.isfinite(v).all() for v in got.values())
        assert np.array_equal(got.pop("r"), r_np)
        check(RC.forward_errors(got, ref[0]), pre)
        assert abs(float(got["alpha"].astype(np.float64).sum()) - 1.0) <= 2 * B * RC.BOUNDS[pre + "alpha"]


# ---- 2. forward, strided; max_reward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["F128_C10_B5_G3", "F384_C100_B13_G4"])
def test_forward_strided_is_the_dense_call(cid):
    """Groups read in place from a [passes, batch, F] table (group g = rows first + g * group_rows .. + B) with filler around them."""
    k = Rewarder(RC.by_id(RC.FORWARD, cid))
    B, G, F = k.B, k.G, k.F
    r, _ = k.fwd()
    Bt, first = B + 6, 3
    table = torch.full((G + 2, Bt, F), 99.0, device=DEV)
    for g in range(G):
        table[g + 1, first:first + B] = k.feats[g * B:(g + 1) * B]
    rs, _ = k.fwd(feats=table, feats_first_row=Bt + first, group_rows=Bt)
    assert torch.equal(rs, r)


@pytest.mark.parametrize("start", [float("-inf"), 2.0])
@pytest.mark.parametrize("cid", ["F128_C10_B1_G1", "F33_C10_B5_G1", "F128_C10_B8_G1"])
def test_max_reward(cid, start):
    c = RC.by_id(RC.FORWARD, cid)
    k = Rewarder(c)
    mr = torch.full((), start, device=DEV)
    r, _ = k.fwd(max_reward=mr)
    r0, _ = k.fwd()
    assert torch.equal(r, r0)
    s = np.float32(0.0)
    for v in r.cpu().numpy():                            # the kernel's own rewards, summed in index order in float32
        s = np.float32(s + v)
    mean = np.float32(s / np.float32(k.B))
    assert float(mr) == max(start, float(mean))
    check(dict(max_reward=abs(float(mean) - float(RC.forward_ref(c, k.inp)[0]["reward"].mean()))))


@pytest.mark.parametrize("cid", ["F128_C10_B5_G3", "F1_C2_B9_G1"])
def test_max_reward_refuses_what_is_not_one_tile(cid):
    k = Rewarder(RC.by_id(RC.FORWARD, cid))              # G = 3; B = 9
    assert k.G > 1 or k.B > 8
    mr = torch.full((), 0.25, device=DEV)
    with pytest.raises(RuntimeError, match="invalid argument"):
        k.fwd(max_reward=mr)
    if k.G > 1:                                          # G = 2, B = 5: a call of its own, buffers sized for it
        G, B = 2, k.B
        r, ws = torch.empty(G * B, device=DEV), torch.empty(ops.rewarder_ws_floats(G, B), device=DEV)
        feats, labels = k.feats[:G * B].contiguous(), k.labels[:G * B].contiguous()
        ops.rewarder_fwd(k.p, k.pt, feats, labels, r, ws, G, B, k.F, k.L)                  # fine without max_reward
        with pytest.raises(RuntimeError, match="invalid argument"):
            ops.rewarder_fwd(k.p, k.pt, feats, labels, r, ws, G, B, k.F, k.L, max_reward=mr)
    assert float(mr) == 0.25


# ---- 3. backward -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RC.BACKWARD, ids=IDS(RC.BACKWARD))
def test_backward(c):
    k = Rewarder(c)
    B = k.B
    ref = RC.backward_ref(c, k.inp)
    r, ws = k.fwd(save=True)
    grads = torch.full_like(k.p, 7.0)                    # must be overwritten everywhere
    losses = torch.full((2,), 7.0, device=DEV)
    ops.rewarder_bwd(k.p, k.feats, k.labels, dev(k.inp["target"]), ws, grads, losses, B, k.F, k.L)
    ops.check_label_errors()
    g = unflat(grads, k.shapes)
    assert all(np.isfinite(v).all() for v in g.values())
    print("  %s" % c["id"])
    check(RC.backward_errors(r.cpu().numpy(), g, float(losses[0]), float(losses[1]), ref), "bwd/")
    assert float(np.abs(g["cross_attention_fc.bias"]).max()) == 0.0          # cancels in the softmax over the batch
    absent = np.setdiff1d(np.arange(k.L), k.inp["labels"])
    assert absent.size > 0 and float(np.abs(g["label_embedding.weight"][absent]).max()) == 0.0
    present = np.unique(k.inp["labels"])
    assert (np.abs(g["label_embedding.weight"][present]).max(axis=1) > 0.0).all()
    if c["same_labels"]:                                 # B rows added into ONE embedding row
        assert present.size == 1 and B > 1


# ---- 4. generator, 5. sr_target ----------------------------------------------------------------------------------------------------------
def run_generator(c):
    inp = RC.generator_inputs(c)
    F, B = c["F"], c["B"]
    p = flat(inp["params"], S.GENERATOR_KEYS)
    assert p.numel() == ops.generator_param_count(F)
    pt = torch.empty(ops.generator_t_floats(F), device=DEV)
    ops.generator_prepare(p, pt, F)
    out, lab = torch.full((B + 5,), -3.0, device=DEV), torch.full((B + 5,), -77, dtype=torch.int64, device=DEV)
    ops.generator_fwd(p, pt, dev(inp["x"]), out, lab, B, F)
    return inp, out, lab


@pytest.mark.parametrize("c", RC.GENERATOR, ids=IDS(RC.GENERATOR))
def test_generator(c):
    inp, out, lab = run_generator(c)
    B = c["B"]
    ref, _ = RC.generator_ref(c, inp)
    print("  %s" % c["id"])
    check({"gen/out": RC.max_abs(out[:B].cpu().numpy(), ref)})
    assert np.array_equal(lab[:B].cpu().numpy(), np.floor(ref).astype(np.int64))          # every row: no output is within 1e-3 of an integer
    assert np.array_equal(out[:B].cpu().numpy() == 0.0, ref == 0.0)                     # the clamped rows are exactly 0
    assert bool((out[B:] == -3.0).all()) and bool((lab[B:] == -77).all())                  # nothing past B is written
    ops.check_label_errors()


@pytest.mark.parametrize("c", RC.GENERATOR, ids=IDS(RC.GENERATOR))
def test_sr_target(c):
    """1.0 where the generated label is the reference label, else 0.5 -- exact; in-range labels leave the error flag clear."""
    inp, _, lab = run_generator(c)
    B = c["B"]
    gen = lab[:B].contiguous()
    gen_np = gen.cpu().numpy()
    C = int(gen_np.max()) + 4
    for shift in (0, 1, 2):
        ref_np = gen_np.copy()
        ref_np[shift::3] += 1 + shift                    # every third row disagrees, starting at row `shift`
        tgt = torch.full((B + 3,), 7.0, device=DEV)
        ops.sr_target(gen, dev(ref_np), tgt, B, C)
        assert np.array_equal(tgt[:B].cpu().numpy(), np.where(gen_np == ref_np, 1.0, 0.5).astype(np.float32))
        assert np.array_equal(tgt[:B].cpu().numpy(), S.cosine_target(torch.from_numpy(gen_np), torch.from_numpy(ref_np), C).numpy()[:, 0])
        assert bool((tgt[B:] == 7.0).all())
    ops.check_label_errors()


# ---- 6. Adam -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", RC.ADAM_RUNS, ids=IDS(RC.ADAM_RUNS))
def test_adam_flat(run):
    n = run["n"] or ops.rewarder_param_count(33, 100)
    assert n == (run["n"] or RC.ADAM_N) and (n == 1 or n % 256 != 0)
    host = RC.adam_inputs(n, run["seed"], run["zero_moments"])
    for steps in range(1, run["steps"] + 1):
        p, g, m, v = (dev(a) for a in host)
        p2, m2, v2 = p.clone(), m.clone(), v.clone()
        for s in range(steps):
            step = run["step0"] + s
            ops.adam_flat(p, g, m, v, n, RC.LR, step)
            block = torch.tensor(ops.adam_bias_corrections(0.9, 0.999, step), dtype=torch.float32, device=DEV)
            ops.adam_flat(p2, g, m2, v2, n, RC.LR, 0, dyn=block.data_ptr())
            torch.cuda.synchronize()                     # (block stays alive until its launch has run)
        assert torch.equal(p2, p) and torch.equal(m2, m) and torch.equal(v2, v)          # the dyn form is the by-value launch, bit for bit
        print("  %s, %d step(s)" % (run["id"], steps))
        got = [t.cpu().numpy() for t in (p, m, v)]
        check(RC.adam_errors(got, RC.adam_ref(*host, run["step0"], steps)))
        check(dict(adam_p_double=RC.adam_errors(got, RC.adam_ref(*host, run["step0"], steps, hp=RC.ADAM_HP_DOUBLE))["adam_p"]))
    assert n == 1 or (float(g.abs().min()) < 1e-7 and float(g.abs().max()) > 10.0)          # the gradients span 1e-8 .. 1e2
