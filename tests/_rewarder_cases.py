"""The cases of tests/test_{cpu,gpu}_rewarder*.py and their seeded inputs: the rewarder / generator / Adam kernels of csrc/rewarder.hip one by one
against oracle/semireward_ref.py in float64.  Nothing is stored: every input is rebuilt from its seed, every expected value is recomputed.

Why the parameters are not ``synth.synth_params`` as they come: with those the attention logits over the 2B rows have a standard deviation of
about 0.5, so the context vector is almost the plain mean of the rows and the rewards of a case sit in a band 0.04 wide -- a softmax that mixes
up rows or drops one moves nothing a test could see.  A case therefore scales ``cross_attention_fc.weight`` by ``att`` and the four head
weights by ``head``; tests/test_cpu_rewarder_cases.py asserts what that buys (logit spread, alpha peak, reward span) on the float64 reference,
so that the seeds and gains below cannot rot.  'sat' cases push the logit spread past 40: exp() of anything but the max-subtracted logit would
overflow.  Generator cases scale the last layer so that the labels differ, one row is clamped to 0 and no output sits near an integer.

Backward cases also keep every ReLU input of the case at least KINK_FACTOR times the float32 oracle's own deviation away from 0, so that no
element has to be left out of a gradient comparison (seeds searched on the CPU, committed here)."""
import numpy as np
import torch

from oracle import semireward_ref as S
from semireward_amd.utils import synth

HEAD_WEIGHTS = ("mlp_fc1.weight", "mlp_fc2.weight", "ffn_fc1.weight", "ffn_fc2.weight")
KINK_FACTOR = 100.0
LR = 5e-4
# Adam's hyper-parameters as the kernel receives them: the C ABI takes them as float32, so -- like every other input -- the float64 reference
# gets the float32 values, cast up.  (Against beta2 = 0.999 as a double the second moment of ANY float32-beta Adam is off by 1.3e-5 relative:
# the rounding of beta2, 1.3e-8, times 1 / (1 - beta2).  It cancels against the bias correction in the step itself.)
ADAM_HP = dict(lr=float(np.float32(LR)), beta1=float(np.float32(0.9)), beta2=float(np.float32(0.999)), eps=float(np.float32(1e-8)))
ADAM_HP_DOUBLE = dict(lr=LR)     # p must agree with this one too: the step itself does not depend on how beta2 was rounded on the way in
SAVED = ("z", "alpha", "ctx", "xhat", "rstd", "u", "m1", "m2", "f1")           # what save_for_bwd leaves in the workspace, besides r


def _rc(F, C, B, G=1, seed=0, att=4.0, head=2.2, sat=False, same_labels=False):
    c = dict(F=F, C=C, B=B, G=G, seed=seed, att=att, head=head, sat=sat, same_labels=same_labels)
    c["id"] = "F{F}_C{C}_B{B}_G{G}".format(**c) + ("_sat" if sat else "") + ("_same" if same_labels else "")
    return c


# (F, C, B, G): B = 1; partial tile, F no multiple of 32; one whole tile; two launches with a partial last tile, F no multiple of 32 or 64;
# whole tiles; 2B > 256 (second stride of the softmax loops) with a one-row last tile; F = 1, one row in the second tile; F = 1024, label_dim
# 1000; several groups with a partial tile in the one-launch and in the two-launch form; a saturated softmax on either path.
FORWARD = (
    _rc(128, 10, 1, seed=2), _rc(33, 10, 5, seed=1), _rc(128, 10, 8, seed=2), _rc(100, 100, 13, seed=13), _rc(384, 100, 64, seed=0),
    _rc(768, 200, 129, seed=0), _rc(1, 2, 9, seed=196, head=3.0), _rc(1024, 1000, 16, seed=1), _rc(128, 10, 5, G=3, seed=3),
    _rc(384, 100, 13, G=4, seed=138), _rc(128, 10, 8, seed=2, att=100.0, sat=True), _rc(384, 100, 13, seed=0, att=100.0, sat=True),
)
BACKWARD = (
    _rc(128, 10, 1, seed=2), _rc(33, 10, 5, seed=1), _rc(128, 10, 8, seed=12), _rc(100, 100, 13, seed=17), _rc(384, 100, 64, seed=1006),
    _rc(768, 200, 129, seed=212), _rc(384, 100, 17, seed=0, same_labels=True),
)


def _gc(F, B, seed=0, gain=40.0, shift=1.5):
    return dict(F=F, B=B, seed=seed, gain=gain, shift=shift, id="F%d_B%d" % (F, B))


GENERATOR = (_gc(128, 8, seed=10), _gc(33, 13, seed=23), _gc(768, 65, seed=1), _gc(1024, 16, seed=7), _gc(1, 3, seed=0))


def by_id(cases, cid):
    return next(c for c in cases if c["id"] == cid)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def rewarder_inputs(c):
    """numpy inputs of a rewarder case: params {name: f32}, feats f32 [G * B, F], labels i64 [G * B] (every group its own rows), target f32 [B]
    in {0.5, 1.0} with at least one of each for B > 1 (used by the backward cases, G = 1)."""
    F, C, B, G = c["F"], c["C"], c["B"], c["G"]
    p = synth.synth_params(S.rewarder_shapes(F, C), 1000 + c["seed"])
    p["cross_attention_fc.weight"] = p["cross_attention_fc.weight"] * np.float32(c["att"])
    for k in HEAD_WEIGHTS:
        p[k] = p[k] * np.float32(c["head"])
    rng = np.random.Generator(np.random.PCG64([c["seed"], F, C, B, G]))
    feats = rng.standard_normal((G * B, F)).astype(np.float32)
    labels = rng.integers(0, C, size=(G * B,), dtype=np.int64)
    if c["same_labels"]:
        labels[:] = labels[0]
    target = rng.choice(np.array([0.5, 1.0], np.float32), size=B)
    if B > 1:
        target[0], target[B - 1] = 0.5, 1.0
    return dict(params=p, feats=feats, labels=labels, target=target)


def generator_inputs(c):
    """params {name: f32} and x f32 [B, F] of a generator case."""
    F, B = c["F"], c["B"]
    p = synth.synth_params(S.generator_shapes(F), 2000 + c["seed"])
    p["fc_layers.6.weight"] = p["fc_layers.6.weight"] * np.float32(c["gain"])
    p["fc_layers.6.bias"] = p["fc_layers.6.bias"] * np.float32(c["gain"]) + np.float32(c["shift"])
    rng = np.random.Generator(np.random.PCG64([c["seed"], F, B, 7]))
    return dict(params=p, x=rng.standard_normal((B, F)).astype(np.float32))


def adam_inputs(n, seed, zero_moments):
    """p, g, m, v f32 [n]: |g| log-uniform over 1e-8 .. 1e2 (v = 1e-3 g^2 stays a normal float32; sqrt(v) crosses eps = 1e-8), random signs;
    the first half of p starts at 0, where the float32 result resolves the step itself and not only p's last bit."""
    rng = np.random.Generator(np.random.PCG64([seed, n]))
    g = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-8, 2, n)).astype(np.float32)
    p = (0.05 * rng.standard_normal(n)).astype(np.float32)
    p[:n // 2] = 0.0
    if zero_moments:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m = (0.3 * g * rng.uniform(0.5, 2.0, n)).astype(np.float32)
        v = (g.astype(np.float64) ** 2 * rng.uniform(0.5, 2.0, n)).astype(np.float32)
    return p, g, m, v


# The float32 oracle's worst deviation from float64 per compared quantity (float32_floors() below, one thread), to three digits: the table in
# the docstring of tests/test_gpu_rewarder_kernels.py.  tests/test_cpu_rewarder_cases.py measures them afresh and holds each within
# FLOOR_HEADROOM of the figure here, from both sides.  A kernel's bound is 8 x the floor, at least 1e-7.
FLOORS = {
    "fwd/reward": 4.87e-7, "fwd/z": 6.55e-7, "fwd/alpha": 1.28e-6, "fwd/ctx": 9.20e-7, "fwd/xhat": 6.24e-7, "fwd/rstd": 1.97e-7,
    "fwd/u": 4.43e-7, "fwd/m1": 5.63e-7, "fwd/m2": 5.00e-7, "fwd/f1": 5.78e-7,
    "sat/reward": 3.81e-7, "sat/z": 4.10e-7, "sat/alpha": 4.21e-24, "sat/ctx": 5.54e-7, "sat/xhat": 3.90e-7, "sat/rstd": 1.21e-7,
    "sat/u": 4.04e-7, "sat/m1": 6.09e-7, "sat/m2": 3.61e-7, "sat/f1": 3.51e-7,
    "max_reward": 1.74e-8, "bwd/reward": 3.24e-7, "bwd/loss": 7.20e-7, "bwd/grad_l2": 1.92e-6, "bwd/grad_max": 1.76e-6, "gen/out": 1.53e-6,
    "adam_p": 5.04e-7, "adam_m": 1.14e-7, "adam_v": 1.69e-7, "adam_p_double": 4.82e-7,
}
FLOOR_HEADROOM = 0.01            # rounding to three digits is 0.5 %; the rest is for a float32 sum that another CPU orders differently
BOUNDS = {k: max(8.0 * f, 1e-7) for k, f in FLOORS.items()}


class _one_thread:
    """The float32 oracle's rounding depends on how many threads split its sums: measure its deviation with one, on every machine alike."""

    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *a):
        torch.set_num_threads(self.n)


# ---- references ------------------------------------------------------------------------------------------------------------------------
def _t(a, dt):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dt) if t.is_floating_point() else t


def _tp(p, dt):
    return {k: _t(v, dt) for k, v in p.items()}


def forward_ref(c, inp, dt=torch.float64):
    """Per group: {name: float64 numpy} of S.rewarder_intermediates run in ``dt`` (float64: the reference; float32: the oracle whose deviation
    from it prices the bounds), reward and the 1-d tensors flattened."""
    B, p = c["B"], _tp(inp["params"], dt)
    out = []
    for g in range(c["G"]):
        m = S.rewarder_intermediates(p, _t(inp["feats"][g * B:(g + 1) * B], dt), _t(inp["labels"][g * B:(g + 1) * B], dt))
        m["reward"] = m["reward"].squeeze(1)
        out.append({k: v.double().numpy() for k, v in m.items()})
    return out


def backward_ref(c, inp, dt=torch.float64):
    """(reward [B], {name: gradient}, generator_loss, rewarder_loss) by autograd through S.rewarder_update_grads in ``dt``, as float64 numpy."""
    r, g, lg, lr_ = S.rewarder_update_grads(_tp(inp["params"], dt), _t(inp["feats"], dt), _t(inp["labels"], dt), _t(inp["target"], dt).view(-1, 1))
    return r.squeeze(1).double().numpy(), {k: v.double().numpy() for k, v in g.items()}, lg, lr_


def generator_ref(c, inp, dt=torch.float64):
    """(outputs [B], ReLU inputs of the last layer [B]) as float64 numpy."""
    pre = S.generator_last_preact(_tp(inp["params"], dt), _t(inp["x"], dt)).squeeze(1)
    out = S.generator_forward(_tp(inp["params"], dt), _t(inp["x"], dt)).squeeze(1)
    return out.double().numpy(), pre.double().numpy()


def adam_ref(p, g, m, v, step0, steps, dt=torch.float64, hp=ADAM_HP):
    """``steps`` S.adam_step calls from 1-based step ``step0`` in ``dt`` -> (p, m, v) as float64 numpy.  hp: ADAM_HP, or ADAM_HP_DOUBLE for
    the hyper-parameters as doubles (adam_step's own defaults)."""
    P, G_, M, V = ({"x": _t(a, dt).clone()} for a in (p, g, m, v))
    for s in range(steps):
        S.adam_step(P, G_, M, V, step0 + s, **hp)
    return tuple(d["x"].double().numpy() for d in (P, M, V))


# ---- error measures ----------------------------------------------------------------------------------------------------------------------
def max_rel(a, b):
    """largest element error over the reference tensor's largest magnitude"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def max_abs(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def elem_rel(a, b, floor=0.0):
    """largest |a - b| / max(|b|, floor) element by element"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(np.maximum(np.abs(b), floor), 1e-300)).max())


def forward_errors(got, ref):
    """{quantity: error} of one group's forward tensors ``got`` (any subset of the names) against the float64 ``ref``: rewards absolute (they
    live in (0, 1)), every saved tensor by max_rel."""
    e = {}
    if "reward" in got:
        e["reward"] = max_abs(got["reward"], ref["reward"])
    for k in SAVED:
        if k in got:
            e[k] = max_rel(got[k], ref[k])
    return e


def backward_errors(got_r, got_g, got_lg, got_lr, ref):
    """{quantity: error} of a backward result against backward_ref's: losses relative, gradients as the worst tensor's rel_l2 / max_rel
    (cross_attention_fc.bias, exactly 0 on the device, is asserted apart)."""
    r, g, lg, lr_ = ref
    keys = [k for k in S.REWARDER_KEYS if k != "cross_attention_fc.bias"]
    return dict(reward=max_abs(got_r, r), loss=max(abs(got_lg - lg) / lg, abs(got_lr - lr_) / lr_),
                grad_l2=max(rel_l2(got_g[k], g[k]) for k in keys), grad_max=max(max_rel(got_g[k], g[k]) for k in keys))


def adam_errors(got, ref):
    """p against max(|p|, lr) element by element (half of p starts at 0: there the error is relative to the step), m and v relative."""
    return dict(adam_p=elem_rel(got[0], ref[0], LR), adam_m=elem_rel(got[1], ref[1]), adam_v=elem_rel(got[2], ref[2]))


ADAM_RUNS = (dict(id="n_params_step1", n=None, seed=1, step0=1, steps=3, zero_moments=True),       # n = rewarder_param_count(33, 100)
             dict(id="n1_step1000", n=1, seed=2, step0=1000, steps=1, zero_moments=False))
ADAM_N = sum(int(np.prod(s)) for s in S.rewarder_shapes(33, 100).values())          # == ops.rewarder_param_count(33, 100), no multiple of 256


# ---- the float32 oracle's own deviation from float64: what the bounds are made of -----------------------------------------------------------
def float32_floors():
    """{table row: worst deviation of the float32 oracle from the float64 one over the cases of that row's test}.  Forward rows are kept apart
    for the ordinary ('fwd/') and the saturated ('sat/') cases, so that the saturated softmax does not loosen the ordinary bounds."""
    with _one_thread():
        return _float32_floors()


def _float32_floors():
    fl = {}

    def up(name, v):
        fl[name] = max(fl.get(name, 0.0), v)
    for c in FORWARD:
        inp = rewarder_inputs(c)
        for r64, r32 in zip(forward_ref(c, inp), forward_ref(c, inp, torch.float32)):
            for k, v in forward_errors(r32, r64).items():
                up(("sat/" if c["sat"] else "fwd/") + k, v)
            if c["G"] == 1 and c["B"] <= 8 and not c["sat"]:
                up("max_reward", abs(float(r32["reward"].astype(np.float32).mean(dtype=np.float32)) - float(r64["reward"].mean())))
    for c in BACKWARD:
        inp = rewarder_inputs(c)
        r, g, lg, lr_ = backward_ref(c, inp, torch.float32)
        for k, v in backward_errors(r, g, lg, lr_, backward_ref(c, inp)).items():
            up("bwd/" + k, v)
    for c in GENERATOR:
        inp = generator_inputs(c)
        up("gen/out", max_abs(generator_ref(c, inp, torch.float32)[0], generator_ref(c, inp)[0]))
    for run in ADAM_RUNS:
        a = adam_inputs(run["n"] or ADAM_N, run["seed"], run["zero_moments"])
        for steps in range(1, run["steps"] + 1):
            for k, v in adam_errors(adam_ref(*a, run["step0"], steps, torch.float32), adam_ref(*a, run["step0"], steps)).items():
                up(k, v)
            up("adam_p_double", adam_errors(adam_ref(*a, run["step0"], steps, torch.float32, ADAM_HP_DOUBLE),
                                            adam_ref(*a, run["step0"], steps, hp=ADAM_HP_DOUBLE))["adam_p"])
    return fl


def kink_margin(c, inp):
    """(smallest |ReLU input| of the case in float64, largest deviation of the float32 oracle's ReLU inputs from the float64 ones), over
    mlp_fc1 and ffn_fc1 together."""
    with _one_thread():
        r64, r32 = forward_ref(c, inp)[0], forward_ref(c, inp, torch.float32)[0]
    return (min(float(np.abs(r64[k]).min()) for k in ("m1_pre", "f1_pre")), max(max_abs(r32[k], r64[k]) for k in ("m1_pre", "f1_pre")))
