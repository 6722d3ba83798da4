"""The cases of tests/test_{cpu,gpu}_score_filter*.py and their seeded inputs: the kernels of csrc/score_filter.hip one by one against a float64
numpy restatement of each operation.  Nothing is stored: every input is rebuilt from its seed, every expected value is recomputed.  The
restatements share no code with the kernels or with semireward_amd; they read the same float32 inputs, cast up, and the hyper-parameters as the
C ABI hands them to the kernels (momentum and 1 - momentum as float32 where the entry point takes floats, as ops passes them).

Every kernel gets inputs made on the CPU (float32 roundings of float64 values), not the output of another kernel, so that a deviation belongs
to the kernel it is measured on.  Data-parallel cases (``ranks`` > 1) hold n_all = ranks * B rows: the statistics (max-probs, column sums,
histograms, n_ulb / n_lb) are those of all rows, the rows masked are the first B.

Wrong versions.  Every restatement takes ``wrong=<name>``: a plausible mistake (WRONG lists them per operation).  tests/test_cpu_score_filter_cases.py
applies each to the committed cases and requires that the committed bounds reject it on at least one.

Measures and scaling (the table in the docstring of tests/test_gpu_score_filter_kernels.py repeats this):
  abs        largest |got - ref|                                       (probabilities, time_p, mu, reward means: values in [0, 1])
  max_rel    largest |got - ref| over the largest |ref| of the tensor  (state vectors, gradients; with accumulate the tensor is the whole
             dlogits that the kernel leaves, prior contents included)
  rel        |got - ref| / |ref|                                       (var)
  rel1       |got - ref| / max(|ref|, 1)                               (scalar losses: up to 28 in magnitude, and 0 for C == 1)
  / sqrt(n)  st/colsum (max_rel / sqrt(B)), fm/time_p_mean (abs / sqrt(n_all)), ce/loss (rel1 / sqrt(B)): a left-to-right float32 sum of n
             terms strays by a random walk of n roundings, and the float32 evaluation that prices them sums left to right as well
  weight     |got - ref| / (ref * max(1, -ln ref)): the SoftMatch weight exp(-x) carries the ABSOLUTE error of its exponent x as a RELATIVE
             error, and the exponent's error grows with x
"""
import numpy as np
import torch

from oracle import hooks_ref as H

F32, F64 = np.float32, np.float64
NEAR = 1e-6                      # rows this close (float64) to their threshold, or with a top-two gap this small, may fall on either side
NEAR_SHARE = 0.02                # ... and at most this share of a case's rows may be that close (the committed cases have none)
EPS_DA = F64(F32(1e-6))          # float32 constants as the kernels hold them
EPS_ENT = F64(F32(1e-12))
CLIP_HI = F64(F32(0.95))
Q = 0.8
CONFIG_M = 0.999                 # the configs' momentum (ema_p); 0 and 0.5 beside it
PLANTS = ("tie_first_last", "tie_three", "onehot_pos", "onehot_neg", "all_equal")


def _rng(*key):
    return np.random.Generator(np.random.PCG64([int(k) for k in key]))


def softmax64(z):
    z = np.asarray(z, F64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def make_logits(rng, B, C, plants=PLANTS):
    """float32 logits [B, C] with per-row scales 0.2 .. 6 and, from the last row backwards (row 0 stays ordinary), the planted rows of
    _score_rows_cases.make_case: ties for the maximum, saturated rows (+-80), an all-equal row.  -> (z, {plant: row})."""
    z = (rng.normal(size=(B, C)) * rng.uniform(0.2, 6.0, size=(B, 1))).astype(F32)
    planted = {}
    todo = [p for p in plants if not (p == "tie_first_last" and C < 2) and not (p == "tie_three" and C < 3)]
    for k, name in enumerate(todo):
        r = B - 1 - k
        if r < 1:
            break
        planted[name] = r
        top = F32(np.abs(z[r]).max() + 1.0)
        if name == "tie_first_last":
            z[r, 0] = z[r, C - 1] = top
        elif name == "tie_three":
            z[r, 0] = z[r, C // 2] = z[r, C - 1] = top
        elif name == "onehot_pos":
            z[r] = F32(-80.0)
            z[r, (C - 1) // 2] = F32(80.0)
        elif name == "onehot_neg":
            z[r] = F32(80.0)
            if C >= 2:
                z[r, : C - 1] = F32(-80.0)
        else:
            z[r] = F32(rng.normal())
    return z, planted


def top_gap(p):
    """float64 gap between the two largest entries of every row (inf for one column)"""
    p = np.asarray(p, F64)
    if p.shape[1] == 1:
        return np.full(p.shape[0], np.inf)
    s = np.sort(p, axis=1)
    return s[:, -1] - s[:, -2]


def dirichlet(rng, C):
    return np.maximum(rng.dirichlet(np.full(C, 2.0)), 1e-4 / C).astype(F32)


def by_id(cases, cid):
    return next(c for c in cases if c["id"] == cid)


# ==== 1. row softmax / max / argmax (row_max_kernel), dense and strided =====================================================================
def _row(B, C, seed=0, rpg=0, pad=0):
    return dict(B=B, C=C, seed=seed, rpg=rpg or B, pad=pad, id="B%d_C%d" % (B, C))


# C = 1, 2 (idle lanes in the argmax shuffle); 63 / 64 / 65 (one-wave boundary); 256 / 257; 1000; 2048.  B = 1; 3 (fewer rows than the four
# waves of a workgroup); 5 (a partial second workgroup); 64 / 65; 257; 1024.  rpg / pad: the strided form reads groups of rpg rows, pad filler
# rows between the groups.
ROWS = (
    _row(1, 1, rpg=1, pad=2), _row(3, 2, rpg=2, pad=1), _row(5, 63, rpg=2, pad=3), _row(5, 64, rpg=5, pad=1), _row(65, 65, rpg=8, pad=2),
    _row(64, 256, rpg=16, pad=1), _row(5, 257, rpg=3, pad=2), _row(3, 1000, rpg=1, pad=1), _row(4, 2048, rpg=2, pad=1),
    _row(257, 3, rpg=64, pad=5), _row(1024, 2, rpg=128, pad=1),
)


def row_inputs(c):
    z, planted = make_logits(_rng(11, c["seed"], c["B"], c["C"]), c["B"], c["C"])
    return dict(z=z, planted=planted)


def row_ref(c, inp, wrong=None):
    """probs, maxp, idx (first maximal column) and the top-two gap that says which argmax rows are decided."""
    p = softmax64(inp["z"])
    return dict(probs=p, maxp=p.max(axis=1), idx=p.argmax(axis=1).astype(np.int64), gap=top_gap(p))


def row_f32(c, inp):
    p = H.softmax_probs(torch.from_numpy(inp["z"]))
    return dict(probs=p.numpy(), maxp=p.max(dim=1)[0].numpy())


# ==== 2. column sums and predicted-class histogram (freematch_stats_kernel, grid ceil(C / 256)) ==============================================
def _st(B, C, seed=0):
    return dict(B=B, C=C, seed=seed, id="B%d_C%d" % (B, C))


# C = 257, 1000, 2048: the second and later workgroups; C = 1, 2, 63 .. 65: a partial first one.  B = 257, 1024: a long sequential sum.
STATS = (_st(1, 1), _st(3, 2), _st(5, 63), _st(64, 64), _st(65, 65), _st(5, 256), _st(5, 257), _st(3, 1000), _st(4, 2048), _st(257, 3),
         _st(1024, 2))


def probs_f32(rng, n, C, plants=PLANTS):
    """float32 probabilities [n, C] (float64 softmax, rounded), their row max and first argmax -- exact functions of the float32 rows"""
    z, planted = make_logits(rng, n, C, plants)
    p = softmax64(z).astype(F32)
    return p, p.max(axis=1), p.argmax(axis=1).astype(np.int64), planted


def stats_inputs(c):
    p, _, idx, _ = probs_f32(_rng(12, c["seed"], c["B"], c["C"]), c["B"], c["C"])
    return dict(probs=p, idx=idx)


def stats_ref(c, inp, wrong=None):
    p, idx = inp["probs"].astype(F64), inp["idx"]
    if wrong == "drop_last_row" and c["B"] > 1:
        p, idx = p[:-1], idx[:-1]
    if wrong == "drop_rows_past_256":
        p, idx = p[:256], idx[:256]
    return dict(colsum=p.sum(axis=0), hist=np.bincount(idx, minlength=c["C"]).astype(F64))


def stats_f32(c, inp):
    s = np.zeros(c["C"], F32)
    for row in inp["probs"]:
        s = s + row                                          # left to right in float32
    return dict(colsum=s)


def colsum_err(got, ref, B):
    return max_rel(got, ref) / np.sqrt(B)


# ==== 3. FreeMatch time_p / p_model / label_hist / mask (freematch_update_kernel, ONE workgroup) ===============================================
def _fm(B, C, ranks=1, m=0.0, uq=True, clip=False, steps=1, seed=0, plant=None, note=""):
    c = dict(B=B, C=C, ranks=ranks, n_all=ranks * B, m=m, uq=uq, clip=clip, steps=steps, seed=seed, plant=plant)
    c["id"] = "B%d_C%d_n%d_m%g_%s" % (B, C, c["n_all"], m, "q" if uq else "mean") + ("_clip" if clip else "") + ("_x%d" % steps if steps > 1 else "") \
        + ("_" + plant if plant else "")
    return c


FREEMATCH = (
    # exact tie at the threshold: m = 0, the mean rule, n_all = 1 -- time_p is the row's confidence, p_model the row, the modulation 1:
    # conf >= time_p * 1 holds with equality in float32 and float64 alike, the row is kept
    _fm(1, 5, uq=False, seed=1),
    _fm(1, 1),                                                       # quantile of one value (rank 0, w == 0); C = 1: idle lanes, mod = 1
    _fm(2, 2, seed=1),                                               # n = 2: rank 0.8, w >= 0.5
    _fm(3, 63, m=0.5),                                               # n = 3: rank 1.6, w >= 0.5; fewer rows than waves
    _fm(4, 64),                                                      # n = 4: rank 2.4, w < 0.5
    _fm(3, 65, ranks=2, seed=2),                                     # n_all = 6 = 2 B: rank 4, integral (w == 0)
    _fm(11, 10, m=CONFIG_M, seed=1),                                 # n = 11: rank 8, integral; the configs' momentum
    _fm(257, 3),                                                     # n = 257: second stride of the rank-by-counting and mask loops
    _fm(1024, 2, seed=1),                                            # n = 1024 = B: the srt[] cap
    _fm(256, 3, ranks=4, seed=3),                                    # n_all = 4 B = 1024, quantile over the gathered max-probs
    _fm(256, 3, ranks=4, uq=False, seed=4),                          # ... and the mean over them
    _fm(5, 257, ranks=3, uq=False, seed=1),                          # n_all = 15 = 3 B (odd multiple); C = 257: second `c += 256` stride
    _fm(5, 256, ranks=3, seed=2),                                    # C = 256: the stride exactly filled
    _fm(4, 1000, ranks=4, m=0.5, seed=1),                            # n_all = 16; C = 1000
    _fm(3, 2048, uq=False),                                          # C = 2048
    _fm(64, 10, m=0.5, steps=4, seed=5),                             # state carried over four calls
    _fm(65, 100, ranks=3, m=CONFIG_M, uq=False, clip=True, steps=3, seed=1),
    _fm(40, 10, seed=1, plant="ones_block"),                         # rows 28 .. 39 hold 1.0f exactly: the tie block straddles rank 31.2
    _fm(40, 10, clip=True, seed=2, plant="ones_block"),              # ... and the quantile 1.0 is clipped to 0.95f
    _fm(16, 1, seed=1),                                              # all max-probs equal (C = 1): every srt[] slot filled by the index tie break
    _fm(16, 1, uq=False, m=0.5, seed=2),
)


def freematch_inputs(c):
    """Per step: probabilities of all n_all rows -> maxp_all, colsum and hist over all rows, the local B rows' max_probs / max_idx; the
    initial state."""
    B, C, n = c["B"], c["C"], c["n_all"]
    rng = _rng(13, c["seed"], B, C, n)
    steps = []
    for t in range(c["steps"]):
        p, mp, idx, planted = probs_f32(rng, n, C)
        if c["plant"] == "ones_block":
            p[28:] = 0.0
            p[np.arange(28, n), idx[28:]] = 1.0
            mp = p.max(axis=1)
        steps.append(dict(probs_all=p, maxp_all=mp, idx_all=idx, colsum=p.astype(F64).sum(axis=0).astype(F32),
                          hist=np.bincount(idx, minlength=C).astype(F32), planted=planted))
    return dict(steps=steps, time_p=np.array([rng.uniform(0.3, 0.9)], F32), p_model=dirichlet(rng, C), label_hist=dirichlet(rng, C))


def quantile64(x, wrong=None):
    """torch.quantile(x, 0.8), 'linear', in float64"""
    s = np.sort(np.asarray(x, F64))
    n = s.size
    rank = Q * (n - 1)
    if wrong == "rank_0.8n":
        rank = min(Q * n, n - 1.0)
    lo, hi = int(np.floor(rank)), int(np.ceil(rank))
    w = rank - lo
    if wrong == "floor_rank":
        return s[lo]
    if wrong == "lerp_from_the_other_end":                   # ATen's two branches, a + w (b - a) and b - (b - a)(1 - w), are the same real number:
        return s[hi] - (s[hi] - s[lo]) * w                   # what a wrong branch can get wrong is the end that w counts from
    return s[lo] + w * (s[hi] - s[lo])


def lerp_weight(n):
    """the float32 interpolation weight of the 0.8-quantile of n values, as the kernel's (and ATen's) branch sees it"""
    rank = F32(0.8) * F32(n - 1)
    return float(rank - np.floor(rank))


def freematch_ref(c, inp, wrong=None):
    """List per step of dict(stat, time_p, p_model, label_hist, mask, thr, conf, near, exact)."""
    B, n = c["B"], c["n_all"]
    m, om = F64(F32(c["m"])), F64(F32(1 - c["m"]))
    tp, pm, lh = F64(inp["time_p"][0]), inp["p_model"].astype(F64), inp["label_hist"].astype(F64)
    out = []
    for s in inp["steps"]:
        x = s["maxp_all"].astype(F64)
        colsum, hist, n_div = s["colsum"].astype(F64), s["hist"].astype(F64), n
        if wrong == "local_rows_only":
            x, n_div = x[:B], B
            colsum, hist = s["probs_all"][:B].astype(F64).sum(axis=0), np.bincount(s["idx_all"][:B], minlength=c["C"]).astype(F64)
        if wrong == "drop_last_row" and n > 1:
            x = x[:-1]
        if wrong == "drop_rows_past_256":
            x = x[:256]
        stat = quantile64(x, wrong) if c["uq"] else x.mean()
        tp = tp * m + om * stat
        if c["clip"]:
            tp = min(max(tp, 0.0), CLIP_HI)
        pm = pm * m + om * (colsum / n_div)
        lh = lh * m + om * (hist / hist.sum())
        conf, idx = s["maxp_all"][:B].astype(F64), s["idx_all"][:B]
        thr = tp * (pm[idx] / pm.max())
        exact = conf == thr
        out.append(dict(stat=stat, time_p=tp, p_model=pm.copy(), label_hist=lh.copy(), mask=(conf >= thr).astype(F64), thr=thr, conf=conf,
                        exact=exact, near=(np.abs(conf - thr) <= NEAR) & ~exact))
    return out


def freematch_f32(c, inp):
    """oracle.hooks_ref.FreeMatchState in float32 on all n_all rows; under the mean rule time_p is redone with the plain left-to-right float32
    sum (torch.mean's blocked sum would price a sequential sum of 1024 terms too low)."""
    st = H.FreeMatchState(c["C"], c["m"], c["uq"], c["clip"])
    st.time_p, st.p_model, st.label_hist = torch.tensor(inp["time_p"][0]), torch.from_numpy(inp["p_model"].copy()), torch.from_numpy(inp["label_hist"].copy())
    tp, m, om = inp["time_p"][0], F32(c["m"]), F32(1 - c["m"])
    out = []
    for s in inp["steps"]:
        st.masking(torch.from_numpy(s["probs_all"]))
        tp = F32(F32(tp * m) + F32(om * F32(np.cumsum(s["maxp_all"], dtype=F32)[-1] / F32(c["n_all"]))))
        if c["clip"]:
            tp = min(max(tp, F32(0.0)), F32(0.95))
        out.append(dict(time_p=float(st.time_p) if c["uq"] else float(tp), p_model=st.p_model.numpy().copy(), label_hist=st.label_hist.numpy().copy()))
    return out


# ==== 4. fairness loss and its gradient (freematch_entropy_kernel, ONE workgroup) ==============================================================
def _en(B, C, sel="some", seed=0, lh_zeros=0, unpredicted=0, acc=False, gs=1.0):
    c = dict(B=B, C=C, sel=sel, seed=seed, lh_zeros=lh_zeros, unpredicted=unpredicted, acc=acc, gs=gs)
    c["id"] = "B%d_C%d_%s" % (B, C, sel) + ("_lh0" if lh_zeros else "") + ("_h0" if unpredicted else "") + ("_acc" if acc else "")
    return c


ENTROPY = (
    _en(1, 1, sel="all"), _en(3, 2, sel="one", seed=1),             # B < 4: fewer rows than waves; exactly one selected row
    _en(5, 63), _en(5, 64, sel="all", acc=True, gs=0.5), _en(64, 65, seed=1, lh_zeros=3),
    _en(65, 10, unpredicted=2, lh_zeros=2, seed=2),                 # classes only unselected rows predict (h == 0, a = 0); label_hist zeros
    _en(5, 256, seed=1), _en(5, 257, seed=2, acc=True, gs=3.0),     # C = 257: second `c += 256` stride
    _en(3, 1000, seed=1),                                           # most classes unpredicted (C > B)
    _en(4, 2048, sel="all"),                                        # the g[] cap
    _en(257, 3, seed=1),                                            # second stride of the row-count loop
    _en(1024, 2, seed=2), _en(1024, 3, sel="one", seed=3, acc=True, gs=0.25),     # the pred[] cap
    _en(8, 10, sel="none"), _en(8, 10, sel="none", acc=True, gs=2.0),              # no row selected: loss 0, gradient 0 / left untouched
)


def entropy_inputs(c):
    B, C = c["B"], c["C"]
    rng = _rng(14, c["seed"], B, C)
    z, planted = make_logits(rng, B, C, PLANTS if B >= 8 else ())
    pred = softmax64(z).argmax(axis=1)
    if c["sel"] == "all":
        mask = np.ones(B, F32)
    elif c["sel"] == "none":
        mask = np.zeros(B, F32)
    elif c["sel"] == "one":
        mask = np.zeros(B, F32)
        mask[B // 2] = 1.0
    else:
        mask = (rng.random(B) < 0.6).astype(F32)
        mask[0], mask[B - 1] = 1.0, 0.0
    dropped = []
    if c["unpredicted"]:
        dropped = [int(k) for k in np.unique(pred)[: c["unpredicted"]]]
        mask[np.isin(pred, dropped)] = 0.0
    pm, lh = dirichlet(rng, C), dirichlet(rng, C)
    if c["lh_zeros"]:
        lh[rng.permutation(C)[: c["lh_zeros"]]] = 0.0
    inp = dict(z=z, mask=mask, p_model=pm, label_hist=lh, planted=planted, dropped=dropped, d0=None)
    if c["acc"]:                                             # prior dlogits of the size of the gradient that is added to them
        g = entropy_ref(c, inp)["grad"]
        inp["d0"] = (rng.normal(size=(B, C)) * max(np.abs(g).max(), 1e-3)).astype(F32)
    return inp


def entropy_ref(c, inp, wrong=None):
    """loss and grad_scale * d loss / d logits in float64, in the analytic form (tests/test_cpu_score_filter_cases.py holds it against float64
    autograd of oracle.hooks_ref.freematch_entropy_loss); 'out': what dlogits must hold afterwards."""
    B, C = c["B"], c["C"]
    p = softmax64(inp["z"])
    sel = inp["mask"] != 0
    ns = int(sel.sum())
    d0 = inp["d0"].astype(F64) if inp["d0"] is not None else None
    if ns == 0:
        z = np.zeros((B, C))
        return dict(loss=0.0, grad=z, out=d0 if d0 is not None else z, pred=p.argmax(axis=1), gap=top_gap(p), h=np.zeros(C))
    pred = p.argmax(axis=1)
    mean = p[sel].mean(axis=0)
    h = np.bincount(pred[sel], minlength=C) / ns
    if wrong == "hist_ignores_mask":
        h = np.bincount(pred, minlength=C) / B
    inv = lambda v: np.where(v > 0, 1.0 / np.where(v > 0, v, 1.0), 0.0)  # noqa: E731
    a = inv(h)
    lh = inp["label_hist"].astype(F64)
    w = inp["p_model"].astype(F64) * inv(lh)
    w = w / w.sum()
    u = mean * a
    Z = u.sum()
    q = u / Z
    loss = float((w * np.log(q + EPS_ENT)).sum())
    cross = 0.0 if wrong == "no_cross_term" else (w * q / (q + EPS_ENT)).sum()
    ag = inv(np.bincount(pred, minlength=C) / B) if wrong == "a_from_all_rows" else a           # (the kernel recomputes a_c for the gradient)
    g = ag * (w / (q + EPS_ENT) - cross) / Z
    grad = np.zeros((B, C))
    grad[sel] = c["gs"] * p[sel] * (g[None, :] - (p[sel] * g[None, :]).sum(axis=1, keepdims=True)) / ns
    return dict(loss=loss, grad=grad, out=grad + d0 if d0 is not None else grad, pred=pred, gap=top_gap(p), h=h)


def entropy_autograd(c, inp, dt=torch.float64):
    """(loss, grad_scale * gradient) by autograd of oracle.hooks_ref.freematch_entropy_loss in ``dt``"""
    z = torch.from_numpy(inp["z"]).to(dt).requires_grad_(True)
    loss = H.freematch_entropy_loss(torch.from_numpy(inp["mask"]), z, torch.from_numpy(inp["p_model"]).to(dt), torch.from_numpy(inp["label_hist"]).to(dt))
    loss.backward()
    return float(loss.detach()), c["gs"] * z.grad.double().numpy()


# ==== 5. DistAlign EMA and aligned probabilities (distalign_kernel, ONE workgroup) ============================================================
def _da(B, C, ranks=1, m=0.5, model=False, steps=2, seed=0, n_lb=0):
    c = dict(B=B, C=C, ranks=ranks, n_ulb=ranks * B, n_lb=(n_lb or max(1, B // 2)) if model else 0, m=m, model=model, steps=steps, seed=seed)
    c["id"] = "B%d_C%d_n%d_m%g_%s_x%d" % (B, C, c["n_ulb"], m, "model" if model else "uniform", steps)
    return c


# step 0 of every case is the first-call form (p_model := batch mean whatever m is), the later steps the EMA form
DISTALIGN = (
    _da(1, 1, steps=2),                                             # C = 1: idle lanes in the argmax shuffle, aligned == 1
    _da(3, 2, model=True, m=0.0, seed=1),                           # fewer rows than waves; m = 0: the later call's state is the batch mean, undamped
    _da(5, 63, m=0.0, seed=3), _da(5, 64, model=True, seed=1),      # one-wave boundary
    _da(65, 65, ranks=3, model=True, m=CONFIG_M, steps=3, seed=1),  # n_ulb = 3 B (odd multiple), n_lb != B; the configs' momentum
    _da(5, 256, ranks=4, seed=2),                                   # n_ulb = 4 B; C = 256: the `c += 256` stride exactly filled
    _da(5, 257, ranks=4, model=True, m=0.0, seed=1),                # C = 257: the second `c += 256` stride of the EMA loop
    _da(3, 1000, model=True, seed=2), _da(4, 2048, ranks=3, seed=1),
    _da(257, 3, model=True, seed=1), _da(1024, 2, steps=2, seed=2),  # second stride of the row loop; B = 1024
    _da(64, 10, model=True, steps=4, seed=3),                       # state carried over four calls at m = 0.5
)


def distalign_inputs(c):
    B, C = c["B"], c["C"]
    rng = _rng(15, c["seed"], B, C, c["n_ulb"])
    steps = []
    for t in range(c["steps"]):
        p, _, _, _ = probs_f32(rng, c["n_ulb"], C, ("onehot_pos", "onehot_neg") if c["n_ulb"] >= 8 else ())
        s = dict(probs_all=p, colsum_ulb=p.astype(F64).sum(axis=0).astype(F32), probs_lb=None, colsum_lb=None)
        if c["model"]:
            s["probs_lb"] = probs_f32(rng, c["n_lb"], C, ())[0]
            s["colsum_lb"] = s["probs_lb"].astype(F64).sum(axis=0).astype(F32)
        steps.append(s)
    return dict(steps=steps, p_target=np.full(C, 1.0 / C, F32))


def distalign_ref(c, inp, wrong=None):
    B = c["B"]
    m, om = F64(F32(c["m"])), F64(F32(1.0 - c["m"]))
    pm, pt = None, inp["p_target"].astype(F64)
    out = []
    for s in inp["steps"]:
        mean_u = s["colsum_ulb"].astype(F64) / c["n_ulb"]
        if wrong == "mean_over_local_rows":
            mean_u = s["probs_all"][:B].astype(F64).mean(axis=0)
        if pm is None:
            pm = mean_u * om if wrong == "first_call_is_an_ema_step" else mean_u
        else:
            pm = pm * m + mean_u * om
        if c["model"] and wrong != "p_target_not_updated":
            pt = pt * m + (s["colsum_lb"].astype(F64) / c["n_lb"]) * om
        a = s["probs_all"][:B].astype(F64) * (pt + EPS_DA) / (pm + EPS_DA)
        a = a / a.sum(axis=1, keepdims=True)
        out.append(dict(p_model=pm.copy(), p_target=pt.copy(), aligned=a, maxp=a.max(axis=1), idx=a.argmax(axis=1).astype(np.int64), gap=top_gap(a)))
    return out


def distalign_f32(c, inp):
    st = H.DistAlignState(c["C"], c["m"], "model" if c["model"] else "uniform")
    out = []
    for s in inp["steps"]:
        a = st.dist_align(torch.from_numpy(s["probs_all"]), torch.from_numpy(s["probs_lb"]) if c["model"] else None)[: c["B"]]
        out.append(dict(p_model=st.p_model.numpy().copy(), p_target=st.p_target.numpy().copy(), aligned=a.numpy(), maxp=a.max(dim=1)[0].numpy()))
    return out


# ==== 6. SoftMatch mu / var EMA and weight (softmatch_mask_kernel, ONE workgroup) ==============================================================
def _sm(B, ranks=1, m=0.0, ns=2, steps=1, seed=0, spread=1.0):
    c = dict(B=B, ranks=ranks, n_all=ranks * B, m=m, ns=ns, steps=steps, seed=seed, spread=spread)
    c["id"] = "B%d_n%d_m%g_s%d" % (B, c["n_all"], m, ns) + ("_x%d" % steps if steps > 1 else "")
    return c


# B = 1 needs ranks >= 2 (the unbiased variance of one value is nan, in the reference too)
SOFTMATCH = (
    _sm(1, ranks=2, seed=1), _sm(3, seed=1),                        # m = 0: mu and var after one call are the batch mean and unbiased variance
    _sm(5, ranks=3, m=0.5, seed=2),                                 # n_all = 3 B (odd multiple)
    _sm(64, ns=3, seed=1), _sm(65, ranks=4, seed=2),                # n_all = 4 B = 260: second stride of the two sums
    _sm(257, m=CONFIG_M, seed=1), _sm(1024, seed=3),                # second stride of the weight loop; B = 1024
    _sm(256, ranks=4, ns=1, seed=1),                                # n_all = 1024, the local rows a quarter of it
    _sm(5, ranks=205, m=0.5, seed=4),                               # n_all = 1025: this kernel has no cap at 1024
    _sm(64, m=0.5, steps=4, seed=5),                                # state carried over four calls
)


def softmatch_inputs(c):
    rng = _rng(16, c["seed"], c["B"], c["n_all"])
    # max-probs in (0.2, 1): a beta draw, one row at 1.0f exactly from n_all >= 4 on
    steps = []
    for t in range(c["steps"]):
        x = (0.2 + 0.8 * rng.beta(2.0, 1.5, size=c["n_all"])).astype(F32)
        if c["n_all"] >= 4:
            x[c["B"] - 1 if c["B"] > 1 else 1] = 1.0
        steps.append(x)
    return dict(steps=steps, mu_var=np.array([0.1, 1.0], F32) if c["steps"] > 1 or c["m"] != 0 else np.array([0.7, 0.3], F32))


def softmatch_ref(c, inp, wrong=None):
    B, n, m = c["B"], c["n_all"], F64(c["m"])
    mu, var = F64(inp["mu_var"][0]), F64(inp["mu_var"][1])
    out = []
    for xs in inp["steps"]:
        x = xs.astype(F64)
        if wrong == "local_rows_only" and B > 1:
            x = x[:B]
        if wrong == "drop_last_row" and x.size > 2:
            x = x[:-1]
        if wrong == "drop_rows_past_256":
            x = x[:256]
        mean = x.mean()
        varb = ((x - mean) ** 2).sum() / (x.size if wrong == "variance_over_n" else x.size - 1)
        mu, var = m * mu + (1.0 - m) * mean, m * var + (1.0 - m) * varb
        d = np.minimum(xs[:B].astype(F64) - mu, 0.0)
        out.append(dict(mu=mu, var=var, weight=np.exp(-(d * d) / (2.0 * var / c["ns"] ** 2))))
    return out


def softmatch_f32(c, inp):
    st = H.SoftMatchState(10, c["ns"], c["m"])
    st.mu, st.var = torch.tensor(inp["mu_var"][0]), torch.tensor(inp["mu_var"][1])
    out = []
    for xs in inp["steps"]:
        w = st.masking(torch.from_numpy(xs).view(-1, 1))[: c["B"]]
        out.append(dict(mu=float(st.mu), var=float(st.var), weight=w.numpy()))
    return out


def weight_err(got, ref):
    """the SoftMatch weight through its exponent: |got - ref| / (ref * max(1, -ln ref))"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    return float((np.abs(got - ref) / (ref * np.maximum(1.0, -np.log(ref)))).max())


# ==== 7. masked cross-entropy (masked_ce_kernel, ONE workgroup) ================================================================================
def _ce(B, C, masks=2, gs=1.0, seed=0, soft=False):
    c = dict(B=B, C=C, masks=masks, gs=gs, seed=seed, soft=soft)
    c["id"] = "B%d_C%d_masks%d" % (B, C, masks) + ("_soft" if soft else "")
    return c


MASKED_CE = (
    _ce(1, 1, masks=0), _ce(3, 2, masks=1, seed=1), _ce(5, 63, gs=0.5), _ce(5, 64, masks=1, soft=True), _ce(65, 65, seed=1), _ce(64, 256, masks=0, gs=2.0),
    _ce(5, 257, seed=1), _ce(3, 1000, masks=1, seed=2), _ce(4, 2048, seed=1), _ce(257, 3, seed=2),
    _ce(1024, 3, seed=1),                                            # B = 1024: rowloss[] filled to its cap, the sequential sum
    _ce(1025, 3, seed=2, gs=0.5),                                    # B = 1025: the per-wave acc / part[4] path
    _ce(1025, 2, masks=0, seed=3),
)


def ce_inputs(c):
    B, C = c["B"], c["C"]
    rng = _rng(17, c["seed"], B, C)
    z, planted = make_logits(rng, B, C, PLANTS if B >= 8 else ())
    y = rng.integers(0, C, size=B, dtype=np.int64)
    if "onehot_pos" in planted:
        y[planted["onehot_pos"]] = 0                                # C >= 3: the target sits on a -80 logit, nll = 160
    mask = mask2 = None
    if c["masks"] >= 1:
        mask = rng.beta(2.0, 2.0, size=B).astype(F32) if c["soft"] else (rng.random(B) < 0.6).astype(F32)
        mask[0] = 1.0
        if B > 1:
            mask[B - 1] = 0.0
    if c["masks"] >= 2:
        mask2 = (rng.random(B) < 0.7).astype(F32)
        mask2[0] = 1.0
    return dict(z=z, y=y, mask=mask, mask2=mask2, planted=planted)


def ce_weights(inp, B):
    w = np.ones(B, F64)
    for k in ("mask", "mask2"):
        if inp[k] is not None:
            w = w * inp[k].astype(F64)
    return w


def ce_ref(c, inp, wrong=None):
    """loss = mean over ALL rows of nll * mask * mask2 (grad_scale does not enter it); dlogits = grad_scale * w (softmax - onehot) / B"""
    B, C = c["B"], c["C"]
    z = inp["z"].astype(F64)
    p = softmax64(z)
    mx = z.max(axis=1)
    nll = (mx + np.log(np.exp(z - mx[:, None]).sum(axis=1))) - z[np.arange(B), inp["y"]]
    w = ce_weights(inp, B)
    den = B
    if wrong == "mean_over_selected_rows":
        den = max(int((w != 0).sum()), 1)
    oh = np.zeros((B, C))
    oh[np.arange(B), inp["y"]] = 1.0
    return dict(loss=float((nll * w).sum() / den), dlogits=c["gs"] * w[:, None] * (p - oh) / den, w=w)


def ce_f32(c, inp):
    """float32 autograd of oracle.hooks_ref.consistency_loss for dlogits; the loss as the left-to-right float32 sum of its float32 rows"""
    z = torch.from_numpy(inp["z"]).requires_grad_(True)
    t = lambda a: None if a is None else torch.from_numpy(a)  # noqa: E731
    loss = H.consistency_loss(z, torch.from_numpy(inp["y"]), t(inp["mask"]), t(inp["mask2"]))
    (loss * float(F32(c["gs"]))).backward()
    rows = H.ce_loss_rows(z.detach(), torch.from_numpy(inp["y"])).numpy()
    for k in ("mask", "mask2"):
        if inp[k] is not None:
            rows = rows * inp[k]
    return dict(loss=float(np.cumsum(rows, dtype=F32)[-1] / F32(c["B"])), dlogits=z.grad.numpy())


# ==== 8. reward-mean mask (reward_mask2_kernel: one workgroup of one wave per group) ============================================================
def _rw(groups, Bg, total=None, mean_in=False, seed=0, plant=None):
    c = dict(groups=groups, Bg=Bg, total=total or groups * Bg, mean_in=mean_in, seed=seed, plant=plant)
    c["id"] = "G%d_B%d" % (groups, Bg) + ("_t%d" % total if total else "") + ("_meanin" if mean_in else "") + ("_" + plant if plant else "")
    return c


REWARD = (
    _rw(1, 1), _rw(2, 3, seed=1), _rw(3, 8, seed=2), _rw(2, 64, seed=1),       # B <= 64: the left-to-right sum
    _rw(2, 65, seed=1), _rw(2, 257, seed=2),                                    # B > 64: per-lane partials and the shuffle tree
    _rw(3, 8, total=19, seed=3), _rw(3, 64, total=129, seed=1),                 # ragged: the last group holds 3 rows / 1 row
    _rw(2, 65, total=129, seed=2), _rw(3, 257, total=600, seed=1),              # ragged: last group 64 rows (the other sum order than its peers) / 86
    _rw(3, 8, mean_in=True, seed=4), _rw(2, 65, mean_in=True, seed=3), _rw(2, 257, mean_in=True, seed=1),
    _rw(2, 8, plant="all_equal"), _rw(2, 65, plant="all_equal"),               # every reward equals the mean: all kept
    _rw(2, 4, plant="one_at_mean"), _rw(1, 68, plant="one_at_mean"),           # multiples of 1/64: exact sums, one row exactly at the mean
)


def reward_inputs(c):
    G, Bg = c["groups"], c["Bg"]
    rng = _rng(18, c["seed"], G, Bg, c["total"])
    r = rng.random(G * Bg).astype(F32)
    if c["plant"] == "all_equal":
        r[:] = 0.5
        r[Bg:] = 0.8125
    elif c["plant"] == "one_at_mean":                        # 0.25, 0.75 pairs around 0.5, then one 0.5 -- every partial sum is a multiple of 1/4
        r[:] = np.tile(np.array([0.25, 0.75], F32), G * Bg // 2)
        r[Bg // 2:: Bg] = 0.5
        r[Bg // 2 + 1:: Bg] = 0.5
    r[c["total"]:] = np.nan                                  # rows past total are never read
    mean_in = None
    if c["mean_in"]:                                         # a "global" mean that is not the group's own
        mean_in = (0.5 + 0.1 * rng.standard_normal(G)).astype(F32)
    return dict(reward=r, mean_in=mean_in)


def group_rows(c, g):
    return min(c["Bg"], c["total"] - g * c["Bg"])


def reward_ref(c, inp, wrong=None):
    G, Bg = c["groups"], c["Bg"]
    r = inp["reward"].astype(F64)
    mean, mask, near = np.zeros(G), np.full(G * Bg, np.nan), np.zeros(G * Bg, bool)
    for g in range(G):
        n = group_rows(c, g)
        x = r[g * Bg: g * Bg + n]
        if inp["mean_in"] is not None:
            mean[g] = F64(inp["mean_in"][g])
        else:
            mean[g] = x.sum() / (Bg if wrong == "ragged_over_full_group" else n)
            if wrong == "drop_last_row" and n > 1:
                mean[g] = x[:-1].mean()
        mask[g * Bg: g * Bg + n] = x >= mean[g]
        near[g * Bg: g * Bg + n] = (np.abs(x - mean[g]) <= NEAR) & (x != mean[g])
    return dict(mean=mean, mask=mask, near=near)


def reward_f32(c, inp):
    mean = np.zeros(c["groups"], F32)
    for g in range(c["groups"]):
        n = group_rows(c, g)
        mean[g] = np.cumsum(inp["reward"][g * c["Bg"]: g * c["Bg"] + n], dtype=F32)[-1] / F32(n)      # left to right in float32
    return dict(mean=mean)


# ==== error measures =====================================================================================================================
def max_abs(a, b):
    return float(np.abs(np.asarray(a, F64) - np.asarray(b, F64)).max())


def max_rel(a, b):
    """largest element error over the reference tensor's largest magnitude"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return float(np.abs(a - b).max() / (np.abs(b).max() or 1.0))              # (an all-zero reference is compared absolutely)


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def rel1(a, b):
    """relative above 1, absolute below (a loss may be 0: C == 1)"""
    return abs(float(a) - float(b)) / max(abs(float(b)), 1.0)


def worst(a, b):
    """(flat index of the worst element, its error)"""
    e = np.abs(np.asarray(a, F64) - np.asarray(b, F64))
    i = int(e.argmax())
    return np.unravel_index(i, e.shape), float(e.ravel()[i])


def row_errors(got, ref):
    return {"rm/probs": max_abs(got["probs"], ref["probs"]), "rm/maxp": max_abs(got["maxp"], ref["maxp"])}


def stats_errors(c, got, ref):
    return {"st/colsum": colsum_err(got["colsum"], ref["colsum"], c["B"])}


def freematch_errors(c, got, ref):
    e = max_abs(got["time_p"], ref["time_p"])
    return {("fm/time_p" if c["uq"] else "fm/time_p_mean"): e if c["uq"] else e / np.sqrt(c["n_all"]), "fm/p_model": max_rel(got["p_model"], ref["p_model"]),
            "fm/label_hist": max_rel(got["label_hist"], ref["label_hist"])}


def entropy_errors(got_loss, got_out, ref):
    return {"ent/loss": rel1(got_loss, ref["loss"]), "ent/grad": max_rel(got_out, ref["out"])}


def distalign_errors(c, got, ref):
    e = {"da/p_model": max_rel(got["p_model"], ref["p_model"]), "da/aligned": max_abs(got["aligned"], ref["aligned"]),
         "da/maxp": max_abs(got["maxp"], ref["maxp"])}
    if c["model"]:
        e["da/p_target"] = max_rel(got["p_target"], ref["p_target"])
    return e


def softmatch_errors(got, ref):
    return {"sm/mu": max_abs(got["mu"], ref["mu"]), "sm/var": rel(got["var"], ref["var"]), "sm/weight": weight_err(got["weight"], ref["weight"])}


def ce_errors(c, got, ref):
    return {"ce/loss": rel1(got["loss"], ref["loss"]) / np.sqrt(c["B"]), "ce/dlogits": max_rel(got["dlogits"], ref["dlogits"])}


def reward_errors(got, ref):
    return {"rw/mean": max_abs(got["mean"], ref["mean"])}


# The float32 evaluation's worst deviation from the float64 restatement per compared quantity over the committed cases (float32_floors()
# below, one thread), to three digits: the table in the docstring of tests/test_gpu_score_filter_kernels.py.
# tests/test_cpu_score_filter_cases.py measures them afresh and holds each within FLOOR_HEADROOM of the figure here, from both sides.
# A kernel's bound is 8 x the floor, at least 1e-7.
FLOORS = {
    "rm/probs": 1.35e-7, "rm/maxp": 1.35e-7, "st/colsum": 4.05e-8, "fm/time_p": 6.56e-8, "fm/time_p_mean": 7.45e-9, "fm/p_model": 1.38e-7,
    "fm/label_hist": 5.73e-8, "ent/loss": 1.44e-7, "ent/grad": 5.21e-7, "da/p_model": 1.63e-7, "da/p_target": 1.19e-7, "da/aligned": 2.02e-7,
    "da/maxp": 2.02e-7, "sm/mu": 5.97e-8, "sm/var": 6.77e-8, "sm/weight": 5.35e-7, "ce/loss": 3.25e-8, "ce/dlogits": 1.56e-7, "rw/mean": 1.42e-7,
}
FLOOR_HEADROOM = 0.01            # rounding to three digits is 0.5 %; the rest is for a float32 sum that another CPU orders differently
BOUNDS = {k: max(8.0 * f, 1e-7) for k, f in FLOORS.items()}


class _one_thread:
    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *a):
        torch.set_num_threads(self.n)


def float32_floors():
    """{table row: worst deviation of the float32 evaluation from the float64 restatement over the committed cases}"""
    with _one_thread():
        return _float32_floors()


def _float32_floors():
    fl = {}

    def up(errors):
        for k, v in errors.items():
            fl[k] = max(fl.get(k, 0.0), v)
    for c in ROWS:
        inp = row_inputs(c)
        up(row_errors(row_f32(c, inp), row_ref(c, inp)))
    for c in STATS:
        inp = stats_inputs(c)
        up(stats_errors(c, stats_f32(c, inp), stats_ref(c, inp)))
    for c in FREEMATCH:
        inp = freematch_inputs(c)
        for g, r in zip(freematch_f32(c, inp), freematch_ref(c, inp)):
            up(freematch_errors(c, g, r))
    for c in ENTROPY:
        inp = entropy_inputs(c)
        if c["sel"] == "none":
            continue
        ref = entropy_ref(c, inp)
        loss, grad = entropy_autograd(c, inp, torch.float32)
        out = grad if inp["d0"] is None else (inp["d0"] + grad.astype(F32)).astype(F32)
        up(entropy_errors(loss, out, ref))
    for c in DISTALIGN:
        inp = distalign_inputs(c)
        for g, r in zip(distalign_f32(c, inp), distalign_ref(c, inp)):
            up(distalign_errors(c, g, r))
    for c in SOFTMATCH:
        inp = softmatch_inputs(c)
        for g, r in zip(softmatch_f32(c, inp), softmatch_ref(c, inp)):
            up(softmatch_errors(g, r))
    for c in MASKED_CE:
        inp = ce_inputs(c)
        up(ce_errors(c, ce_f32(c, inp), ce_ref(c, inp)))
    for c in REWARD:
        inp = reward_inputs(c)
        if inp["mean_in"] is None:
            up(reward_errors(reward_f32(c, inp), reward_ref(c, inp)))
    return fl


# ==== discrete outputs: which rows are decided, and problems of a 0 / 1 or argmax output ====================================================
def check_discrete(what, got, ref, near, n_rows=None):
    """Problems (strings) of a mask / label vector ``got`` against ``ref`` where ``near`` marks the rows that may fall on either side."""
    got, ref, near = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(near, bool)
    bad = []
    if near.sum() > NEAR_SHARE * (n_rows or got.size):
        bad.append("%s: %d rows within %g of their threshold" % (what, int(near.sum()), NEAR))
    diff = (got != ref) & ~near
    if diff.any():
        bad.append("%s: rows %s" % (what, np.nonzero(diff)[0].tolist()[:8]))
    return bad


def argmax_near(gap):
    """rows whose top two are a positive distance of at most NEAR apart (an exact tie has one answer: the first column)"""
    return (gap > 0) & (gap <= NEAR)


# ==== the wrong versions the committed bounds must reject (tests/test_cpu_score_filter_cases.py) ================================================
WRONG = {
    "stats": ("drop_last_row", "drop_rows_past_256"),
    "freematch": ("drop_last_row", "drop_rows_past_256", "floor_rank", "lerp_from_the_other_end", "rank_0.8n", "local_rows_only"),
    "entropy": ("hist_ignores_mask", "no_cross_term", "a_from_all_rows"),
    "distalign": ("first_call_is_an_ema_step", "p_target_not_updated", "mean_over_local_rows"),
    "softmatch": ("variance_over_n", "local_rows_only", "drop_last_row", "drop_rows_past_256"),
    "ce": ("mean_over_selected_rows",),
    "reward": ("ragged_over_full_group", "drop_last_row"),
}
