"""Seeded cases for srhip_score_rows / srhip_score_commit and a float64 numpy restatement of their semantics (include/srhip.h) from the
same fp32 logits.  The restatement shares no code with the kernels or with semireward_amd.core.pl_table
(``training_launches``, for the GPU tests, runs the launches of a training step to compare against).

The five columns of one batch, per row, from p = softmax(z) in float64 (or, SOFT with alignment and inited != 0, from
q = p (p_target + 1e-6) / (p_model + 1e-6) renormalised, hooks/dist_align.py:31-32):
  label    the first maximal column                          (hooks/pseudo_label.py:40)
  conf     the maximum
  margin   conf - the second largest value (0 for a tie at the top, conf for C == 1)
  entropy  -sum p ln p, 0 ln 0 = 0
  weight   FIXED  conf >= p_cutoff                                            masking.py:42-57
           FLEX   conf >= p_cutoff * acc[label] / (2 - acc[label])            srflexmatch/utils.py:50-56
           FREE   conf >= time_p * p_model[label] / max(p_model)              freematch/utils.py:24-66
           SOFT   exp(-clamp(conf - mu, max=0)^2 / (2 var / n_sigma^2))       srsoftmatch/utils.py:32-76
"""
import itertools

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24                                   # half an fp32 ulp of 1
NEAR = 1e-6                                      # rows this close to their threshold may fall on either side in fp32
NEAR_SHARE = 0.02                                # ... and at most this share of a case's rows may be that close
EPS_DA = F64(F32(1e-6))                          # the fp32 constant of dist_align.py:31 as the kernels hold it
MODES = ("fixed", "flex", "free", "soft", "soft_da0", "soft_da1")      # soft_da<i>: distribution alignment with inited == i
REG_COLS = 1024                                  # rows up to this length live in registers, longer ones are re-read (eval.hip's NIT * 256)
CS = (1, 2, 10, 100, REG_COLS, REG_COLS + 1)
BS = (1, 3, 8, 17, 65)                           # one wave of four in a workgroup; a partial workgroup; two; 4 + 1; 16 + 1
IDX_KINDS = ("perm", "offset", "oob")
COLUMNS = ("label", "conf", "margin", "entropy", "weight")
TABLE = COLUMNS + ("reward", "reward_keep", "selected", "count")
TABLE_DTYPES = dict(label=np.int64, conf=F32, margin=F32, entropy=F32, weight=F32, reward=F32, reward_keep=np.uint8, selected=np.uint8,
                    count=np.int32)


def margin_bound(C):
    """Sequential-sum, 2-ulp-expf and 1-ulp-division bound on a probability difference."""
    return 2.0 * (C + 8) * U


def entropy_bound(C):
    return 2.0 * (C + 8) * U * (1.0 + np.log(C))


def case_table():
    """(C, B, mode, pad, off, idx_kind): every C x B once, the mode / row pitch / base offset / index kind cycling at different periods, then
    every mode on both sides of the register / re-read switch with a padded pitch and an offset base."""
    out = []
    for i, (C, B) in enumerate(itertools.product(CS, BS)):
        out.append((C, B, MODES[i % 6], (0, 3)[(i // 2) % 2], (0, 1)[(i // 3) % 2], IDX_KINDS[i % 3]))
    for i, (mode, C) in enumerate(itertools.product(MODES, (100, REG_COLS, REG_COLS + 1))):
        out.append((C, (17, 65, 8)[i % 3], mode, 3, 1, IDX_KINDS[(i + 1) % 3]))
    return out


def case_id(spec):
    return "C%d-B%d-%s-pad%d-off%d-%s" % spec


def make_case(C, B, mode, pad, off, idx_kind, seed=0):
    rng = np.random.Generator(np.random.PCG64(1000003 * seed + 7919 * C + 104729 * B + 31 * MODES.index(mode) + 7 * pad + off))
    z = (rng.normal(size=(B, C)) * rng.uniform(0.2, 6.0, size=(B, 1))).astype(F32)
    # planted rows, from the last row backwards, row 0 stays an ordinary one
    plants = []
    if C >= 2:
        plants.append("tie_first_last")
    if C >= 3:
        plants += ["tie_three", "tie_second"]
    plants += ["onehot_pos", "onehot_neg", "all_equal"]
    planted = {}
    for k, name in enumerate(plants):
        r = B - 1 - k
        if r < 1:
            break
        planted[name] = r
        top = F32(np.abs(z[r]).max() + 1.0)
        if name == "tie_first_last":
            z[r, 0] = z[r, C - 1] = top
        elif name == "tie_three":
            z[r, 0] = z[r, C // 2] = z[r, C - 1] = top
        elif name == "tie_second":
            z[r, C // 2] = top
            z[r, 0] = z[r, C - 1] = top - F32(0.5)
        elif name == "onehot_pos":
            z[r] = F32(-80.0)
            z[r, (C - 1) // 2] = F32(80.0)
        elif name == "onehot_neg":
            z[r] = F32(80.0)
            if C >= 2:
                z[r, : C - 1] = F32(-80.0)
        else:
            z[r] = F32(rng.normal())
    ld = C + pad
    buf = np.full(off + B * ld + 5, np.nan, dtype=F32)           # NaN sentinels in front, in the row padding and behind
    for b in range(B):
        buf[off + b * ld: off + b * ld + C] = z[b]
    st = dict(p_cutoff=0.7, n_sigma=2)
    dirichlet = lambda: np.maximum(rng.dirichlet(np.full(C, 2.0)), 1e-4).astype(F32)      # noqa: E731
    if mode == "flex":
        acc = rng.random(C).astype(F32)
        acc[rng.random(C) < 0.1] = 0.0
        acc[rng.random(C) < 0.1] = 1.0
        st["classwise_acc"] = acc
    elif mode == "free":
        st["time_p"] = np.array([rng.uniform(0.3, 0.9)], F32)
        st["p_model"] = dirichlet()
    elif mode.startswith("soft"):
        st["mu_var"] = np.array([rng.uniform(0.3, 0.8), rng.uniform(0.01, 0.1)], F32)
        if mode != "soft":
            st["da_p_model"], st["da_p_target"] = dirichlet(), (np.full(C, 1.0 / C, F32) if seed % 2 == 0 else dirichlet())
            st["da_inited"] = np.array([int(mode[-1])], np.int32)
    # the commit: a table of n entries holding NaN / sentinel values, a reward and a reward filter per row, the index kind
    n = 2 * B + 3
    idx, row_offset = None, 0
    if idx_kind == "offset":
        row_offset = 2
    else:
        idx = rng.permutation(n)[:B].astype(np.int64)
        if idx_kind == "oob":
            idx[B // 2] = n if B % 2 else -1
    reward = rng.random(B).astype(F32)
    keep = (rng.random(B) < 0.6).astype(F32)
    return dict(C=C, B=B, mode=mode, ld=ld, off=off, buf=buf, logits=z, state=st, planted=planted, n=n, idx=idx, row_offset=row_offset,
                reward=reward, keep=keep, idx_kind=idx_kind)


def probabilities(case):
    """float64 probabilities the columns are taken from (aligned and renormalised in SOFT mode with inited != 0)."""
    z = case["logits"].astype(F64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    st = case["state"]
    if "da_inited" in st and int(st["da_inited"][0]) != 0:
        q = p * (st["da_p_target"].astype(F64) + EPS_DA) / (st["da_p_model"].astype(F64) + EPS_DA)          # dist_align.py:31
        p = q / q.sum(axis=1, keepdims=True)                                                                # :32
    return p


def restate_rows(case):
    """The five columns in float64 (label int64), plus 'near': the rows within NEAR of their 0 / 1 threshold, and 'soft_tol': the bound on
    the SOFT weight."""
    p = probabilities(case)
    B, C = p.shape
    st, mode = case["state"], case["mode"]
    label = p.argmax(axis=1).astype(np.int64)                                   # the first maximal column
    conf = p.max(axis=1)
    if C == 1:
        second = np.zeros(B)
    else:
        second = np.sort(p, axis=1)[:, -2]
    with np.errstate(divide="ignore", invalid="ignore"):
        plogp = np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)       # 0 ln 0 = 0
    out = dict(label=label, conf=conf, margin=conf - second, entropy=-plogp.sum(axis=1), soft_tol=0.0)
    pc = F64(F32(st["p_cutoff"]))
    thr = None
    if mode == "fixed":
        thr = np.full(B, pc)                                                    # masking.py:55
    elif mode == "flex":
        acc = st["classwise_acc"].astype(F64)[label]
        thr = pc * (acc / (2.0 - acc))                                          # srflexmatch/utils.py:53
    elif mode == "free":
        pm = st["p_model"].astype(F64)
        thr = F64(st["time_p"][0]) * (pm[label] / pm.max())                     # freematch/utils.py:63-64
    if thr is not None:
        out["weight"] = (conf >= thr).astype(F64)
        out["near"] = np.abs(conf - thr) <= NEAR
    else:
        mu, var = F64(st["mu_var"][0]), F64(st["mu_var"][1])
        den = 2.0 * var / st["n_sigma"] ** 2
        out["weight"] = np.exp(-(np.minimum(conf - mu, 0.0) ** 2) / den)        # srsoftmatch/utils.py:75
        out["near"] = np.zeros(B, bool)
        # |dw / dconf| <= sqrt(2 / (e den)) (the Gaussian's steepest slope) times the error of conf, plus the relative error of the
        # exponent (four roundings) and expf's 2 ulp on a value x e^-x <= 1 / e: 8 * 2^-24 covers them
        out["soft_tol"] = float(np.sqrt(2.0 / (np.e * den)) * margin_bound(C) + 8 * U)
    return out


def check_rows(case, ref, got):
    """Problems of the five columns ``got`` (arrays [B]) against the restatement ``ref``: a list of strings, empty when all is well."""
    C, B = case["C"], case["B"]
    bad = []
    g = {k: np.asarray(got[k]) for k in COLUMNS}
    # the label: exact ties at the top take the first column; otherwise the restated argmax wherever the top two are more than NEAR apart
    sure = (ref["margin"] == 0.0) | (ref["margin"] > NEAR)
    if not np.array_equal(g["label"][sure].astype(np.int64), ref["label"][sure]):
        bad.append("label: rows %s" % np.nonzero(sure & (g["label"].astype(np.int64) != ref["label"]))[0].tolist())
    for k, bound in (("conf", margin_bound(C)), ("margin", margin_bound(C)), ("entropy", entropy_bound(C))):
        v = g[k].astype(F64)
        if not np.isfinite(v).all():
            bad.append("%s: not finite in rows %s" % (k, np.nonzero(~np.isfinite(v))[0].tolist()))
            continue
        err = np.abs(v - ref[k])
        if (err > bound).any():
            bad.append("%s: error %.3e > %.3e in row %d" % (k, err.max(), bound, int(err.argmax())))
    tie = ref["margin"] == 0.0
    if C > 1 and (g["margin"][tie] != 0).any():
        bad.append("margin: not 0 for a tie at the top")
    w = g["weight"].astype(F64)
    if case["mode"].startswith("soft"):
        err = np.abs(w - ref["weight"])
        if not (err <= ref["soft_tol"]).all():
            bad.append("weight: error %.3e > %.3e" % (np.nanmax(err), ref["soft_tol"]))
    else:
        if ref["near"].sum() > NEAR_SHARE * B:
            bad.append("weight: %d rows of %d within %g of their threshold" % (ref["near"].sum(), B, NEAR))
        diff = (w != ref["weight"]) & ~ref["near"]
        if diff.any():
            bad.append("weight: rows %s" % np.nonzero(diff)[0].tolist())
    return bad


def max_errors(ref, got):
    return {k: float(np.abs(np.asarray(got[k]).astype(F64) - ref[k]).max()) for k in ("conf", "margin", "entropy")}


def sentinel_table(n, seed=0):
    """Table columns full of values a commit must leave alone where it does not write: label -1 / a sentinel, NaN floats, odd bytes."""
    rng = np.random.Generator(np.random.PCG64(77 + seed))
    t = {}
    for k, dt in TABLE_DTYPES.items():
        if dt is F32:
            t[k] = np.full(n, np.nan, F32)
        elif k == "label":
            t[k] = np.where(rng.random(n) < 0.5, -1, 0x5EED0000 + np.arange(n)).astype(np.int64)
        elif k == "count":
            t[k] = rng.integers(0, 3, size=n).astype(np.int32)
        else:
            t[k] = rng.integers(0, 256, size=n).astype(np.uint8)
    return t


def restate_commit(case, cols, table):
    """``table`` (dict of numpy columns, copied) after one commit of the batch columns ``cols``: (new table, out-of-range flag)."""
    t = {k: v.copy() for k, v in table.items()}
    n, B = case["n"], case["B"]
    flag = False
    for b in range(B):
        j = int(case["idx"][b]) if case["idx"] is not None else case["row_offset"] + b
        if j < 0 or j >= n:
            flag = True
            continue
        for k in COLUMNS:
            t[k][j] = cols[k][b]
        keep = case["keep"][b] > 0
        t["reward"][j] = case["reward"][b]
        t["reward_keep"][j] = 1 if keep else 0
        t["selected"][j] = 1 if (cols["weight"][b] > 0 and keep) else 0
        t["count"][j] += 1
    return t, flag


def tables_differ(got, want):
    """Names of the columns whose BITS differ (NaN sentinels compare by bit pattern)."""
    return [k for k in TABLE if np.asarray(got[k]).astype(TABLE_DTYPES[k]).tobytes() != np.asarray(want[k]).astype(TABLE_DTYPES[k]).tobytes()]


def training_launches(z, mode, st, p_cutoff, n_sigma):
    """(conf, label, weight) of dense device rows ``z`` [B, C] from the launches a TRAINING step uses, on copies of the threshold state
    ``st`` (device tensors under the names of ops.score_rows' arguments) with momentum 1, which leaves the state where it is:
    ops.row_max (aligned SOFT mode: + ops.distalign), then ops.fixed_mask / ops.flexmatch_mask (its mask precedes its update) /
    ops.freematch_update / ops.softmatch_mask.  mode: 'fixed' | 'flex' | 'free' | 'soft'."""
    import torch
    from semireward_amd import ops
    B, C = z.shape
    dv = z.device
    f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dv)      # noqa: E731
    probs, mp, mi, mask = f(B, C), f(B), torch.empty(B, dtype=torch.int64, device=dv), f(B)
    ops.row_max(z.contiguous(), False, probs, mp, mi, B, C)
    if mode == "soft" and st.get("da_inited") is not None and int(st["da_inited"]) != 0:
        pm, pt, inited = st["da_p_model"].clone(), st["da_p_target"].clone(), st["da_inited"].clone()
        ops.distalign(probs, torch.zeros(C, dtype=torch.float32, device=dv), B, None, 0, pm, pt, inited, 1.0, f(B, C), mp, mi, B, C)
        assert torch.equal(pm, st["da_p_model"]) and torch.equal(pt, st["da_p_target"]) and int(inited) == 1
    if mode == "fixed":
        ops.fixed_mask(mp, float(p_cutoff), mask, B)
    elif mode == "flex":
        n = 4 * B
        sel = torch.full((n,), -1, dtype=torch.int64, device=dv)
        hist = torch.zeros(C + 1, dtype=torch.int32, device=dv)
        ops.flexmatch_rebuild_hist(sel, hist, n, C)
        ops.flexmatch_mask(mp, mi, torch.arange(B, device=dv), float(p_cutoff), sel, hist, st["classwise_acc"].clone(), mask, B, C, n, True)
    elif mode == "free":
        tp, pm = st["time_p"].clone(), st["p_model"].clone()
        ops.freematch_update(mp, B, torch.zeros(C, dtype=torch.float32, device=dv), torch.ones(C, dtype=torch.float32, device=dv), mp, mi, tp, pm,
                             torch.ones(C, dtype=torch.float32, device=dv) / C, mask, B, C, 1.0, False, False)
        assert torch.equal(tp, st["time_p"]) and torch.equal(pm, st["p_model"])
    else:
        mv = st["mu_var"].clone()
        allp = mp if B >= 2 else torch.cat((mp, mp))                # torch.var of one value is nan: the EMA could not be frozen
        ops.softmatch_mask(allp.contiguous(), int(allp.numel()), mp, mv, 1.0, int(n_sigma), mask, B)
        assert torch.equal(mv, st["mu_var"])
    return mp, mi, mask
