"""The reward-filter rules in numpy (what tests/test_cpu_reward_filter.py and tests/test_gpu_reward_filter.py compare the library with), the
reward patterns the kernel is run on, and a short list of planted faults the comparison must reject.

topk, per independent group: order the rows non-NaN before NaN, larger reward first with -0 == +0, lower index first among equal rewards;
keep the first min(k, non-NaN rows).  A NaN reward is never kept."""
import numpy as np

F32 = np.float32
DENORM = np.array([1, 2, 0x7fffff], np.uint32).view(F32)          # the smallest two denormals and the largest one


def topk_mask(reward, k):
    """One group (1-D fp32) -> fp32 0/1 mask: np.lexsort((index, -reward, isnan))[:k], NaN rows dropped."""
    r = np.asarray(reward, F32)
    nan = np.isnan(r)
    val = np.where(nan, F32(0), r).astype(np.float64) + 0.0            # (-0) + 0 = +0; float64 holds every fp32 (denormals included) exactly
    order = np.lexsort((np.arange(r.size), -val, nan))
    mask = np.zeros(r.size, F32)
    mask[order[:max(int(k), 0)]] = 1.0
    mask[nan] = 0.0
    return mask


def ordered_key(reward):
    """The sign-flip map of the fp32 bits: unsigned order == float order; -0 canonicalised, NaN -> 0 (below -Inf, which maps to 0x007fffff)."""
    u = np.ascontiguousarray(reward, F32).view(np.uint32).copy()
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    u[u == np.uint32(0x80000000)] = 0
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key[nan] = 0
    return key


def topk_mask_by_rank(reward, k, index=None):
    """The second statement: rank(i) = #{j : c(j) > c(i)} on c = (ordered_key << 32) | (0xFFFFFFFF - index); kept iff rank < k and no NaN."""
    key = ordered_key(reward).astype(np.uint64)
    idx = np.arange(key.size, dtype=np.uint64) if index is None else np.asarray(index, np.uint64)
    c = (key << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx)
    rank = (c[None, :] > c[:, None]).sum(axis=1)
    return ((rank < k) & (key != 0)).astype(F32)


def group_rows(g, groups, B, total):
    return min(B, total - g * B)


def topk_groups(reward, groups, B, k, k_last=None, total=None, peers=None, self_peer=0, one=topk_mask):
    """The launch: ``total`` rows in groups of B (the last one ragged, with k_last), optional peer table [n_peers, groups * B] -> the mask of
    the caller's own rows; entries behind ``total`` are left at -1 (never written)."""
    total = groups * B if total is None else total
    k_last = k if k_last is None else k_last
    out = np.full(groups * B, -1.0, F32)
    for g in range(groups):
        n = group_rows(g, groups, B, total)
        kk = k_last if g == groups - 1 else k
        if peers is None:
            out[g * B:g * B + n] = one(reward[g * B:g * B + n], kk)
        else:
            cand = np.concatenate([p[g * B:g * B + n] for p in peers])       # candidate index peer * B + row: the same order
            out[g * B:g * B + n] = one(cand, kk)[self_peer * n:(self_peer + 1) * n]
    return out


def fixed_mask(reward, threshold):
    return (np.asarray(reward, F32) >= F32(threshold)).astype(F32)


def mean_mask(reward):
    """reward >= mean, the fp32 left-to-right mean of groups of up to 64 rows (csrc/score_filter.hip)."""
    s = F32(0)
    for v in np.asarray(reward, F32):
        s = F32(s + v)
    return (reward >= F32(s / F32(len(reward)))).astype(F32)


def ratio_k(ratio, rows, world=1):
    """k = ceil(ratio * rows * world) with the ratio resolved to 1e-6, in integers."""
    ppm = int(round(ratio * 1000000))
    return max(1, -(-(ppm * rows * world) // 1000000))


# ---- reward patterns ------------------------------------------------------------------------------------------------------------------
def patterns(groups, B, k, seed, slice_rows=256):
    """name -> fp32 [groups * B]: distinct rewards, all equal, a run of duplicates straddling rank k, +-0 / +-Inf / denormals among
    duplicates, NaN at the first and last row of every row slice."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = groups * B
    out = {}
    out["distinct"] = np.stack([rng.permutation(B) for _ in range(groups)]).astype(F32).reshape(n) * F32(0.25) - F32(B / 8)
    out["equal"] = np.full(n, 0.5, F32)
    d = np.empty((groups, B), F32)
    for g in range(groups):
        v = np.arange(B, 0, -1).astype(F32)                           # descending: rank r holds value B - r
        lo, hi = max(0, min(k, B) - 2), min(B, min(k, B) + 3)
        v[lo:hi] = v[lo]                                              # ranks lo .. hi - 1 tie, rank k in their middle
        d[g] = v[rng.permutation(B)]
    out["dup_run"] = d.reshape(n)
    pool = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 0.5], F32), DENORM, -DENORM])
    out["specials"] = pool[rng.integers(0, pool.size, size=n)]
    e = rng.standard_normal(n).astype(F32).reshape(groups, B)
    edge = sorted({i for s in range(0, B, slice_rows) for i in (s, min(s + slice_rows, B) - 1)})
    e[:, edge] = np.nan
    out["nan_edges"] = e.reshape(n)
    return out


# ---- planted faults: variants of topk_groups that a comparison with the rule must reject --------------------------------------------
def _fault_keeps_every_tie(r, k):            # non-strict: reward >= the k-th best
    m = topk_mask(r, k)
    if m.sum() == 0:
        return m
    kth = np.min(np.where(m > 0, np.where(r == 0, F32(0), r), np.inf))
    return ((r >= kth) & ~np.isnan(r)).astype(F32)


def _fault_drops_every_tie(r, k):            # strict: reward > the (k + 1)-th best
    m = topk_mask(r, k + 1)
    m1 = topk_mask(r, k)
    if m.sum() == m1.sum():
        return m1
    nxt = np.min(np.where(m > 0, r, np.inf))
    return ((r > nxt) & ~np.isnan(r)).astype(F32)


def _fault_tie_to_higher_index(r, k):
    return topk_mask(np.asarray(r, F32)[::-1], k)[::-1].copy()


def _fault_keeps_nan(r, k):
    r = np.asarray(r, F32)
    return topk_mask(np.where(np.isnan(r), F32(-np.inf), r), k)


def _fault_minus_zero_below_zero(r, k):      # the raw sign-flip key, -0 not canonicalised
    r = np.asarray(r, F32)
    u = r.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.int64)
    key[np.isnan(r)] = 0
    order = np.lexsort((np.arange(r.size), -key))
    m = np.zeros(r.size, F32)
    m[order[:k]] = 1.0
    m[np.isnan(r)] = 0.0
    return m


def _per_group(one):
    return lambda reward, groups, B, k, k_last=None, total=None: topk_groups(reward, groups, B, k, k_last, total, one=one)


def _fault_k_per_launch(reward, groups, B, k, k_last=None, total=None):
    total = groups * B if total is None else total
    out = np.full(groups * B, -1.0, F32)
    out[:total] = topk_mask(reward[:total], k)
    return out


def _fault_ragged_takes_k(reward, groups, B, k, k_last=None, total=None):
    return topk_groups(reward, groups, B, k, k, total)


FAULTS = {
    "every row tied with the k-th is kept": _per_group(_fault_keeps_every_tie),
    "every row tied with the k-th is dropped": _per_group(_fault_drops_every_tie),
    "a tie goes to the higher index": _per_group(_fault_tie_to_higher_index),
    "a NaN reward is kept": _per_group(_fault_keeps_nan),
    "-0 ranks below +0": _per_group(_fault_minus_zero_below_zero),
    "k is taken per launch, not per group": _fault_k_per_launch,
    "the ragged group takes k, not k_last": _fault_ragged_takes_k,
}


def checker_cases():
    """(reward, groups, B, k, k_last, total) the planted faults are run on: small, every clause of the rule decides at least one of them."""
    nan = np.nan
    return [
        (np.array([1, 2, 2, 2, 3, 0, 2, 1], F32), 1, 8, 3, None, None),                        # ties straddle rank k
        (np.array([0.0, -0.0, -1.0, -0.0, 0.0, -2.0], F32), 1, 6, 2, None, None),              # +-0 are one value, index decides
        (np.array([-0.0, 0.0, -1.0, 5.0], F32), 1, 4, 2, None, None),
        (np.array([nan, 1.0, nan, 0.5], F32), 1, 4, 3, None, None),                            # fewer numbers than k
        (np.array([nan, nan], F32), 1, 2, 1, None, None),
        (np.array([5, 4, 3, 2, 9, 8, 7, 6, 1, 1, 1, 1], F32), 3, 4, 2, None, None),            # three groups, k each
        (np.array([5, 4, 3, 2, 9, 8, 7, 6, 3, 1, 2, -1], F32), 3, 4, 3, 1, 11),                # ragged last group with its own k_last
        (np.array([np.inf, -np.inf, DENORM[0], -DENORM[0], 0.0, DENORM[1]], F32), 1, 6, 3, None, None),
    ]


def agrees_with_rule(launch):
    """The checker: ``launch(reward, groups, B, k, k_last, total)`` equals the rule on every case, entries behind ``total`` untouched."""
    for r, groups, B, k, k_last, total in checker_cases():
        buf = np.zeros(groups * B, F32)
        buf[:r.size] = r
        if not np.array_equal(launch(buf, groups, B, k, k_last, total), topk_groups(buf, groups, B, k, k_last, total)):
            return False
    return True
