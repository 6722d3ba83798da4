"""The opt-in reward filter without a GPU: the yaml keys and their refusals, the ratio -> k arithmetic, every SR_EINVAL of
srhip_reward_topk_mask, the numpy rule of tests/_reward_filter_cases.py against its second statement, the checker against planted faults,
and DataParallel.gather_rewards on two gloo ranks."""
import argparse
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _reward_filter_cases as RF
from semireward_amd.algorithms.reward_filter import MAX_CANDIDATES, RewardFilter, read_reward_filter

F32 = np.float32


def NS(**kw):
    return argparse.Namespace(**kw)


# ---- parser ---------------------------------------------------------------------------------------------------------------------------
def test_absent_key_and_mean_are_the_reference_rule():
    for a in (NS(), NS(reward_filter=None), NS(reward_filter="mean"), NS(reward_filter=" Mean ")):
        f = read_reward_filter(a)
        assert (f.kind, f.topk, f.ratio_ppm, f.threshold) == ("mean", None, None, None)
        assert f.meta(8) == dict(reward_filter="mean")


def test_accepted_settings():
    f = read_reward_filter(NS(reward_filter="topk", reward_topk=2))
    assert (f.kind, f.topk, f.ratio_ppm) == ("topk", 2, None) and f.k_for(8) == 2 and f.k_for(8, world=2) == 4 and f.k_for(1) == 2
    assert f.meta(8) == dict(reward_filter="topk", k=2)
    f = read_reward_filter(NS(reward_filter="topk", reward_keep_ratio=0.25))
    assert (f.kind, f.topk, f.ratio_ppm) == ("topk", None, 250000) and f.meta(8) == dict(reward_filter="topk", k=2, reward_keep_ratio=0.25)
    f = read_reward_filter(NS(reward_filter="topk", reward_keep_ratio=1))
    assert f.ratio_ppm == 1000000
    f = read_reward_filter(NS(reward_filter="fixed", reward_threshold=0.6))
    assert (f.kind, f.threshold) == ("fixed", 0.6) and f.meta(8) == dict(reward_filter="fixed", reward_threshold=0.6)
    assert read_reward_filter(NS(reward_filter="fixed", reward_threshold=-3)).threshold == -3.0


@pytest.mark.parametrize("kw, key", [
    (dict(reward_filter="median"), "reward_filter"),                                              # an unknown filter
    (dict(reward_filter=3), "reward_filter"),
    (dict(reward_filter="topk"), "reward_topk"),                                                  # topk without either
    (dict(reward_filter="topk", reward_topk=2, reward_keep_ratio=0.5), "reward_keep_ratio"),      # ... with both
    (dict(reward_filter="fixed"), "reward_threshold"),                                            # fixed without its threshold
    (dict(reward_topk=2), "reward_topk"),                                                         # a key of another filter
    (dict(reward_filter="mean", reward_keep_ratio=0.5), "reward_keep_ratio"),
    (dict(reward_filter="mean", reward_threshold=0.5), "reward_threshold"),
    (dict(reward_filter="topk", reward_topk=2, reward_threshold=0.5), "reward_threshold"),
    (dict(reward_filter="fixed", reward_threshold=0.5, reward_topk=2), "reward_topk"),
    (dict(reward_filter="fixed", reward_threshold=0.5, reward_keep_ratio=0.5), "reward_keep_ratio"),
    (dict(reward_filter="topk", reward_topk=0), "reward_topk"),                                   # out of range
    (dict(reward_filter="topk", reward_topk=-1), "reward_topk"),
    (dict(reward_filter="topk", reward_topk=2.0), "reward_topk"),
    (dict(reward_filter="topk", reward_topk=True), "reward_topk"),
    (dict(reward_filter="topk", reward_topk="2"), "reward_topk"),
    (dict(reward_filter="topk", reward_topk=2 ** 31), "reward_topk"),
    (dict(reward_filter="topk", reward_keep_ratio=0.0), "reward_keep_ratio"),
    (dict(reward_filter="topk", reward_keep_ratio=-0.1), "reward_keep_ratio"),
    (dict(reward_filter="topk", reward_keep_ratio=1.000001), "reward_keep_ratio"),
    (dict(reward_filter="topk", reward_keep_ratio=float("nan")), "reward_keep_ratio"),
    (dict(reward_filter="topk", reward_keep_ratio=4e-7), "reward_keep_ratio"),                    # rounds to 0 at 1e-6
    (dict(reward_filter="topk", reward_keep_ratio="0.5"), "reward_keep_ratio"),
    (dict(reward_filter="fixed", reward_threshold=float("inf")), "reward_threshold"),
    (dict(reward_filter="fixed", reward_threshold=float("nan")), "reward_threshold"),
    (dict(reward_filter="fixed", reward_threshold="0.5"), "reward_threshold"),
])
def test_refusals_name_the_key(kw, key):
    with pytest.raises(ValueError, match=key):
        read_reward_filter(NS(**kw))


def test_validation_happens_at_construction_before_any_device_work():
    """SRConsistencyBase.__init__ parses the keys first: a bad setting raises although nothing else of ``args`` exists and no GPU is there."""
    from semireward_amd.algorithms.srflexmatch import SRFlexMatch
    from semireward_amd.algorithms.srpseudolabel import SRPseudoLabel
    for cls in (SRFlexMatch, SRPseudoLabel):
        with pytest.raises(ValueError, match="reward_threshold"):
            cls(NS(reward_filter="fixed"), None)


def test_no_key_is_a_get_argument_entry():
    from semireward_amd.algorithms import srflexmatch, srpseudolabel
    for cls in (srflexmatch.SRFlexMatch, srpseudolabel.SRPseudoLabel):
        names = {a.name for a in cls.get_argument()}
        assert not names & {"--reward_filter", "--reward_topk", "--reward_keep_ratio", "--reward_threshold"}


@pytest.mark.parametrize("ratio, rows, world, k", [
    (0.25, 8, 1, 2), (0.250001, 8, 1, 3), (0.249999, 8, 1, 2),
    (0.3, 10, 1, 3),                              # 0.3 * 10 = 3.0000000000000004 in binary floating point: the integer form says 3
    (0.300001, 10, 1, 4), (0.299999, 10, 1, 3),
    (1e-6, 448, 1, 1), (1e-6, 1, 1, 1),
    (1.0, 1, 1, 1), (1.0, 8, 1, 8), (1.0, 448, 1, 448), (1.0, 4097, 1, 4097), (0.999999, 448, 1, 448), (0.999999, 1000000, 1, 999999),
    (0.25, 8, 2, 4), (0.3, 5, 2, 3), (0.3, 5, 3, 5), (1.0, 448, 8, 3584), (0.125, 4, 1, 1), (0.125, 4, 3, 2),
])
def test_ratio_to_k_in_integer_arithmetic(ratio, rows, world, k):
    f = read_reward_filter(NS(reward_filter="topk", reward_keep_ratio=ratio))
    assert f.k_for(rows, world) == k == RF.ratio_k(ratio, rows, world)


def test_over_limit_configuration_is_a_value_error_naming_the_key():
    """More candidates per group than the kernel ranks: refused in Python before the call (no tensor is touched)."""
    f = RewardFilter("topk", topk=2)
    with pytest.raises(ValueError, match="reward_filter"):
        f.apply(None, None, 1, MAX_CANDIDATES + 1)
    peers = torch.empty(3, 0)
    with pytest.raises(ValueError, match="reward_filter"):
        f.apply(None, None, 1, MAX_CANDIDATES // 3 + 1, peers=peers)


# ---- the C ABI: argument errors before any launch -------------------------------------------------------------------------------------
def test_topk_entry_point_refuses_bad_arguments_without_launching():
    from semireward_amd import _lib
    lib = _lib.lib()
    a, E = 0x10000, -1                                                   # (never dereferenced)
    call = lib.srhip_reward_topk_mask
    assert call(None, a, 1, 8, 8, 2, 2, None, 0, 0, None) == E and call(a, None, 1, 8, 8, 2, 2, None, 0, 0, None) == E
    for groups, B, total in [(0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (2, 8, 8), (1, 8, 9), (2, 8, 17), (3, 8, 16)]:
        assert call(a, a, groups, B, total, 2, 2, None, 0, 0, None) == E, (groups, B, total)
    for k, k_last in [(0, 1), (1, 0), (-3, 2), (2, -1)]:
        assert call(a, a, 1, 8, 8, k, k_last, None, 0, 0, None) == E, (k, k_last)
    assert call(a, a, 1, 65537, 65537, 1, 1, None, 0, 0, None) == E                                  # B * n_peers <= 65536
    assert call(a, a, 1, 32769, 32769, 1, 1, a, 2, 0, None) == E
    assert call(a, a, 1 << 20, 1 << 11, 1 << 31, 1, 1, None, 0, 0, None) == E                        # groups * B < 2^31
    assert call(a, a, 32768, 65536, 2 ** 31 - 1, 1, 1, None, 0, 0, None) == E
    for n_peers, self_peer in [(0, 0), (2, 2), (2, -1), (-1, 0)]:
        assert call(a, a, 1, 8, 8, 2, 2, a, n_peers, self_peer, None) == E, (n_peers, self_peer)
    assert call(a, a, 1, 8, 8, 2, 2, None, 2, 0, None) == E and call(a, a, 1, 8, 8, 2, 2, None, 1, 1, None) == E   # no table: one peer, itself


# ---- the rule -------------------------------------------------------------------------------------------------------------------------
def test_the_two_statements_of_the_rule_agree():
    rng = np.random.Generator(np.random.PCG64(11))
    pool = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.5, 0.25], F32), RF.DENORM, -RF.DENORM,
                           np.array([0x7fc00001, 0xffc00000], np.uint32).view(F32)])
    for trial in range(2000):
        n = int(rng.integers(1, 40))
        r = pool[rng.integers(0, pool.size, size=n)] if trial % 2 else rng.standard_normal(n).astype(F32).round(1)
        k = int(rng.integers(1, n + 6))
        assert np.array_equal(RF.topk_mask(r, k), RF.topk_mask_by_rank(r, k)), (r, k)
    for (r, groups, B, k, k_last, total) in RF.checker_cases():
        a = RF.topk_groups(r, groups, B, k, k_last, total)
        b = RF.topk_groups(r, groups, B, k, k_last, total, one=RF.topk_mask_by_rank)
        assert np.array_equal(a, b)


def test_rule_properties_on_the_kernel_patterns():
    """min(k, non-NaN rows) rows are kept per group, never a NaN, never a row below a dropped one; both statements agree."""
    for groups, B, k in [(1, 1, 1), (3, 8, 2), (3, 65, 64), (9, 257, 262), (1, 448, 112)]:
        for name, r in RF.patterns(groups, B, k, seed=B).items():
            m = RF.topk_groups(r, groups, B, k)
            assert np.array_equal(m, RF.topk_groups(r, groups, B, k, one=RF.topk_mask_by_rank)), name
            for g in range(groups):
                rg, mg = r[g * B:(g + 1) * B], m[g * B:(g + 1) * B]
                assert mg.sum() == min(k, int((~np.isnan(rg)).sum())) and not mg[np.isnan(rg)].any(), (name, g)
                if 0 < mg.sum() < (~np.isnan(rg)).sum():
                    assert rg[mg > 0].min() >= np.nanmax(np.where(mg > 0, -np.inf, rg)), (name, g)
    dup = RF.patterns(1, 64, 10, seed=1)["dup_run"]
    assert (dup == np.sort(dup)[::-1][10]).sum() >= 4 and np.sort(dup)[::-1][9] == np.sort(dup)[::-1][10]      # the run straddles rank k


def test_peer_tables_rank_the_union():
    rng = np.random.Generator(np.random.PCG64(5))
    peers = rng.integers(0, 6, size=(3, 2 * 8)).astype(F32)
    peers[1, 3] = np.nan
    masks = [RF.topk_groups(peers[p], 2, 8, 5, peers=peers, self_peer=p) for p in range(3)]
    for g in range(2):
        cand = peers[:, g * 8:(g + 1) * 8].reshape(-1)
        assert np.array_equal(np.concatenate([m[g * 8:(g + 1) * 8] for m in masks]), RF.topk_mask(cand, 5))
        assert sum(m[g * 8:(g + 1) * 8].sum() for m in masks) == 5


def test_checker_accepts_the_rule_and_rejects_every_planted_fault():
    assert RF.agrees_with_rule(RF.topk_groups)
    assert RF.agrees_with_rule(lambda *a: RF.topk_groups(*a, one=RF.topk_mask_by_rank))
    assert len(RF.FAULTS) == 7
    for name, fault in RF.FAULTS.items():
        assert not RF.agrees_with_rule(fault), "not rejected: " + name


# ---- DataParallel.gather_rewards ------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from semireward_amd.distributed import DataParallel
    dp = DataParallel(world, rank, global_reward_threshold=True)
    assert dp.active
    rng = np.random.Generator(np.random.PCG64(3))
    r_all = torch.from_numpy(rng.random((world, 3 * 8)).astype(np.float32))          # [rank, K * nu]
    r_all[1, 5] = float("nan")
    table = dp.gather_rewards(r_all[rank].clone())
    ok = table.shape == (world, 24) and table.dtype == torch.float32 and table.is_contiguous()
    ok = ok and np.array_equal(table.numpy().view(np.uint32), r_all.numpy().view(np.uint32))        # bit for bit, in rank order
    q.put((rank, bool(ok)))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_rewards_world2_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=180) for _ in ps]
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(res) == [(0, True), (1, True)]


def test_gather_rewards_of_one_rank_is_its_own_row():
    from semireward_amd.distributed import DataParallel
    r = torch.arange(6, dtype=torch.float32)
    t = DataParallel(1, 0).gather_rewards(r)
    assert t.shape == (1, 6) and torch.equal(t[0], r)
