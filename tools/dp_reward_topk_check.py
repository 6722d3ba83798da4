"""Run with 2 ranks on one GPU (gloo):  SR_DIST_BACKEND=gloo python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1
--master-port 29535 tools/dp_reward_topk_check.py.  One SRFlexMatch step per rank (its own shard of the unlabeled stream) through the HIP
engine with ``reward_filter: topk`` (reward_topk 2) and ``global_reward_threshold`` on and off:
  on : mask2 of every pass == the top-k rule over BOTH ranks' rewards of that pass (candidate index rank * nu + row), k * 2 rows kept together;
  off: mask2 == the rule over the rank's own rewards, k rows each -- per rank, as the mean rule under the reference's DDP."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
import torch.distributed as dist
import bench
import _reward_filter_cases as RF
from semireward_amd.algorithms import get_algorithm
from semireward_amd.nets import vit
from semireward_amd.utils import synth

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group(os.environ.get("SR_DIST_BACKEND", "gloo"), rank=rank, world_size=world)
NSt = dict(bench.NS, num_classes=10, ulb_dest_len=256, feature_dim=128, num_train_iter=2000, start_timing=100, num_warmup_iter=0)
TOPK = 2
for flag in (True, False):
    args = argparse.Namespace(gpu=0, rank=rank, world_size=world, distributed=True, global_reward_threshold=flag, reward_filter="topk",
                              reward_topk=TOPK, **NSt)
    alg = get_algorithm(args, vit.vit_tiny_test)
    alg.model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_params(alg.model.names_shapes, 0).items()})
    alg.dp.broadcast_params(alg.model, alg.rewarder, alg.generator)
    assert alg.dp.active and alg.dp.global_reward_threshold == flag and alg.reward_filter.kind == "topk"
    alg.model.seed = 77 + rank
    b = synth.synth_batch(500 + rank, 4, 4, 8, 10, 256)                 # each rank its own shard
    alg.it = 250                                                        # K = sr_decay() = 9
    alg.optimizer.sched_step = alg.it
    alg.trace = {}
    alg.out_dict, alg.log_dict = alg.train_step(**alg.process_batch(**{k: torch.from_numpy(v) for k, v in b.items()}))
    alg.call_hook("after_train_step")                                   # gradient all-reduce + optimizer: the step completes on both ranks
    torch.cuda.synchronize()
    K, nu = alg.trace["K"], 4
    r = alg.trace["reward"].float().cpu().view(-1)
    m2 = alg.trace["mask2"].cpu().view(-1)
    both_r, both_m = [torch.empty_like(r) for _ in range(world)], [torch.empty_like(m2) for _ in range(world)]
    dist.all_gather(both_r, r)
    dist.all_gather(both_m, m2)
    peers = np.stack([x.numpy() for x in both_r])
    if flag:
        want = RF.topk_groups(peers[rank], K, nu, TOPK * world, peers=peers, self_peer=rank)
    else:
        want = RF.topk_groups(peers[rank], K, nu, TOPK)
    ok = bool(np.array_equal(m2.numpy(), want))
    kept = np.stack([x.numpy() for x in both_m]).reshape(world, K, nu).sum(axis=(0, 2))
    other = RF.topk_groups(peers[rank], K, nu, TOPK) if flag else RF.topk_groups(peers[rank], K, nu, TOPK * world, peers=peers, self_peer=rank)
    print("rank %d: global_reward_threshold=%s K=%d mask2 == the rule: %s (the other form would give a different mask: %s)" % (
        rank, flag, K, ok, bool((want != other).any())), flush=True)
    assert ok, (m2.numpy().reshape(K, nu), want.reshape(K, nu))
    assert (kept == TOPK * world).all(), kept
    print("rank %d: kept per pass over both ranks: %d" % (rank, int(kept[0])), flush=True)
    params = alg.model.flat.clone()
    other_p = params.clone()
    dist.broadcast(other_p, src=0)
    assert torch.equal(other_p, params), "ranks diverged after the step"
dist.destroy_process_group()
