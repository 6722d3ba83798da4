"""``AlgorithmBase.score_unlabeled`` through the algorithms and backbone families: tiny nets, 40 unlabelled rows, ulb_dest_len 64, a few
training steps across start_timing first so that every piece of state is non-trivial.
  1. nothing is mutated: the whole checkpoint dictionary (parameters, optimizer, hook state, rewarder, RNG position), max_reward, ``it`` and
     the training flag carry the same bits before and after; the next training step equals that of a twin that never scored
  2. every column equals a recomputation from the public pieces, batch by batch, bit for bit: forward_features with training = False,
     ops.row_max (+ ops.distalign), the momentum-1 hook launch on a state copy, the Rewarder's forward on the same groups, ops.reward_mask2
  3. a batch size that does not divide 40 and a reward_group that does not divide the batch
  4. loader=None with device_data / device_tokens; ValueError without a device mode
  5. the launches per batch behind the backbone's forward
  6. save -> load; the example script as a fresh child process"""
import argparse
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _score_rows_cases as SC                                  # noqa: E402
from semireward_amd import _lib, ops                            # noqa: E402
from semireward_amd.algorithms import get_algorithm            # noqa: E402
from semireward_amd.algorithms import srflexmatch as SF        # noqa: E402
from semireward_amd.core import pl_table as PT                 # noqa: E402
from semireward_amd.core.pl_table import COLUMNS, PseudoLabelTable     # noqa: E402
from semireward_amd.nets import bert, hubert, vit, wrn         # noqa: E402
from semireward_amd.utils import synth                         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, BL, BU, N_ULB, N_ROWS, IMG, WAVE = 10, 4, 6, 64, 40, 8, 400
ITS = (1, 2, 3, 4)                     # start_timing 2: K = 0, 0, then two steps with data_generator passes (num_train_iter 24)
BATCH, GROUP = 16, 6                   # 40 = 16 + 16 + 8; 16 = 6 + 6 + 4, 8 = 6 + 2
BUILDERS = {"vit": vit.vit_tiny_test, "bert": bert.bert_tiny_test, "wrn": wrn.wrn_tiny_test, "hubert": hubert.hubert_tiny_test}
CONFIGS = [("srflexmatch", "vit"), ("srfixmatch", "vit"), ("srfreematch", "vit"), ("srsoftmatch", "vit"), ("srpseudolabel", "vit"),
           ("srsoftmatch", "bert"), ("srpseudolabel", "wrn"), ("srfreematch", "hubert")]
IDS = ["%s+%s" % c for c in CONFIGS]


def _args(algorithm, backbone, **kw):
    d = dict(algorithm=algorithm, num_classes=C, num_train_iter=24, epoch=1, ema_m=0.0, ulb_loss_ratio=1.0, use_cat=backbone in ("vit", "wrn"),
             amp=False, lr=5e-4, weight_decay=5e-4, layer_decay=0.5, num_warmup_iter=0, optim="AdamW", T=0.5, p_cutoff=0.12, hard_label=True,
             thresh_warmup=True, ulb_dest_len=N_ULB, N_k=10, start_timing=2, feature_dim=128, sr_lr=5e-4, sr_ema=False, sr_ema_m=0.99, gpu=0,
             rank=0, world_size=1, distributed=False, unsup_warm_up=0.4, ema_p=0.5, use_quantile=False, clip_thresh=False, ent_loss_ratio=0.01,
             n_sigma=2, dist_uniform=True, dist_align=True, per_class=False, batch_size=BL, uratio=2, eval_batch_size=BATCH)
    if backbone == "wrn":
        d.update(optim="SGD", lr=0.03, momentum=0.9, weight_decay=1e-3, layer_decay=1.0)
    d.update(kw)
    return argparse.Namespace(**d)


def _tokens(g, rows, L):
    ids = torch.randint(1, 120, (rows, L), generator=g)
    am = torch.ones(rows, L, dtype=torch.int64)
    am[0, L - 3:] = 0                                           # a padded row
    return {"input_ids": ids * am, "attention_mask": am}


def _train_batch(backbone, n):
    b = {k: torch.from_numpy(v) for k, v in synth.synth_batch(900 + n, BL, BU, IMG, C, N_ULB).items()}
    g = torch.Generator().manual_seed(400 + n)
    if backbone == "bert":
        b.update(x_lb=_tokens(g, BL, 12 + n), x_ulb_w=_tokens(g, BU, 15), x_ulb_s=_tokens(g, BU, 10 + 2 * n))
    elif backbone == "hubert":
        b.update({k: 0.1 * torch.randn(r, WAVE, generator=g) for k, r in (("x_lb", BL), ("x_ulb_w", BU), ("x_ulb_s", BU))})
    return b


def _score_batches(backbone, style="eval", batch=BATCH):
    """The 40 unlabelled rows as a loader hands them over (CPU tensors): evaluation style {'x_lb'} in index order, or training style
    {'x_ulb_w', 'idx_ulb'} with the rows at shuffled positions of the 64-entry table."""
    g = torch.Generator().manual_seed(5150)
    perm = torch.randperm(N_ULB, generator=g)[:N_ROWS]
    out = []
    for s in range(0, N_ROWS, batch):
        r = min(batch, N_ROWS - s)
        if backbone == "bert":
            x = _tokens(g, r, 9 + s // 4)
        elif backbone == "hubert":
            x = 0.1 * torch.randn(r, WAVE, generator=g)
        else:
            x = torch.randn(r, 3, IMG, IMG, generator=g)
        out.append({"x_lb": x} if style == "eval" else {"x_ulb_w": x, "idx_ulb": perm[s:s + r]})
    return out


def _trained(algorithm, backbone, **kw):
    alg = get_algorithm(_args(algorithm, backbone, **kw), BUILDERS[backbone])
    for n, it in enumerate(ITS):
        _step(alg, backbone, n, it)
    torch.cuda.synchronize()
    ops.check_label_errors()
    return alg


def _step(alg, backbone, n, it, trace=False):
    alg.model.train()
    alg.it = it
    alg.optimizer.sched_step = it
    alg.trace = {} if trace else None
    alg.out_dict, alg.log_dict = alg.train_step(**alg.process_batch(**_train_batch(backbone, n)))
    alg.call_hook("after_train_step")
    return alg.trace


def _flat(d, prefix=""):
    """A nested checkpoint dictionary as {path: bytes or value}."""
    out = {}
    if isinstance(d, dict):
        for k, v in d.items():
            out.update(_flat(v, "%s/%s" % (prefix, k)))
    elif isinstance(d, (list, tuple)):
        for i, v in enumerate(d):
            out.update(_flat(v, "%s/%d" % (prefix, i)))
    elif torch.is_tensor(d):
        out[prefix] = d.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes() if d.numel() else b""
    elif isinstance(d, np.ndarray):
        out[prefix] = d.tobytes()
    else:
        out[prefix] = d
    return out


def _snapshot(alg):
    """Every piece of state the scoring pass must leave alone."""
    s = _flat(alg.get_save_dict())
    h = alg.hooks_dict["MaskingHook"]
    for name in ("selected_label", "classwise_acc", "hist", "time_p", "p_model", "label_hist", "mu_var"):
        if hasattr(h, name):
            s["hook/" + name] = _flat(getattr(h, name))[""]
    da = alg.hooks_dict.get("DistAlignHook")
    if da is not None:
        s.update({"da/" + k: _flat(getattr(da, k))[""] for k in ("p_model", "p_target", "inited")})
    s.update(max_reward=_flat(alg.max_reward)[""], it=alg.it, training=alg.model.training, draws=getattr(alg.model, "_rng_calls", None),
             rewarder=_flat(alg.rewarder.flat)[""], rewarder_t=_flat(alg.rewarder.flat_t)[""], rewarder_grad=_flat(alg.rewarder.grad)[""],
             rewarder_training=alg.rewarder.training, flat=_flat(alg.model.flat)[""])
    return s


def _copy_state(dst, src):
    buf = io.BytesIO()
    torch.save(src.get_save_dict(), buf)
    buf.seek(0)
    dst.load_model(buf)
    assert torch.equal(dst.model.flat, src.model.flat) and torch.equal(dst.rewarder.flat, src.rewarder.flat)


def _recompute(alg, backbone, batches, group):
    """The table from the public pieces, batch by batch."""
    mode, kw, st = PT.score_rule(alg)
    net, rw = alg.model, alg.rewarder
    cols = {k: np.zeros(N_ULB, SC.TABLE_DTYPES[k]) for k in SC.TABLE}
    cols["label"][:] = -1
    cols["margin"], cols["entropy"] = np.zeros(N_ULB), np.zeros(N_ULB)          # float64: compared within the kernel test's bounds
    was, net.training = net.training, False
    seen = 0
    try:
        for data in batches:
            x, idx = PT._batch_rows(alg, data)
            lg, feat, _ = net.forward_features(x, None, None, save=False)
            lg, feat = lg.clone().contiguous(), feat.float().clone().contiguous()
            B = lg.shape[0]
            mp, mi, w = SC.training_launches(lg, mode, st, kw.get("p_cutoff", 0.0), kw.get("n_sigma", 0))
            probs = torch.softmax(lg.double(), dim=-1)
            if mode == "soft" and int(st["da_inited"]) != 0:
                q = probs * (st["da_p_target"].double() + SC.EPS_DA) / (st["da_p_model"].double() + SC.EPS_DA)
                probs = q / q.sum(dim=-1, keepdim=True)
            reward, keep = torch.empty(B, device=lg.device), torch.empty(B, device=lg.device)
            for s in range(0, B, group):                                       # the Rewarder's forward and the reward filter group by group
                e = min(s + group, B)
                reward[s:e] = rw.score(feat[s:e].contiguous(), mi[s:e].contiguous())
                m2 = torch.empty(e - s, device=lg.device)
                ops.reward_mask2(reward[s:e].contiguous(), m2, None, 1, e - s)
                keep[s:e] = m2
            j = (idx if idx is not None else torch.arange(seen, seen + B, device=lg.device)).cpu().numpy()
            h = lambda t: t.cpu().numpy()                                       # noqa: E731
            cols["label"][j], cols["conf"][j], cols["weight"][j], cols["reward"][j] = h(mi), h(mp), h(w), h(reward)
            cols["reward_keep"][j] = h(keep) > 0
            cols["selected"][j] = (h(w) > 0) & (h(keep) > 0)
            cols["count"][j] += 1
            top2 = torch.topk(probs, 2, dim=-1).values
            cols["margin"][j] = h(top2[:, 0] - top2[:, 1])                      # float64 values: compared within the kernel test's bounds
            cols["entropy"][j] = h(torch.special.entr(probs).sum(dim=-1))
            seen += B
    finally:
        net.training = was
    return cols


@pytest.mark.parametrize("algorithm,backbone", CONFIGS, ids=IDS)
def test_scoring_mutates_nothing_and_equals_the_public_pieces(algorithm, backbone, monkeypatch, tmp_path):
    monkeypatch.setattr(SF, "_DEFER_AUTOTUNE", False)
    alg = _trained(algorithm, backbone)
    twin = get_algorithm(_args(algorithm, backbone), BUILDERS[backbone])
    _copy_state(twin, alg)
    style = "train" if algorithm in ("srflexmatch", "srsoftmatch") else "eval"
    batches = _score_batches(backbone, style)
    before = _snapshot(alg)
    table = alg.score_unlabeled(loader=batches, reward_group=GROUP)
    got = table.read()
    after = _snapshot(alg)
    assert sorted(before) == sorted(after)
    changed = [k for k in before if before[k] != after[k]]
    assert not changed, changed                                                 # 1. nothing the pass may not touch carries other bits
    # 2. + 3. the columns, from the public pieces (batches of 16, 16, 8 rows; reward groups of 6, 6, 4 and 6, 2 rows)
    want = _recompute(alg, backbone, batches, GROUP)
    assert _snapshot(alg) == before
    for k in ("label", "conf", "weight", "reward", "reward_keep", "selected", "count"):
        assert got[k].tobytes() == want[k].astype(SC.TABLE_DTYPES[k]).tobytes(), k
    scored = got["count"] > 0
    assert scored.sum() == N_ROWS and (got["count"][scored] == 1).all() and (got["label"][~scored] == -1).all()
    assert (got["conf"][~scored] == 0).all() and (got["selected"][~scored] == 0).all()
    assert np.abs(got["margin"].astype(np.float64) - want["margin"])[scored].max() <= SC.margin_bound(C)
    assert np.abs(got["entropy"].astype(np.float64) - want["entropy"])[scored].max() <= SC.entropy_bound(C)
    assert got["reward_keep"][scored].sum() > 0 and np.isfinite(got["reward"]).all()      # a group's largest reward reaches its mean
    assert table.meta["algorithm"] == algorithm and table.meta["it"] == alg.it and table.meta["reward_group"] == GROUP
    # 6. save -> load
    back = PseudoLabelTable.load(table.save(str(tmp_path / "t.npz"))).read()
    assert all(back[k].tobytes() == got[k].tobytes() for k in COLUMNS)
    # 1. the next training step equals that of the twin that never scored
    ta, tb = _step(alg, backbone, 4, 5, trace=True), _step(twin, backbone, 4, 5, trace=True)
    torch.cuda.synchronize()
    for k in ("masks", "pseudo", "mask2"):
        a, b = ta[k], tb[k]
        a, b = (torch.cat(list(a)), torch.cat(list(b))) if isinstance(a, (list, tuple)) else (a, b)
        assert (a is None and b is None) or torch.equal(a, b), k
    pa, pb = alg.model.flat.double(), twin.model.flat.double()                  # parameters: the bound of tests/test_gpu_resume.py
    assert float((pa - pb).norm()) / (float(pa.norm()) + 1e-30) <= 1e-6
    ops.check_label_errors()


def test_eval_and_train_style_batches_fill_the_same_rows():
    alg = _trained("srfixmatch", "vit")
    ev = alg.score_unlabeled(loader=_score_batches("vit", "eval"), reward_group=GROUP).read()
    tr = alg.score_unlabeled(loader=_score_batches("vit", "train"), reward_group=GROUP).read()
    perm = _score_batches("vit", "train")
    idx = torch.cat([b["idx_ulb"] for b in perm]).numpy()
    for k in COLUMNS:                                                           # arrival order against idx_ulb: the same rows, other places
        assert ev[k][:N_ROWS].tobytes() == tr[k][idx].tobytes(), k
    # another batch size regroups the rewards, and only them
    b8 = alg.score_unlabeled(loader=_score_batches("vit", "eval", batch=7), reward_group=GROUP).read()
    for k in ("label", "conf", "margin", "entropy", "weight"):
        assert b8[k].tobytes() == ev[k].tobytes(), k
    # too many rows for the table: skipped, reported at the read
    alg.args.ulb_dest_len = 32
    t = alg.score_unlabeled(loader=_score_batches("vit", "eval"), reward_group=GROUP)
    with pytest.raises(IndexError, match="pseudo-label table"):
        t.read()
    alg.args.ulb_dest_len = N_ULB
    ops.check_label_errors()


def _images(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(0, 256, size=(n, IMG, IMG, 3)).astype(np.uint8), rng.integers(0, C, size=n).astype(np.int64)


def test_loader_none_builds_the_device_mode_loader(monkeypatch):
    monkeypatch.setattr(SF, "_DEFER_AUTOTUNE", False)
    (xl, yl), (xu, _), (xe, ye) = _images(8, 1), _images(N_ROWS, 2), _images(6, 3)
    dd = {"train_lb": {"data": xl, "targets": yl}, "train_ulb": {"data": xu, "targets": None}, "eval": {"data": xe, "targets": ye}}
    alg = get_algorithm(_args("srfixmatch", "vit", device_data=True, dataset_dict=dd, dataset="cifar100", img_size=IMG, crop_ratio=0.875,
                              train_sampler="RandomSampler", seed=0, ulb_dest_len=None), vit.vit_tiny_test)
    assert alg.args.ulb_dest_len == N_ROWS and alg.dataset_dict["train_ulb"].targets is None
    t = alg.score_unlabeled(batch_size=12)                                       # 40 = 12 + 12 + 12 + 4; reward groups of batch_size * uratio = 8
    got = t.read()
    assert (got["count"] == 1).all() and t.meta["reward_group"] == BL * 2 and alg.dataset_dict["train_ulb"].targets is None
    loader = PT.unlabelled_eval_loader(alg, 12)
    host = [{"x_lb": b["x_lb"].cpu()} for b in loader]                           # the same unaugmented views handed in as batches
    assert [b["x_lb"].shape[0] for b in host] == [12, 12, 12, 4]
    same = alg.score_unlabeled(loader=host).read()
    assert all(same[k].tobytes() == got[k].tobytes() for k in COLUMNS)
    s = t.summary(np.arange(N_ROWS) % C)
    assert s["rows"] == N_ROWS and 0 <= s["selected_ratio"] <= 1 and s["selected_by_class"].sum() == s["selected"] and 0 <= s["acc_all"] <= 1
    plain = get_algorithm(_args("srfixmatch", "vit"), vit.vit_tiny_test)
    with pytest.raises(ValueError, match="loader"):
        plain.score_unlabeled()
    ops.check_label_errors()


def test_loader_none_with_device_tokens(monkeypatch):
    monkeypatch.setattr(SF, "_DEFER_AUTOTUNE", False)
    rng = np.random.Generator(np.random.PCG64(11))
    rows = lambda n: [rng.integers(1, 120, size=int(rng.integers(4, 15))).astype(np.int32) for _ in range(n)]      # noqa: E731
    dd = {"train_lb": {"data": rows(8), "targets": rng.integers(0, C, size=8)},
          "train_ulb": {"data": rows(N_ROWS), "targets": None, "data_s": [rows(N_ROWS), rows(N_ROWS)]},
          "eval": {"data": rows(6), "targets": rng.integers(0, C, size=6)}}
    alg = get_algorithm(_args("srsoftmatch", "bert", device_tokens=True, dataset_dict=dd, dataset="aclImdb", max_length=16,
                              train_sampler="RandomSampler", seed=7, ulb_dest_len=None), bert.bert_tiny_test)
    for n, (lb, ulb) in enumerate(zip(alg.loader_dict["train_lb"], alg.loader_dict["train_ulb"])):      # four steps through the token loaders
        if n == 4:
            break
        alg.it = n + 1
        alg.optimizer.sched_step = n + 1
        alg.train_step(**alg.process_batch(**lb, **ulb))
    before = _snapshot(alg)
    t = alg.score_unlabeled(batch_size=16, reward_group=GROUP)
    got = t.read()
    assert _snapshot(alg) == before and (got["count"] == 1).all()
    host = [{"x_lb": {k: v.cpu() for k, v in b["x_lb"].as_dict().items()}} for b in PT.unlabelled_eval_loader(alg, 16)]
    same = alg.score_unlabeled(loader=host, reward_group=GROUP).read()          # token dicts, as evaluate() takes them
    assert all(same[k].tobytes() == got[k].tobytes() for k in COLUMNS)
    ops.check_label_errors()


def test_launches_per_batch(monkeypatch):
    """Behind the backbone's forward a batch is: one score_rows, the Rewarder's forward (whole groups, + the ragged last group), one
    reward_mask2, one score_commit -- counted by entry point (ops._call) and by the library's own launch counter; no allocation after the
    first batch between the first and the last of them."""
    alg = _trained("srflexmatch", "vit")
    batches = _score_batches("vit", "train")
    alg.score_unlabeled(loader=batches, reward_group=GROUP)                      # workspaces of every group shape exist from here on
    lib = _lib.lib()
    names, counts, allocs, real_call = [], [], [], ops._call

    def call(name, *a):
        if name == "srhip_score_rows":
            names.append([])
            counts.append(lib.srhip_prof_count())
            allocs.append(torch.cuda.memory_stats()["allocation.all.allocated"])
        if names:
            names[-1].append(name)
        real_call(name, *a)
        if name == "srhip_score_commit":
            counts[-1] = lib.srhip_prof_count() - counts[-1]
            allocs[-1] = torch.cuda.memory_stats()["allocation.all.allocated"] - allocs[-1]

    monkeypatch.setattr(ops, "_call", call)
    lib.srhip_prof_enable(1)
    try:
        alg.score_unlabeled(loader=batches, reward_group=GROUP)
        torch.cuda.synchronize()
        # what one Rewarder forward launches at these group shapes, by the same counter
        n0 = lib.srhip_prof_count()
        rw = alg.rewarder
        rw.score(torch.zeros(GROUP, rw.feature_dim, device=alg.device), torch.zeros(GROUP, dtype=torch.int64, device=alg.device))
        per_fwd = lib.srhip_prof_count() - n0
    finally:
        lib.srhip_prof_enable(0)
        monkeypatch.setattr(ops, "_call", real_call)
    tails = [[n for n in seq[:seq.index("srhip_score_commit") + 1]] for seq in names]
    want = ["srhip_score_rows", "srhip_rewarder_fwd", "srhip_rewarder_fwd", "srhip_reward_mask2_ragged", "srhip_score_commit"]
    assert tails == [want, want, want], tails                                   # 16 = 6 + 6 | 4, 16, 8 = 6 | 2
    assert per_fwd >= 1 and counts == [3 + 2 * per_fwd] * 3, (counts, per_fwd)
    assert allocs == [0, 0, 0], allocs
    # whole groups only: one Rewarder call, the plain reward_mask2
    names.clear()
    monkeypatch.setattr(ops, "_call", lambda name, *a: (names.append(name), real_call(name, *a))[1])
    alg.score_unlabeled(loader=_score_batches("vit", "eval", batch=8), reward_group=4)
    monkeypatch.setattr(ops, "_call", real_call)
    i = names.index("srhip_score_rows")
    assert names[i:i + 4] == ["srhip_score_rows", "srhip_rewarder_fwd", "srhip_reward_mask2", "srhip_score_commit"]
    torch.cuda.synchronize()
    ops.check_label_errors()


def test_example_runs_as_a_child_process(tmp_path):
    out = str(tmp_path / "pl.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "export_pseudo_labels.py"), "--steps", "24", "--out", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    t = PseudoLabelTable.load(out)
    c = t.read()
    assert (c["count"] == 1).all() and t.meta["algorithm"] == "srflexmatch" and "classwise_acc" in t.meta["state"]
    assert "selected" in r.stdout and "acc_selected" in r.stdout
