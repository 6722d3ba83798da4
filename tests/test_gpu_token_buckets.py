"""The token engine over batches of many padded lengths, on the MI355X: the saved context and the output-gradient buffers as views of grow-only
arenas give the bits separate buffers give; memory stays bounded by the largest batch met; the filler rows of a joined / bucketed batch are
inert bit for bit; a bucketed batch computes the function of separate calls; ``token_len_bucket`` through SRSoftMatch and SRPseudoLabel on the
device token loaders; the reservation ``device_tokens`` makes.  bert_tiny_test throughout (hidden 128, 2 layers, 2 heads, 64 positions)."""
import argparse
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import bert_ref as BR                                      # noqa: E402
from semireward_amd import ops                                         # noqa: E402
from semireward_amd.algorithms import get_algorithm                    # noqa: E402
from semireward_amd.algorithms import srflexmatch as SF                # noqa: E402
from semireward_amd.nets import bert                                   # noqa: E402

DEV = "cuda:0"
C = 4
SEED = (9 << 32) + 5                                                   # the injected 64-bit dropout seed


def rel(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _model(**cfg):
    m = bert.ClassificationBert(bert.BertConfig(num_classes=C, **BR.BERT_TINY_TEST, **cfg), device=DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in BR.synth_params(BR.BertCfg(num_classes=C, **BR.BERT_TINY_TEST), 3).items()})
    return m


def _tok(seed, S, L, lo=1, hi=100):
    """S rows padded to L: ids in [lo, hi), one row of full length, the others shorter, [PAD] behind them."""
    g = torch.Generator().manual_seed(seed)
    kl = torch.randint(1, L + 1, (S,), generator=g)
    kl[0] = L
    ids = torch.randint(lo, hi, (S, L), generator=g) * (torch.arange(L)[None] < kl[:, None])
    return bert.TokenBatch(ids.to(DEV).contiguous(), kl.to(torch.int32).to(DEV))


def _dl(seed, B):
    return (0.1 * torch.randn(B, C, generator=torch.Generator().manual_seed(seed))).to(DEV)


def _step(m, tok, dl, seed=SEED):
    """One save=True forward and its backward on zeroed gradients: (logits, features, the whole gradient block), copies."""
    m.train()
    m.inject_seed = seed
    m.zero_grad()
    lg, ft, ctx = m.forward_features(tok, None, save=True)
    m.backward(ctx, dl)
    return lg.clone(), ft.clone(), m.grad.clone()


def _same(a, b):
    return [torch.equal(x, y) for x, y in zip(a, b)]


# ---- 1. the same bits through an arena -----------------------------------------------------------------------------------------------------------------
def _close(a, b):
    """A step at (6, 64): logits and features bit for bit; the gradient block to 1e-6 -- the encoder's LayerNorm affine gradients are summed
    by fp32 atomics (srhip_postln_bwd_part), and at 384 token rows their order differs from run to run on one model and one set of buffers
    (1e-7 of the tensor's largest entry; profiles/run_to_run_distance.txt).  At (3, 19) every run gives the same bits."""
    return [torch.equal(a[0], b[0]), torch.equal(a[1], b[1]), rel(a[2], b[2]) < 1e-6]


def test_same_bits_through_an_arena():
    small, big, tiny = _tok(1, 3, 19), _tok(2, 6, 64), _tok(5, 2, 7)
    dls, dlb, dlt = _dl(3, 3), _dl(4, 6), _dl(6, 2)
    ref_small = _step(_model(), small, dls)                      # a model that never ran another shape
    ref_big = _step(_model(), big, dlb)
    m = _model()                                                 # first (6, 64): (3, 19) takes the leading rows of that arena
    first = _step(m, big, dlb)
    allocs = m.arena_allocations
    second = _step(m, small, dls)
    assert m.arena_allocations == allocs == 2                    # the context arena and the output-gradient arena, made once
    assert _same(second, ref_small) == [True] * 3 and _close(first, ref_big) == [True] * 3
    for n, g in m.named_grads():                                 # (the comparison above is over the whole block: every gradient tensor)
        assert torch.equal(g, ref_small[2][m.offsets[n][0]:m.offsets[n][0] + g.numel()].view(g.shape)), n
    m = _model()                                                 # the order reversed: the arenas grow between the calls
    _step(m, tiny, dlt)
    assert m.arena_allocations == 2
    second = _step(m, small, dls)                                # in arenas made for this call, after another shape ran
    assert m.arena_allocations == 4
    third = _step(m, big, dlb)
    assert m.arena_allocations == 6
    fourth = _step(m, small, dls)                                # ... and in the arenas grown again
    assert m.arena_allocations == 6
    assert _same(second, ref_small) == [True] * 3 and _same(fourth, ref_small) == [True] * 3 and _close(third, ref_big) == [True] * 3


# ---- 2. memory is bounded --------------------------------------------------------------------------------------------------------------------------------
def _ctx_bytes(m, B, L):
    """Bytes of ONE saved-context set at (B, L), from the shapes enc_alloc_ctx and head_alloc_ctx allocate."""
    c = types.SimpleNamespace()
    m.enc_alloc_ctx(c, B, L)
    m.head_alloc_ctx(c, B)
    return sum(t.numel() * t.element_size() for v in vars(c).values() for t in (v if isinstance(v, list) else [v]))


LENGTHS = [64, 3, 61, 5, 58, 8, 55, 11, 52, 14, 49, 17, 46, 20, 43, 23, 40, 26, 37, 29, 34]       # the largest first, then 20 distinct ones


def test_memory_is_bounded_by_the_largest_batch_model_level():
    m, B = _model(), 6
    bound = _ctx_bytes(m, B, min(LENGTHS))
    assert bound == B * min(LENGTHS) * 9520 + 3 * B * 128 * 4                 # tiny: 9520 bytes of saved context per token row (+ the head's three)
    _step(m, _tok(10, B, LENGTHS[0]), _dl(11, B))
    torch.cuda.synchronize()
    base, allocs = torch.cuda.memory_allocated(), m.arena_allocations
    for i, L in enumerate(LENGTHS[1:]):
        out = _step(m, _tok(20 + i, B, L), _dl(11, B))
        assert all(torch.isfinite(t).all() for t in out)
        del out
    torch.cuda.synchronize()
    growth = torch.cuda.memory_allocated() - base
    print("\nmodel level: %d bytes more after 20 distinct lengths (one context set at L = %d: %d bytes), arena allocations %d -> %d"
          % (growth, min(LENGTHS), bound, allocs, m.arena_allocations))
    assert growth < bound                                                     # descriptor tables are a few KB; a leaked context set is not
    assert m.arena_allocations == allocs


def _alg_args(algorithm=None, **kw):
    d = dict(algorithm=algorithm, num_classes=C, num_train_iter=24, epoch=1, ema_m=0.0, ulb_loss_ratio=1.0, use_cat=False, amp=False, lr=5e-4,
             weight_decay=5e-4, layer_decay=0.75, num_warmup_iter=0, optim="AdamW", T=0.5, p_cutoff=0.3, hard_label=True, ulb_dest_len=64, N_k=10,
             start_timing=2, feature_dim=128, sr_lr=5e-4, sr_ema=False, sr_ema_m=0.99, gpu=0, rank=0, world_size=1, distributed=False,
             unsup_warm_up=0.4, ema_p=0.9, n_sigma=2, dist_uniform=True, dist_align=True, per_class=False, batch_size=4, uratio=2, eval_batch_size=8)
    d.update(kw)
    return argparse.Namespace(**d)


def test_memory_is_bounded_by_the_largest_batch_step_level(monkeypatch):
    monkeypatch.setattr(SF, "_DEFER_AUTOTUNE", False)
    alg = get_algorithm(_alg_args("srsoftmatch"), bert.bert_tiny_test)
    nl, nu = 4, 8
    y = torch.arange(nl, device=DEV) % C
    idx = torch.arange(nu, device=DEV)

    def step(i, L):                                                           # three views of different lengths
        alg.model.train()
        alg.it = 1
        alg.optimizer.sched_step = 1
        views = dict(x_lb=_tok(100 + i, nl, L), x_ulb_w=_tok(200 + i, nu, max(1, L - 2)), x_ulb_s=_tok(300 + i, nu, max(1, L - 1)))
        out, log = alg.train_step(**alg.process_batch(y_lb=y, idx_ulb=idx, **views))
        assert np.isfinite(float(log["train/total_loss"]))
    lengths = [64, 7, 57, 12, 50, 19, 43, 26, 36]
    bound = _ctx_bytes(alg.model, nl + nu, min(lengths))                      # the gradient rows: labelled + strong
    step(0, lengths[0]), step(1, lengths[0])
    torch.cuda.synchronize()
    base, allocs = torch.cuda.memory_allocated(), alg.model.arena_allocations
    for i, L in enumerate(lengths[1:]):
        step(2 + 2 * i, L), step(3 + 2 * i, L)                                # two steps per length
    torch.cuda.synchronize()
    growth = torch.cuda.memory_allocated() - base
    print("\nstep level: %d bytes more after 8 distinct lengths (one context set at L = %d: %d bytes), arena allocations %d"
          % (growth, min(lengths), bound, alg.model.arena_allocations))
    assert growth < bound and alg.model.arena_allocations == allocs
    ops.check_label_errors()


# ---- 3. filler is inert, bit for bit --------------------------------------------------------------------------------------------------------------------
def _three_views():
    return [_tok(41, 2, 5), _tok(42, 3, 17), _tok(43, 2, 33)]                 # own padded lengths 5, 17, 33; ids below 100


def _filler_runs(cache={}):
    """One bucketed step with [PAD] in the filler rows and the same step with arbitrary ids there (ids nothing else uses): (model, a, b)."""
    if not cache:
        m = _model()
        tb = bert.TokenBatch.cat(_three_views(), bucket=16, max_pos=m.cfg.max_pos, pad_id=m.cfg.pad_id)
        assert tb.L == 48 and tb.seq_len.cpu().tolist() == [5, 5, 17, 17, 17, 33, 33]
        filler = torch.arange(tb.L, device=DEV)[None] >= tb.seq_len[:, None]
        assert bool((tb.ids[filler] == m.cfg.pad_id).all())
        other = tb.ids.clone()
        other[filler] = torch.randint(100, 120, (int(filler.sum()),), generator=torch.Generator().manual_seed(44)).to(DEV)
        dl = _dl(45, tb.S)
        cache["runs"] = (m, _step(m, tb, dl), _step(m, bert.TokenBatch(other.contiguous(), tb.key_len, tb.seq_len), dl))
    return cache["runs"]


def test_filler_is_inert_bit_for_bit():
    """Logits, features and ALL gradients of the two runs, bit for bit, and the word-embedding rows of the filler ids exactly zero.  (The
    embedding stage's backward sums its three tables and its LayerNorm's affine gradients in one fixed order -- srhip_embed_ln_bwd_ordered --;
    summed by fp32 atomics, as they were, these five tensors changed bits whenever the SAME batch ran twice.)"""
    m, a, b = _filler_runs()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    wg = m.view(bert.E + "word_embeddings.weight", b[2])
    assert float(wg[100:120].abs().max()) == 0.0 and float(wg[1:100].abs().max()) > 0.0       # the filler ids' embedding rows: exactly zero
    assert float(m.view(bert.E + "word_embeddings.weight", a[2])[100:120].abs().max()) == 0.0
    differ = [n for n, _ in m.names_shapes if not torch.equal(m.p(n, a[2]), m.p(n, b[2]))]
    print("\ngradient tensors whose bits differ between the two runs: %s" % (differ or "none"))
    assert differ == []                                                       # every gradient, bit for bit


def test_ordered_embedding_backward_against_the_atomic_one():
    """srhip_embed_ln_bwd_ordered beside srhip_embed_ln_bwd (tested per element against float64 by tests/test_gpu_enc_cases.py) on the same
    inputs: the same sums in another order, [PAD] rows without a gradient, a gathered batch
    (seq_index), accumulation into what the tables hold, and the same bits when it runs again."""
    cfg = BR.BERT_TINY_TEST
    D, V, P_ = cfg["hidden"], cfg["vocab"], cfg["max_pos"]
    g = torch.Generator().manual_seed(8)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)                  # noqa: E731
    for B, L, gather in ((6, 64, False), (3, 19, False), (5, 33, True), (1, 1, False)):
        S = B + 2 if gather else B
        ids = torch.randint(0, 40, (S, L), generator=g).to(DEV)              # few ids: every table row is hit many times; 0 = [PAD]
        si = torch.randperm(S, generator=g)[:B].to(torch.int32).to(DEV) if gather else None
        M = B * L
        dy, word, pos, typ, gamma = rnd(M, D), rnd(V, D), rnd(P_, D), rnd(2, D), rnd(D)
        mean, rstd = rnd(M), rnd(M).abs() + 0.5
        drop = ops.Drop(SEED, bert.SITE_EMB, 0.1)
        start = [0.1 * rnd(V, D), 0.1 * rnd(P_, D), 0.1 * rnd(2, D), 0.1 * rnd(D), 0.1 * rnd(D)]
        ws = torch.empty(ops.embed_ln_bwd_ws_floats(B, L, D) + 7, device=DEV)
        assert ops.embed_ln_bwd_ws_floats(B, L, D) == M * D + (M + 31) // 32 * 3 * D + 2 * M

        def run(ordered):
            out = [t.clone() for t in start]
            if ordered:
                ws.fill_(float("nan"))                                        # nothing is kept between calls
                ops.embed_ln_bwd_ordered(dy, ids, si, word, pos, typ, mean, rstd, gamma, *out, ws, B, L, D, 0, drop)
            else:
                ops.embed_ln_bwd(dy, ids, si, word, pos, typ, mean, rstd, gamma, *out, B, L, D, 0, drop)
            return out
        a, b, c = run(True), run(True), run(False)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), (B, L)
        for x, y, s0 in zip(a, c, start):
            # up to M fp32 addends per element, in two orders: M roundings of 2^-24 relative to the largest entry at the most
            assert float((x - y).abs().max()) <= 2.0 ** -24 * M * float(y.abs().max()), (B, L, float((x - y).abs().max()), float(y.abs().max()))
        assert torch.equal(a[0][0], start[0][0]) and not torch.equal(a[0][1:40], start[0][1:40])       # [PAD]'s row untouched, the others moved
        assert torch.equal(a[0][40:], start[0][40:]) and torch.equal(a[1][L:], start[1][L:])           # rows no token or position reaches


# ---- 4. bucketing computes the same function ---------------------------------------------------------------------------------------------------------------
TOL = 2e-3            # what test_bert_matches_reference_golden holds two schedules of one function to (no-save against save)


def test_bucketed_batch_computes_the_function_of_separate_calls():
    views = _three_views()
    m = _model()
    m.eval()
    tb = bert.TokenBatch.cat(views, bucket=16, max_pos=m.cfg.max_pos)
    lg, ft, _ = m.forward_features(tb, None, save=False)
    lg, ft = lg.clone(), ft.clone()
    sep = [m.forward_features(v, None, save=False) for v in views]
    lg_s, ft_s = torch.cat([s[0] for s in sep]), torch.cat([s[1] for s in sep])
    print("\neval: rel-L2 bucketed against separate calls: logits %.2e features %.2e" % (rel(lg, lg_s), rel(ft, ft_s)))
    assert rel(lg, lg_s) < TOL and rel(ft, ft_s) < TOL
    # the gradients of a save=True step without dropout
    m = _model(p_drop=0.0, p_head=0.0)
    dl = _dl(46, tb.S)
    _, _, g_cat = _step(m, tb, dl, seed=None)
    m.zero_grad()
    r = 0
    for v in views:                                                           # three separate forwards and backwards, accumulated
        _, _, ctx = m.forward_features(v, None, save=True)
        m.backward(ctx, dl[r:r + v.S].contiguous())
        r += v.S
    g_sep = m.grad.clone()
    worst = {}
    for n, _ in m.names_shapes:
        a, b = m.p(n, g_cat), m.p(n, g_sep)
        if float(b.abs().max()) == 0.0:                                       # pooler (no path to the loss), the [PAD] row's tensor-mates are not: whole tensors only
            assert float(a.abs().max()) == 0.0, n
            continue
        if n.endswith("key.bias"):                                            # analytically zero (softmax is invariant): round-off on both sides
            continue
        worst[n] = rel(a, b)
    print("gradients: worst rel-L2 bucketed against separate calls: %s"
          % ", ".join("%s %.2e" % (k.replace("bert.encoder.layer.", "L"), v) for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:5]))
    assert max(worst.values()) < TOL, sorted(worst.items(), key=lambda kv: -kv[1])[:5]


# ---- 5. the key through the algorithms -----------------------------------------------------------------------------------------------------------------------
MAX_LENGTH, BUCKET = 40, 16
# The data seed (77) and the cutoff were fixed after running the fp32 oracle (oracle/bert_ref.py) on the CPU over these rows with the weights the
# algorithm starts from: the unlabelled confidences run from 0.402 to 0.608, the cutoff sits in their widest gap near the low end (0.4177 | 0.4365:
# 30 of 32 rows selected, the closest row 2.2 % away), the smallest top-2 logit gap is 2.4 % of the largest logit (evaluation rows and unlabelled
# rows alike).  Two schedules of one function agree to TOL = 0.2 %, so no row can change sides; the test asserts the margins it meets on the
# GPU (at twice TOL) before it compares.
P_CUTOFF = 0.427
ALGS = {"srpseudolabel": dict(algorithm="srpseudolabel"), "srsoftmatch": dict(algorithm="srsoftmatch")}


def _dataset_dict(strong):
    rng = np.random.Generator(np.random.PCG64(77))
    rows = lambda n: [rng.integers(1, 120, size=int(rng.integers(2, MAX_LENGTH + 1))).astype(np.int32) for _ in range(n)]      # noqa: E731
    dd = {"train_lb": {"data": rows(8), "targets": rng.integers(0, C, size=8)},
          "train_ulb": {"data": rows(32), "targets": None},
          "eval": {"data": rows(13), "targets": rng.integers(0, C, size=13)}}
    if strong:
        dd["train_ulb"]["data_s"] = [rows(32), rows(32)]
    return dd


def _token_alg(name, **kw):
    alg = get_algorithm(_alg_args(dataset="aclImdb", max_length=MAX_LENGTH, train_sampler="RandomSampler", seed=7, ulb_dest_len=None,
                                  device_tokens=True, dataset_dict=_dataset_dict(name == "srsoftmatch"), num_train_iter=4, p_cutoff=P_CUTOFF, **ALGS[name], **kw),
                        bert.bert_tiny_test)
    alg.model.view("classifier.2.weight").mul_(8.0)                          # spread the logits (a random-init head is flat)
    alg.model.refresh_operands()
    return alg


def _record_lengths(alg):
    seen, real = [], alg.model.forward_features

    def forward_features(tok, *a, **kw):
        seen.append((tok.S, tok.L, tok.seq_len is not None))
        return real(tok, *a, **kw)
    alg.model.forward_features = forward_features
    return seen


@pytest.mark.parametrize("name", sorted(ALGS))
def test_key_through_the_algorithms(monkeypatch, name):
    monkeypatch.setattr(SF, "_DEFER_AUTOTUNE", False)
    plain, keyed = _token_alg(name), _token_alg(name, token_len_bucket=BUCKET)
    assert torch.equal(plain.model.flat, keyed.model.flat) and keyed.token_len_bucket == BUCKET and plain.token_len_bucket is None
    max_pos = keyed.model.cfg.max_pos
    seen_plain, seen = _record_lengths(plain), _record_lengths(keyed)
    # evaluate() and score_unlabeled() of the same weights: the metrics and the table of the run without the key
    ev_p, ev_k = (a.evaluate("eval", return_logits=True) for a in (plain, keyed))
    gap = np.sort(ev_p["eval/logits"], axis=-1)
    gap = (gap[:, -1] - gap[:, -2]) / np.abs(ev_p["eval/logits"]).max()
    print("\n%s evaluate: smallest top-2 logit gap / largest logit %.3e; rel-L2 of the logits %.2e"
          % (name, gap.min(), rel(torch.from_numpy(ev_k["eval/logits"]), torch.from_numpy(ev_p["eval/logits"]))))
    assert gap.min() > 2 * TOL                                                # no row sits within the margin of a tie
    assert rel(torch.from_numpy(ev_k["eval/logits"]), torch.from_numpy(ev_p["eval/logits"])) < TOL
    assert all(ev_k[k] == ev_p[k] for k in ev_p if k not in ("eval/loss", "eval/logits"))
    assert ev_k["eval/loss"] == pytest.approx(ev_p["eval/loss"], rel=TOL)
    tp, tk = (a.score_unlabeled(batch_size=8).read() for a in (plain, keyed))
    near = np.abs(tp["conf"] - P_CUTOFF) / P_CUTOFF if name == "srpseudolabel" else np.ones(1)      # (SoftMatch weighs, it has no cutoff)
    away, moved = np.abs(tp["reward"] - np.repeat(tp["reward"].reshape(-1, 8).mean(1), 8)), np.abs(tk["reward"] - tp["reward"]).max()
    print("%s score_unlabeled: conf within %.3e (relative) of the cutoff at the closest row; reward at least %.3e from its group mean, moved by at most %.3e"
          % (name, near.min(), away.min(), moved))
    # no row sits at a threshold: the cutoff, and the reward filter's group mean (an untrained Rewarder gives every row of a group the same
    # reward, bit for bit in both runs: then nothing moved and nothing can change sides)
    assert near.min() > 2 * TOL and (moved == 0.0 or away.min() > 10 * moved)
    for k in ("label", "reward_keep", "selected", "count") + (("weight",) if name == "srpseudolabel" else ()):
        assert np.array_equal(tk[k], tp[k]), k                                # labels, masks and `selected`: exactly
    assert np.allclose(tk["conf"], tp["conf"], rtol=TOL, atol=0)
    if name == "srsoftmatch":
        # the weight is a smooth function of the confidence: |dw / dconf| <= n_sigma^2 |conf - mu| / var <= 4 / var at n_sigma = 2
        var = float(plain.hooks_dict["MaskingHook"].mu_var[1])
        assert np.allclose(tk["weight"], tp["weight"], rtol=0, atol=4 / var * TOL)
    assert all(L % BUCKET == 0 or L == max_pos for _, L, _ in seen) and any(L % BUCKET for _, L, _ in seen_plain)
    # steps through the device token loaders
    del seen[:], seen_plain[:]
    for alg in (keyed, plain):
        losses = []
        for n, (lb, ulb) in enumerate(zip(alg.loader_dict["train_lb"], alg.loader_dict["train_ulb"])):
            alg.model.train()
            alg.it = n + 1                                                    # start_timing 2: the last steps run data_generator passes
            alg.optimizer.sched_step = n + 1
            out, log = alg.train_step(**alg.process_batch(**lb, **ulb))
            losses.append(float(log["train/total_loss"]))
        torch.cuda.synchronize()
        assert len(losses) == 4 and all(np.isfinite(v) for v in losses), losses
    assert seen and all(L % BUCKET == 0 or L == max_pos for _, L, _ in seen), seen
    assert all(has_seq_len for _, _, has_seq_len in seen) and any(L % BUCKET for _, L, _ in seen_plain)
    ops.check_label_errors()


# ---- 6. the reservation -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bucket", [None, BUCKET])
def test_reservation_covers_a_whole_epoch(monkeypatch, bucket):
    monkeypatch.setattr(SF, "_DEFER_AUTOTUNE", False)
    alg = _token_alg("srsoftmatch", **({} if bucket is None else dict(token_len_bucket=bucket)))
    m = alg.model
    longest = max(int(alg.loader_dict[k].dataset.row_len_host.max()) for k in ("train_lb", "train_ulb"))
    n_seq, L = 4 + 8 + 8, ops.token_len_bucket(longest, bucket, m.cfg.max_pos)            # labelled + weak + strong, the longest stored row, bucketed
    assert longest == MAX_LENGTH and L == (MAX_LENGTH if bucket is None else 48)
    assert m._reserved == (n_seq * L, n_seq) and m.arena_allocations == 2     # made when the algorithm was built
    assert all(a.rows == n_seq * L for a in m._arenas.values())
    torch.cuda.synchronize()
    for n, (lb, ulb) in enumerate(zip(alg.loader_dict["train_lb"], alg.loader_dict["train_ulb"])):
        alg.model.train()
        alg.it = n + 1
        alg.optimizer.sched_step = n + 1
        alg.train_step(**alg.process_batch(**lb, **ulb))
    alg.evaluate("eval")
    torch.cuda.synchronize()
    assert n == 3 and m.arena_allocations == 2 and len(m._arenas) == 2        # a whole epoch: nothing regrew, nothing was added
    ops.check_label_errors()
