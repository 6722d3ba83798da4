"""BERT classification backbone engine on libsrhip: forward / backward over a flat parameter block.

Mirrors the reference's ``semilearn/nets/bert/bert.py`` plugin surface (class ``ClassificationBert``, builders ``bert_base_uncased`` /
``bert_base_cased``, ``state_dict`` keys = ``bert.`` + the HF BertModel names + ``classifier.0/2``, dict input
``{'input_ids', 'attention_mask'}``, ``{'logits','feat'}`` result, ``group_matcher`` / ``no_weight_decay``) but not its implementation:
no nn.Module, no autograd, no ``transformers``.  The encoder the reference obtains from ``transformers.BertModel`` (post-LN layers,
erf-GELU, LayerNorm eps 1e-12, dropout 0.1 in train mode) is a short list of HIP launches per layer:

    qkv  = x_bf16 . Wqkv^T + b                       srhip_gemm_nt            (q | k | v packed: one product, N = 3D)
    ctx  = softmax(q k^T / 8 + key mask) v           srhip_attn_masked_fwd    (per-sequence key length, dropout on the probabilities)
    y1   = x + dropout(ctx . Wo^T + b)               srhip_gemm_nt_resid_dropout
    x    = LayerNorm(y1)          (fp32 + bf16)      srhip_postln_fwd
    h    = GELU(x_bf16 . W1^T + b)                   srhip_gemm_nt (GELU epilogue)
    y2   = x + dropout(h . W2^T + b)                 srhip_gemm_nt_resid_dropout
    x    = LayerNorm(y2)                             srhip_postln_fwd

and the backward is hand-written (post-LN: the gradient of a LayerNorm input feeds the residual path in fp32 and, dropout-masked, the
branch's dX / dW products in bf16).  Data layout: B sequences padded to a common L, M = B * L token rows; the residual stream is fp32
[M, D], GEMM operands bf16; the flat parameter block keeps q/k/v weights (and biases) of a layer adjacent, so the packed [3D, D]
operand is a VIEW, and a reference checkpoint still maps by name.  ``from_pretrained`` becomes a lookup of the checkpoint on disk
(nets/pretrained.py: a ``pretrained_path`` directory or the Hugging Face hub cache, never the network); without one the weights are
random-init (HF: normal(0, 0.02), LayerNorm 1/0).

Padding: batches are right-padded (``tokenizer.pad``, nlp_collactor.py:63-69), so the attention mask is a prefix mask and the engine
carries ``key_len = mask.sum(1)``; every position -- padding included -- is computed and averaged, exactly like bert.py:36-37.
"""
import types

import torch

from .. import ops
from . import pretrained
from .encoder import PostLNEncoderMixin

SITE_EMB, SITE_HEAD = 0x7FFFFFF0, 0x7FFFFFF1


class BertConfig:
    def __init__(self, vocab=30522, hidden=768, layers=12, heads=12, inter=3072, max_pos=512, num_classes=2, p_drop=0.1, eps=1e-12,
                 pad_id=0, p_head=None):
        self.vocab, self.hidden, self.layers, self.heads, self.inter, self.max_pos = vocab, hidden, layers, heads, inter, max_pos
        self.num_classes, self.p_drop, self.eps, self.pad_id = num_classes, p_drop, eps, pad_id
        self.p_head = p_drop if p_head is None else p_head       # dropout before the mean-pool (bert.py:14); a checkpoint's config sets p_drop only
        assert hidden // heads == 64 and hidden in (128, 384, 768), "libsrhip attention is built for head_dim 64"
        assert inter % 32 == 0 and max_pos <= 512
    embed_dim = property(lambda self: self.hidden)
    depth = property(lambda self: self.layers)
    drop_path_rate = 0.0


E = "bert.embeddings."


def _layer(i):
    return "bert.encoder.layer.%d." % i


def param_names_shapes(cfg):
    """Flat-block order: the reference's names; q/k/v weights, then q/k/v biases, adjacent (packed operand views)."""
    D, I = cfg.hidden, cfg.inter
    out = [(E + "word_embeddings.weight", (cfg.vocab, D)), (E + "position_embeddings.weight", (cfg.max_pos, D)),
           (E + "token_type_embeddings.weight", (2, D)), (E + "LayerNorm.weight", (D,)), (E + "LayerNorm.bias", (D,))]
    for i in range(cfg.layers):
        p = _layer(i)
        out += [(p + "attention.self.%s.weight" % n, (D, D)) for n in ("query", "key", "value")]
        out += [(p + "attention.self.%s.bias" % n, (D,)) for n in ("query", "key", "value")]
        out += [(p + "attention.output.dense.weight", (D, D)), (p + "attention.output.dense.bias", (D,)),
                (p + "attention.output.LayerNorm.weight", (D,)), (p + "attention.output.LayerNorm.bias", (D,)),
                (p + "intermediate.dense.weight", (I, D)), (p + "intermediate.dense.bias", (I,)),
                (p + "output.dense.weight", (D, I)), (p + "output.dense.bias", (D,)),
                (p + "output.LayerNorm.weight", (D,)), (p + "output.LayerNorm.bias", (D,))]
    out += [("bert.pooler.dense.weight", (D, D)), ("bert.pooler.dense.bias", (D,)),
            ("classifier.0.weight", (D, D)), ("classifier.0.bias", (D,)), ("classifier.2.weight", (cfg.num_classes, D)),
            ("classifier.2.bias", (cfg.num_classes,))]
    return out


class TokenBatch:
    """A right-padded token batch on the device: ids int64 [S, L] (contiguous), key_len int32 [S] = valid tokens per sequence,
    seq_len int32 [S] or None = the padded length of every sequence's own source batch when batches of different padded lengths were
    concatenated (rows [seq_len, L) are filler: masked as keys, left out of the mean pool, zero gradient -- results equal separate calls)."""
    __slots__ = ("ids", "key_len", "seq_len", "S", "L")

    def __init__(self, ids, key_len, seq_len=None):
        self.ids, self.key_len, self.seq_len = ids, key_len, seq_len
        self.S, self.L = ids.shape

    @classmethod
    def from_dict(cls, x, device):
        ids = x["input_ids"].to(device=device, dtype=torch.int64).contiguous()
        S, L = ids.shape
        kl = torch.empty(S, dtype=torch.int32, device=device)
        am = x.get("attention_mask")
        if am is None:
            kl.fill_(L)
        else:
            ops.mask_lengths(am.to(device=device, dtype=torch.int64).contiguous(), kl, S, L)
        return cls(ids, kl)

    def to(self, device, non_blocking=False):
        """What ``process_batch`` asks of every batch value: a batch already on ``device`` (the device token loaders') is returned as it is."""
        if self.ids.device == torch.device(device):
            return self
        mv = lambda t: None if t is None else t.to(device, non_blocking=non_blocking)     # noqa: E731
        return TokenBatch(mv(self.ids), mv(self.key_len), mv(self.seq_len))

    def as_dict(self):
        """The collator's {'input_ids', 'attention_mask'} (int64, on the batch's device): what ``from_dict`` would turn back into this batch."""
        mask = (torch.arange(self.L, device=self.ids.device)[None, :] < self.key_len[:, None]).to(torch.int64)
        return {"input_ids": self.ids, "attention_mask": mask}

    @classmethod
    def cat(cls, batches, bucket=None, max_pos=None, pad_id=0, out=None):
        """One batch out of several (x_lb, x_ulb_w, x_ulb_s of one step; the reference forwards them in separate model calls under
        use_cat=False, each padded to its own longest row).  Batches of one padded length without a ``bucket`` are concatenated as they are
        (seq_len stays None).  Otherwise ONE srhip_token_cat launch fills every row up to L_out with ``pad_id`` and writes seq_len, each
        row's own padded length: L_out is the longest L, or with ``bucket`` (``token_len_bucket``) min(ceil(L / bucket) * bucket, max_pos)
        -- a single batch is a cat of one source.  ``out``: a TokenCatBuffer the three outputs are views of (nothing is allocated once it
        has met the largest batch; the result is valid until the next cat into it)."""
        batches = list(batches)
        L = max(b.L for b in batches)
        if not bucket and all(b.L == L and b.seq_len is None for b in batches):
            return cls(torch.cat([b.ids for b in batches]).contiguous(), torch.cat([b.key_len for b in batches]).contiguous())
        if bucket and max_pos is None:
            raise ValueError("TokenBatch.cat: a bucket needs max_pos, the length no batch may exceed")
        L_out = ops.token_len_bucket(L, bucket, max_pos)
        ids, kl, sl = ops.token_cat([(b.ids, b.key_len, b.seq_len) for b in batches], L_out, pad_id,
                                    out=None if out is None else out.take(sum(b.S for b in batches), L_out))
        return cls(ids, kl, sl)


class TokenCatBuffer:
    """Grow-only storage of ``TokenBatch.cat``'s outputs on one device: ``take(S, L)`` returns (ids int64 [S, L], key_len int32 [S], seq_len
    int32 [S]) as leading views of the largest allocation made so far, every ids row as aligned as a fresh tensor's."""

    def __init__(self, device):
        self.device, self.ids, self.lens = torch.device(device), None, None

    def take(self, S, L):
        if self.ids is None or self.ids.numel() < S * L:
            self.ids = None
            self.ids = torch.empty(S * L, dtype=torch.int64, device=self.device)
        if self.lens is None or self.lens.shape[1] < S:
            self.lens = None
            self.lens = torch.empty(2, S, dtype=torch.int32, device=self.device)
        return self.ids[:S * L].view(S, L), self.lens[0, :S], self.lens[1, :S]


class ClassificationBert(PostLNEncoderMixin):
    takes_tokens = True
    rows_independent = True       # LayerNorm only, counter-based dropout indexed per row

    def __init__(self, cfg=None, device="cuda", **kw):
        self.cfg = cfg if cfg is not None else BertConfig(**kw)
        cfg = self.cfg
        self.device = torch.device(device)
        self.num_features = cfg.hidden
        self._init_block(param_names_shapes(cfg), align=8, bf16=True)     # 16-byte alignment of every tensor in the bf16 copy
        self.enc_alloc_wT()                           # per layer: transposed bf16 operands of the dX products
        self.enc_p = dict(attn=cfg.p_drop, hidden=cfg.p_drop, act=0.0)
        self._rng_calls, self.seed = 0, 0
        self.inject_seed = None                       # tests: the 64-bit dropout seed of the next forward calls
        self.token_cat_out = TokenCatBuffer(self.device)     # where TokenBatch.cat joins a step's views (the algorithms' _token_cat)

    def enc_names(self, i):
        p = _layer(i)
        return dict(q_w=p + "attention.self.query.weight", q_b=p + "attention.self.query.bias",
                    o_w=p + "attention.output.dense.weight", o_b=p + "attention.output.dense.bias",
                    ln1_w=p + "attention.output.LayerNorm.weight", ln1_b=p + "attention.output.LayerNorm.bias",
                    w1=p + "intermediate.dense.weight", b1=p + "intermediate.dense.bias",
                    w2=p + "output.dense.weight", b2=p + "output.dense.bias",
                    ln2_w=p + "output.LayerNorm.weight", ln2_b=p + "output.LayerNorm.bias")

    def init_weights(self, seed=0):
        """HF BertPreTrainedModel._init_weights: normal(0, 0.02) for Linear / Embedding weights ([PAD] row zero), LayerNorm 1 / 0, biases 0;
        the classifier Linears keep torch's default U(+-1/sqrt(fan_in))."""
        g = torch.Generator(device="cpu").manual_seed(seed)
        sd = {}
        for n, s in self.names_shapes:
            if "LayerNorm.weight" in n:
                sd[n] = torch.ones(s)
            elif n.startswith("classifier"):
                bound = 1.0 / (self.cfg.hidden ** 0.5)
                sd[n] = (torch.rand(s, generator=g) * 2 - 1) * bound
            elif len(s) == 1:
                sd[n] = torch.zeros(s)
            else:
                sd[n] = torch.randn(s, generator=g) * 0.02
        sd[E + "word_embeddings.weight"][self.cfg.pad_id].zero_()
        self.load_state_dict(sd)

    frozen_params = ("bert.pooler.dense.weight", "bert.pooler.dense.bias")    # feed nothing on this path: grad None in the reference

    def layer_ids(self):
        """group_with_matcher(named_parameters, group_matcher, reverse=True) (nets/utils.py:208-270): embeddings 0, encoder layer i -> i + 1,
        everything unmatched (pooler, classifier) -> the last id."""
        L = self.cfg.layers
        ids = {}
        for n, _ in self.names_shapes:
            if n.startswith("bert.embeddings"):
                ids[n] = 0
            elif n.startswith("bert.encoder.layer."):
                ids[n] = int(n.split(".")[3]) + 1
            else:
                ids[n] = L + 1
        return ids, L + 1

    def group_matcher(self, coarse=False, prefix=""):
        return dict(stem=r"^{}bert.embeddings".format(prefix), blocks=r"^{}bert.encoder.layer.(\d+)".format(prefix))

    def next_seed(self):
        """64-bit dropout seed of one forward call (None in eval mode / p_drop == p_head == 0)."""
        if not self.training or max(self.cfg.p_drop, self.cfg.p_head) <= 0.0:
            return None
        if self.inject_seed is not None:
            return self.inject_seed
        self._rng_calls += 1
        return ((self.seed & 0xFFFFFFFF) << 32) + self._rng_calls

    # ---- forward ----------------------------------------------------------------------------------------
    def _ctx_arena(self, tag, rows=0, seqs=0):
        a = self._arenas.get(("ctx", tag))
        if a is None:
            a = self._arena(("ctx", tag), self.enc_ctx_spec() + [("st0", 1, "row", 2, torch.float32)], rows, seqs)
            a.views = {}                                     # (B, L) -> the view set; void when the arena is replaced
            a.on_release.append(a.views.clear)
        else:
            a.reserve(max(rows, self._reserved[0]), max(seqs, self._reserved[1]))
        return a

    def _ctx_buffers(self, B, L, tag):
        """The saved context of a save=True forward at (B, L): views of the first B * L rows of the grow-only arena of ``tag`` (nets/surface.py
        RowArena) -- memory follows the largest batch met, not the number of distinct padded lengths.  Two contexts that are alive at the same
        time need two tags: they would share the arena's rows."""
        a = self._ctx_arena(tag, B * L, B)
        c = a.views.get((B, L))
        if c is None:
            if len(a.views) >= 64:                           # host objects only: the oldest view set goes
                a.views.pop(next(iter(a.views)))
            c = a.views[(B, L)] = types.SimpleNamespace(arena=a)
            self.enc_view_ctx(c, a, B, L)
            c.st0 = a.view("st0", 0, (2, B * L))
        return c

    def reserve_tokens(self, n_seq, L, tags=("",)):
        """Room for batches of up to ``n_seq`` sequences padded to ``L`` in every arena and rows-capacity workspace: the saved context of ``tags``
        and of every tag met so far, their output-gradient buffers, and whatever is made later starts at this size.  A run that reserves its
        largest batch up front (``set_data_loader`` with ``device_tokens``) never regrows: ``arena_allocations`` stays put."""
        n_seq, L = int(n_seq), int(L)
        if n_seq < 1 or not 1 <= L <= self.cfg.max_pos:
            raise ValueError("reserve_tokens: n_seq >= 1 sequences of 1 .. %d (max_pos) tokens, got %d x %d" % (self.cfg.max_pos, n_seq, L))
        self._reserved = (max(self._reserved[0], n_seq * L), max(self._reserved[1], n_seq))
        self.token_cat_out.take(n_seq, L)
        for tag in tags:                                     # the context arena and, through its plan, the output-gradient arena
            self.enc_bwd_arena(n_seq * L, self._ctx_buffers(n_seq, L, tag))
        for a in list(self._arenas.values()):
            a.reserve(*((self._reserved[0], 0) if not any(s[2] == "seq" for s in a.spec) else self._reserved))

    def forward_features(self, tok, seq_index=None, droppath=None, save=False, B=None, seed="auto", tag="", buftag=""):
        """tok: TokenBatch; seq_index int32 [B] (optional gather of sequences: lets the K+1 passes of one SemiReward step share one
        copy of the tokens).  Returns (logits [B, C], feat [B, D], ctx or None).  ``droppath`` is accepted for interface parity
        with the ViT engine and unused (BERT has no stochastic depth)."""
        cfg = self.cfg
        D, I, H, C, L = cfg.hidden, cfg.inter, cfg.heads, cfg.num_classes, tok.L
        B = int(seq_index.numel()) if seq_index is not None else tok.S
        M = B * L
        f32, bf16 = torch.float32, torch.bfloat16
        seed = self.next_seed() if seed == "auto" else seed
        key_len = tok.key_len if seq_index is None else tok.key_len.index_select(0, seq_index.long()).contiguous()
        seq_len = None
        if tok.seq_len is not None:
            seq_len = tok.seq_len if seq_index is None else tok.seq_len.index_select(0, seq_index.long()).contiguous()
        P = self.p
        t = ("s" if save else "i") + buftag
        dr = (lambda site, p=cfg.p_drop: ops.Drop(seed, site, p) if p > 0 else None) if seed is not None else (lambda site, p=0.0: None)
        ctx = None
        x = self._buf_rows(t + "x", (M, D), f32, M)
        if save:
            ctx = self._ctx_buffers(B, L, tag)
            ctx.B, ctx.L, ctx.tok, ctx.seq_index, ctx.key_len, ctx.seq_len, ctx.seed = B, L, tok, seq_index, key_len, seq_len, seed
            xb = ctx.xb[0]
        else:
            xb = self._buf_rows(t + "xb", (M, D), bf16, M)
        ops.embed_ln_fwd(tok.ids, seq_index, P(E + "word_embeddings.weight"), P(E + "position_embeddings.weight"),
                         P(E + "token_type_embeddings.weight"), P(E + "LayerNorm.weight"), P(E + "LayerNorm.bias"), cfg.eps, x, xb,
                         ctx.st0[0] if save else None, ctx.st0[1] if save else None, B, L, D, dr(SITE_EMB))
        self.enc_forward(x, xb, ctx, save, B, L, key_len, dr, tag=t)
        logits, feat = self.head_forward(x, B, L, dr(SITE_HEAD, cfg.p_head), seq_len, ctx)
        return logits, feat, ctx

    def forward(self, x, only_fc=False, only_feat=False, return_embed=False, **kw):
        """Reference-compatible entry (bert.py:22-48): x = {'input_ids', 'attention_mask'} -> {'logits','feat'}."""
        assert not only_fc and not return_embed, "only_fc / return_embed (VAT) are not on the SemiReward hot path"
        tok = x if isinstance(x, TokenBatch) else TokenBatch.from_dict(x, self.device)
        logits, feat, _ = self.forward_features(tok, None, save=False)
        return feat if only_feat else {"logits": logits, "feat": feat}

    __call__ = forward

    def extract(self, x):
        return self.forward(x, only_feat=True)

    # ---- backward -----------------------------------------------------------------------------------------
    def backward(self, ctx, dlogits):
        """Accumulates d(loss)/d(params) into ``self.grad`` given dlogits fp32 [B, C] of a save=True forward."""
        cfg = self.cfg
        D = cfg.hidden
        B, L, seed = ctx.B, ctx.L, ctx.seed
        M = B * L
        dr = (lambda site, p=cfg.p_drop: ops.Drop(seed, site, p) if p > 0 else None) if seed is not None else (lambda site, p=0.0: None)
        P, G = self.p, (lambda n: self.p(n, self.grad))
        dx = self._buf_rows("b_dx", (M, D), torch.float32, M)
        self.head_backward(ctx, dlogits, dx, B, L, dr(SITE_HEAD, cfg.p_head), ctx.seq_len)
        self.enc_backward(dx, ctx, B, L, ctx.key_len, dr)
        # one summation order for the three tables and the embedding LayerNorm (no fp32 atomics): equal bits for equal inputs, and the
        # filler rows of a joined / bucketed batch change no bit whatever ids they hold
        nws = M * D + (M + 31) // 32 * 3 * D + 2 * M            # = ops.embed_ln_bwd_ws_floats(B, L, D)
        ws = self._buf_rows("b_embws", (nws,), torch.float32, M)
        ops.embed_ln_bwd_ordered(dx, ctx.tok.ids, ctx.seq_index, P(E + "word_embeddings.weight"), P(E + "position_embeddings.weight"),
                         P(E + "token_type_embeddings.weight"), ctx.st0[0], ctx.st0[1], P(E + "LayerNorm.weight"),
                         G(E + "word_embeddings.weight"), G(E + "position_embeddings.weight"), G(E + "token_type_embeddings.weight"),
                                 G(E + "LayerNorm.weight"), G(E + "LayerNorm.bias"), ws, B, L, D, cfg.pad_id, dr(SITE_EMB))


# ---- builders with the reference's names (bert.py:62-69) --------------------------------------------------------------------------------
def _build(num_classes, kw, hub_name=None, **cfg):
    """Like the reference's ``BertModel.from_pretrained(name)``, whatever ``pretrained`` says: the encoder starts from the ``pretrained_path``
    directory or the hub-cache snapshot of ``hub_name`` when one is on disk (nets/pretrained.py), with the dropout of its config.json;
    the classifier and, when nothing is found, the whole model keep the random init of ``seed``."""
    kw = dict(kw)
    kw.pop("pretrained", None)
    path = kw.pop("pretrained_path", None)
    device = kw.pop("device", "cuda")
    bcfg = BertConfig(num_classes=num_classes, **cfg)
    found = pretrained.find_hf_weights("ClassificationBert", hub_name, path)
    if found is not None:
        pretrained.apply_bert_config(found[0], bcfg, found[2])
    m = ClassificationBert(bcfg, device=device)
    m.init_weights(kw.pop("seed", 0))
    if found is not None:
        pretrained.load_hf(m, found[1], "bert", found[2])
    return m


def bert_base_uncased(num_classes=2, **kw):
    return _build(num_classes, kw, hub_name="bert-base-uncased", vocab=30522)


def bert_base_cased(num_classes=2, **kw):
    return _build(num_classes, kw, hub_name="bert-base-cased", vocab=28996)


def bert_tiny_test(num_classes=4, **kw):
    return _build(num_classes, kw, vocab=120, hidden=128, layers=2, heads=2, inter=512, max_pos=64)
