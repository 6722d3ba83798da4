"""ViT backbone engine on libsrhip: forward / backward over a flat parameter block.

Mirrors the reference's ``semilearn/nets/vit/vit.py`` plugin surface (class name, builder names,
``state_dict`` keys, ``{'logits','feat'}`` result dict, ``no_weight_decay`` / ``group_matcher``) but not
its implementation: there is no nn.Module, no autograd.  Parameters, gradients, bf16 operand copies
and Adam moments are each ONE contiguous device buffer (the layout is the reference's
``named_parameters()`` order, so a reference checkpoint maps 1:1), every layer is a short list of
HIP kernel launches, and the backward is hand-written.

Data layout in HBM (B images, N tokens, D channels, M = B*N rows):
  residual stream x         fp32 [M, D]      (in place when nothing is saved for a backward)
  LN output / attn out      bf16 [M, D]      GEMM A-operands
  qkv                       bf16 [M, 3D]     exactly as the qkv Linear writes it; attention indexes heads in place
  MLP hidden                bf16 [M, 4D]
  weights                   bf16 [out, in]   (+ transposed bf16 copies for the dX products)
"""
import math
import os
import types

import numpy as np
import torch

from .. import ops
from .pretrained import load_checkpoint
from .surface import ModuleSurface


class VitConfig:
    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12,
                 num_heads=12, mlp_ratio=4.0, drop_path_rate=0.0, eps=1e-6):
        self.img_size, self.patch_size, self.in_chans, self.num_classes = img_size, patch_size, in_chans, num_classes
        self.embed_dim, self.depth, self.num_heads, self.mlp_ratio = embed_dim, depth, num_heads, mlp_ratio
        self.drop_path_rate, self.eps = drop_path_rate, eps
        assert embed_dim % num_heads == 0 and embed_dim // num_heads == 64, "libsrhip attention is built for head_dim 64"
        assert embed_dim in (128, 384, 768)

    @property
    def num_tokens(self):
        return (self.img_size // self.patch_size) ** 2 + 1

    @property
    def hidden(self):
        return int(self.embed_dim * self.mlp_ratio)


def param_names_shapes(cfg):
    """named_parameters() order of the reference VisionTransformer (vit.py:228-275)."""
    D, Hd, p, C = cfg.embed_dim, cfg.hidden, cfg.patch_size, cfg.num_classes
    out = [("cls_token", (1, 1, D)), ("pos_embed", (1, cfg.num_tokens, D)),
           ("patch_embed.proj.weight", (D, cfg.in_chans, p, p)), ("patch_embed.proj.bias", (D,))]
    for i in range(cfg.depth):
        b = "blocks.%d." % i
        out += [(b + "norm1.weight", (D,)), (b + "norm1.bias", (D,)),
                (b + "attn.qkv.weight", (3 * D, D)), (b + "attn.qkv.bias", (3 * D,)),
                (b + "attn.proj.weight", (D, D)), (b + "attn.proj.bias", (D,)),
                (b + "norm2.weight", (D,)), (b + "norm2.bias", (D,)),
                (b + "mlp.fc1.weight", (Hd, D)), (b + "mlp.fc1.bias", (Hd,)),
                (b + "mlp.fc2.weight", (D, Hd)), (b + "mlp.fc2.bias", (D,))]
    out += [("norm.weight", (D,)), ("norm.bias", (D,)), ("head.weight", (C, D)), ("head.bias", (C,))]
    return out


DW_GROUPS = 3              # layer groups of the weight-gradient launch when a grad_ready_cb is installed (data parallel)
LN_REP = 16                # partial copies of a LayerNorm's dgamma / dbeta in the backward (ops.layernorm_bwd_part)
# Which launches the rows without a backward take (module constants: the tests flip them to compare the fused chain with the launches it replaces)
_FUSED_MLP = True          # LN2 + fc1 + GELU + fc2 + residual as one launch
_FUSED_ATTN = True         # qkv Linear + attention as one launch
_FUSED_PROJ = True         # attention projection + residual inside the fused MLP launch
_FUSED_NEXT_LN = True      # ... which then also writes the next block's norm1 output
# the head reads one row per image (the class token): behind the LAST block's attention the fused proj + MLP launch runs those rows only
_LAST_BLOCK_CLASS_ROWS = True
# stochastic depth skips a dropped branch: the fused attention launch leaves an image whose factor is 0 before its first weight tile
# (srhip_attn_block_fused), and the fused proj + MLP launch takes its rows through a per-forward plan built on the device that sends the
# images whose MLP branch is dropped to tiles that stop after the projection (srhip_vit_droppath_plan, srhip_mlp_fused_proj_planned).
# SRHIP_SKIP_DROPPED=0: the dense launch (the attention early exit is part of the kernel either way)
_SKIP_DROPPED_BRANCHES = os.environ.get("SRHIP_SKIP_DROPPED", "1") != "0"
# the fused kernel owns a CU per 128-row tile for ~90 us whatever the launch size: below ~half a chip of tiles (the 8 inference images of the
# pre-start_timing regime = 17 tiles) LayerNorm + two 64x64-tiled GEMMs spread over all CUs are faster
_FUSED_MLP_MIN_ROWS = 16384


def _fused_mlp(cfg, rows):
    """Whether a no-save launch whose kernel choice is made for ``rows`` rows takes the fused row-streaming MLP (forward_features)."""
    Hd = cfg.hidden
    return cfg.embed_dim == 384 and Hd % 128 == 0 and Hd <= 4096 and rows >= _FUSED_MLP_MIN_ROWS and _FUSED_MLP


def launch_kernels(cfg, n_images, kernels_as_images=None, precision="bf16"):
    """The launch-size-dependent kernel choices of a no-save forward_features over ``n_images`` images (host logic, no launch): two launches
    with equal results here run every row through the same kernels, hence to the same bits.  bf16x3: fixed tiles, nothing depends on the size.
    bf16: the fused / unfused MLP switch and the tile kernel (srhip_gemm_nt_plan at the current run-time settings) of every GEMM launched."""
    if precision == "bf16x3":
        return ("bf16x3",)
    D, N, H, Hd = cfg.embed_dim, cfg.num_tokens, cfg.num_heads, cfg.hidden
    M = n_images * N
    fused = _fused_mlp(cfg, max(M, (kernels_as_images or 0) * N))
    fused_attn = _FUSED_ATTN and ops.attn_block_supported(N, D, H)
    gemms = []
    if cfg.in_chans * cfg.patch_size ** 2 > 64:
        gemms.append((ops.EPI_F32, n_images * (N - 1), D, cfg.in_chans * cfg.patch_size ** 2))
    if not fused_attn:
        gemms.append((ops.EPI_BF16, M, 3 * D, D))
    if not (fused and _FUSED_PROJ):
        gemms.append((ops.EPI_RESID_F32, M, D, D))
    if not fused:
        gemms += [(ops.EPI_GELU_BF16, M, Hd, D), (ops.EPI_RESID_F32, M, D, Hd)]
    return (fused, fused_attn) + tuple(ops.gemm_nt_plan(e, m, n, k) for e, m, n, k in gemms)


def droppath_keep_host(probs, depth, B, seed, cols=None):
    """Host replica of droppath_fill_kernel (csrc/vit_ops.hip): which samples KEEP each block's two branches in the draw of ``seed`` over B columns
    -- bool [depth, 2, B], or [depth, 2, len(cols)] for the columns ``cols`` in that order -- bit for bit the device table's ``!= 0``, with no
    device round trip.  probs: the fp32 per-block drop rates as a host array (the values the device table was made from).
    The kernel: i = (2 * block + branch) * B + col, splitmix64 of seed + 0x9E3779B97F4A7C15 * (i + 1), u = (z >> 40) * 2^-24, keep iff
    p <= 0 or u < 1.0f - p in fp32."""
    p = np.asarray(probs, dtype=np.float32)[:depth]
    col = np.arange(B, dtype=np.int64) if cols is None else np.asarray(cols, dtype=np.int64)
    col = np.where((col < 0) | (col >= B), 0, col)
    i = (np.arange(2 * depth, dtype=np.int64)[:, None] * B + col[None, :]).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) + np.uint64(0x9E3779B97F4A7C15) * (i + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)      # exact: < 2^24 times a power of two
    pp = np.repeat(p, 2)[:, None]
    keep = (pp <= np.float32(0)) | (u < (np.float32(1.0) - pp))
    return keep.reshape(depth, 2, col.shape[0])


class FwdContext:
    """Activations kept by a ``save=True`` forward for the hand-written backward."""
    __slots__ = ("B", "img", "img_index", "dp", "xs", "xmid", "ln1", "ln2", "qkv", "ao", "lse", "pre", "h", "st1", "st2",
                 "feat", "xhat", "rstd", "precision")


class VisionTransformer(ModuleSurface):
    GEMM_WEIGHTS = ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")
    rows_independent = True       # LayerNorm only: a row's outputs do not depend on which other rows share the launch
    scatter_outputs = True        # forward_features(out=...) writes logits / features at the caller's row numbers (no index_copy_)
    droppath_by_cols = True       # make_droppath(cols=...) lays the DropPath table out in the caller's column order (no index_select)
    precise_rows = True           # forward_features(precision="bf16x3"): split-bf16 products, fp32 activations (read_rows_precision)
    precise_grad_rows = True      # forward_features(save=True, precision="bf16x3") + its backward (grad_rows_precision)
    pass_prefix_sharing = True    # forward_features(tree=...): passes that agree on their DropPath draws so far share rows (share_pass_prefixes)
    lazy_transposed = True        # the optimizer only marks the transposed weight copies stale (ensure_transposed)

    def __init__(self, cfg=None, device="cuda", **kw):
        self.cfg = cfg if cfg is not None else VitConfig(**kw)
        cfg = self.cfg
        self.device = torch.device(device)
        self._init_block(param_names_shapes(cfg), align=1, bf16=True)
        self.grad_ready_cb = None          # callable(lo, hi) or None: see backward() / distributed.DataParallel.install_overlap
        # "bf16x3": save=True forwards may run the split-bf16 chain (its fp32 context is ~2.5x the bf16 one per batch size: an explicit opt-in,
        # set by the algorithms from grad_rows_precision)
        self.grad_rows_precision = "bf16"
        self.wT = {}
        for i in range(cfg.depth):
            for w in self.GEMM_WEIGHTS:
                n = "blocks.%d.%s" % (i, w)
                r, c = self.offsets[n][1]
                self.wT[n] = torch.zeros(c, r, dtype=torch.bfloat16, device=self.device)
        self.dp_probs_host = torch.linspace(0, cfg.drop_path_rate, cfg.depth)                # vit.py:247-249
        self.dp_probs = self.dp_probs_host.to(self.device)
        self.last_droppath_seed = None       # 64-bit seed of the latest make_droppath draw (droppath_keep_host replays its decisions)
        self._rng_calls = 0
        self.seed = 0

    def init_weights(self, seed=0):
        """The reference VisionTransformer has no init function: torch defaults -- nn.Linear / Conv2d kaiming_uniform(a = sqrt 5) =
        U(+-1/sqrt(fan_in)) for weight and bias, LayerNorm 1 / 0, cls_token and pos_embed zeros (vit.py:241-244)."""
        g = torch.Generator(device="cpu").manual_seed(seed)
        sd, fan = {}, {}
        for n, s_ in self.names_shapes:
            if n in ("cls_token", "pos_embed"):
                sd[n] = torch.zeros(s_)
            elif "norm" in n.split(".")[-2]:
                sd[n] = torch.ones(s_) if n.endswith("weight") else torch.zeros(s_)
            else:
                if n.endswith("weight"):
                    fan[n[:-7]] = int(torch.Size(s_[1:]).numel())
                bound = 1.0 / (fan[n.rsplit(".", 1)[0]] ** 0.5)
                sd[n] = (torch.rand(s_, generator=g) * 2 - 1) * bound
        self.load_state_dict(sd)

    def transpose_items(self):
        """W [out,in] fp32 -> W^T [in,out] bf16 for all 4*depth GEMM weights (the dX operands of the backward)."""
        items = []
        for n, t in self.wT.items():
            r, c = self.offsets[n][1]
            items.append((self.p(n), True, c, t, r, r, r, c, False))
        return items

    def no_weight_decay(self):
        return {"pos_embed", "cls_token"}

    def make_droppath(self, B, cols=None):
        """timm DropPath scales [depth, 2, B] for one forward (vit.py:148,161); cols (int64 device tensor): only those columns of the draw, in
        that order ([depth, 2, len(cols)])."""
        dp = torch.empty(self.cfg.depth, 2, B if cols is None else cols.numel(), dtype=torch.float32, device=self.device)
        self._rng_calls += 1
        # (under core/stepgraph.py the device seed below is the pushed (seed << 32) + counter at the step start plus the draw number inside the
        # step: the same value)
        self.last_droppath_seed = ((self.seed << 32) + self._rng_calls) & 0xFFFFFFFFFFFFFFFF
        sc = getattr(self, "step_scalars", None)
        if sc is not None:
            # core/stepgraph.py: the step's seed base ((seed << 32) + the draw counter at the start of the step) sits in device memory; this call
            # adds its own number inside the step -- the same 64-bit seed as below, from a launch that can be replayed
            self._step_draws = getattr(self, "_step_draws", 0) + 1
            ops.droppath_fill(dp, self.dp_probs, self.cfg.depth, B, self._step_draws, cols=cols, seed_dev=sc.seed_ptr)
        else:
            ops.droppath_fill(dp, self.dp_probs, self.cfg.depth, B, (self.seed << 32) + self._rng_calls, cols=cols)
        return dp

    def _ctx_buffers(self, B, precision="bf16"):
        """Activation buffers of a save=True forward.  Persistent per batch size (one live context per size), so the
        batched-transpose / grouped-GEMM descriptor tables that point into them are built once.  precision "bf16x3": the same fields, every
        activation fp32 -- a context apart from the bf16 one of the same size, so a captured step allocates nothing and the two modes never
        share a buffer."""
        key = ("ctx" if precision == "bf16" else "ctx3", B)
        if key in self._buf_cache:
            return self._buf_cache[key]
        cfg = self.cfg
        D, N, H, Hd = cfg.embed_dim, cfg.num_tokens, cfg.num_heads, cfg.hidden
        M = B * N
        f32 = torch.float32
        act = torch.bfloat16 if precision == "bf16" else f32         # the GEMM operands among the activations
        mk = lambda shape, dt: [torch.empty(shape, dtype=dt, device=self.device) for _ in range(cfg.depth)]   # noqa: E731
        ctx = FwdContext()
        ctx.precision = precision
        ctx.xs = mk((M, D), f32) + [torch.empty(M, D, dtype=f32, device=self.device)]
        ctx.xmid, ctx.ln1, ctx.ln2 = mk((M, D), f32), mk((M, D), act), mk((M, D), act)
        ctx.qkv, ctx.ao, ctx.pre = mk((M, 3 * D), act), mk((M, D), act), mk((M, Hd), act)
        ctx.h = mk((M, Hd), act)                 # GELU output: the X operand of dW_fc2
        ctx.lse = mk((B, H, N), f32)
        ctx.st1 = [(t[0], t[1]) for t in mk((2, M), f32)]            # (mean, rstd) rows as ready views: indexing costs host time per launch
        ctx.st2 = [(t[0], t[1]) for t in mk((2, M), f32)]
        ctx.xhat = torch.empty(B, D, dtype=f32, device=self.device)
        ctx.rstd = torch.empty(B, dtype=f32, device=self.device)
        self._buf_cache[key] = ctx
        return ctx

    # ---- forward ----------------------------------------------------------------------------------
    def forward_features(self, img, img_index=None, droppath=None, save=False, B=None, buftag="", out=None, precision="bf16",
                         kernels_as_images=None, tree=None):
        """img fp32 [n_img, C, H, W]; img_index int32 [B] (optional gather); droppath fp32 [depth,2,B] or None.
        Returns (logits [B,C], feat [B,D], ctx or None).
        precision="bf16x3": the split-bf16 chain of _forward_x3 instead of the bf16-operand one; with save=True the context keeps fp32
        activations for the split-bf16 backward (grad_rows_precision).
        kernels_as_images: pick the kernels a launch of that many images would take (rows split off a larger launch keep its results bit for bit).
        tree (share_pass_prefixes, rows without a backward, out= required): a pass-prefix tree of the B columns (algorithms/srflexmatch.py
        _PassTree, uploaded): the patch embedding runs once per distinct image (tree.uimg_dev), block i over the tree.level_n[i] nodes of that
        block (their DropPath scales: droppath = tree.dp, [depth, 2, >= max nodes]), new nodes are forked from their parents in front of the
        block (srhip_vit_fork), and every column takes its node's outputs at its row of ``out`` (srhip_vit_fanout).  Every kernel choice is
        made for the unshared launch of B images, so each column's logits and feature are that launch's, bit for bit."""
        if tree is not None:
            assert not save and out is not None, "a pass-prefix tree is for rows without a backward that write the step's tables"
        if precision == "bf16x3":
            if save:
                assert self.grad_rows_precision == "bf16x3", "a bf16x3 forward with saved activations needs model.grad_rows_precision = 'bf16x3'"
            return self._forward_x3(img, img_index, droppath, B, buftag, out, tree, save)
        if precision != "bf16":
            raise ValueError("precision must be 'bf16' or 'bf16x3', got %r" % (precision,))
        cfg = self.cfg
        D, N, H, Hd = cfg.embed_dim, cfg.num_tokens, cfg.num_heads, cfg.hidden
        B = tree.n if tree is not None else (int(img_index.numel()) if img_index is not None else (B or img.shape[0]))
        M = B * N
        Mk = max(M, (kernels_as_images or 0) * N)       # the launch size the kernel choice is made for
        # a tree launches fewer rows per block than the unshared launch: its GEMMs take that launch's tile kernel (srhip_gemm_nt_planned)
        gp = dict(plan_M=M) if tree is not None else {}
        f32, bf16 = torch.float32, torch.bfloat16
        tag = ("s" if save else "i") + buftag        # buftag: a second inference launch train on another stream needs its own workspaces
        ctx = None
        if save:
            ctx = self._ctx_buffers(B)
            ctx.B, ctx.img, ctx.img_index, ctx.dp = B, img, img_index, droppath
            x = ctx.xs[0]
        else:
            x = self._buf(tag + "x", (M, D), f32)
            ln = self._buf(tag + "ln", (M, D), bf16)
            qkv = self._buf(tag + "qkv", (M, 3 * D), bf16)
            ao = self._buf(tag + "ao", (M, D), bf16)
        # rows without a backward run LN2 + fc1 + GELU + fc2 + residual as ONE kernel (ViT-S width; SRHIP_FUSED_MLP=0: off)
        fused_mlp = (not save) and _fused_mlp(cfg, Mk)
        hbuf = None if (fused_mlp or save) else self._buf(tag + "h", (M, Hd), bf16)
        fused_attn = (not save) and _FUSED_ATTN and ops.attn_block_supported(N, D, H)       # SRHIP_FUSED_ATTN=0: separate qkv GEMM + attention
        qkvx = self._buf(tag + "qkvx", (B, 3 * D), bf16) if (fused_attn and N == 257) else None
        wb = self.flat_bf16
        P = self.p
        Be, idx_e = (tree.U, tree.uimg_dev) if tree is not None else (B, img_index)       # the images the patch embedding runs on
        self._patch_embed(img, idx_e, x, Be, B, tag, "bf16", B * (N - 1) if tree is not None else None)
        scale = 64 ** -0.5
        dst0, dst1 = (droppath.stride(0), droppath.stride(1)) if droppath is not None else (0, 0)      # (a column range of the step's table: strided rows)
        ln_ready = False           # the previous block's fused launch already wrote this block's norm1 output
        plan = None
        if _SKIP_DROPPED_BRANCHES and droppath is not None and tree is None and fused_attn and fused_mlp and _FUSED_PROJ:
            # one plan per forward, from the table itself (device memory: nothing here depends on the host knowing the draws)
            plan = self._buf(tag + "dpplan", (cfg.depth, 1 + B), torch.int32)
            ops.vit_droppath_plan(droppath, cfg.depth, B, plan)
        for i in range(cfg.depth):
            b = "blocks.%d." % i
            if tree is not None:
                # this block's nodes: the new ones start as copies of their parents (x, and the norm1 output when the last launch wrote it)
                fk = tree.forks[i]
                if fk is not None:
                    ops.vit_fork(x, ln if ln_ready else None, fk[0], fk[1], fk[2], N, D)
                B = tree.level_n[i]
                M = B * N
                tree.launched.append(B)
            s1 = ops.RawRows(droppath, i * dst0) if droppath is not None else None            # droppath[i, 0], droppath[i, 1] without building views
            s2 = ops.RawRows(droppath, i * dst0 + dst1) if droppath is not None else None
            if save:
                ln, qkv, ao = ctx.ln1[i], ctx.qkv[i], ctx.ao[i]
                ops.layernorm_fwd(x, P(b + "norm1.weight"), P(b + "norm1.bias"), cfg.eps, ln, ctx.st1[i][0], ctx.st1[i][1], M, D)
            elif not ln_ready:
                ops.layernorm_fwd(x, P(b + "norm1.weight"), P(b + "norm1.bias"), cfg.eps, ln, None, None, M, D)
            ao_scaled = False
            if fused_attn:
                # rows without a backward: qkv Linear + attention as ONE launch (one workgroup per image; qkv never reaches HBM)
                # (the DropPath factor of the branch rides on its bf16 output when the fused proj + MLP launch consumes it)
                ao_scaled = fused_mlp and _FUSED_PROJ and s1 is not None
                ops.attn_block_fused(ln, P(b + "attn.qkv.weight", wb), P(b + "attn.qkv.bias"), ao, B, N, D, H, scale, qkv_extra=qkvx,
                                     out_scale=s1 if ao_scaled else None)
            else:
                ops.gemm_nt(ops.EPI_BF16, ln, P(b + "attn.qkv.weight", wb), qkv, M, 3 * D, D, bias=P(b + "attn.qkv.bias"), **gp)
                ops.attn_fwd(qkv, ao, ctx.lse[i] if save else None, B, N, H, scale)
            if save:
                xm = ctx.xmid[i]
                ops.gemm_nt(ops.EPI_RESID_F32, ao, P(b + "attn.proj.weight", wb), xm, M, D, D, bias=P(b + "attn.proj.bias"),
                            row_scale=s1, rows_per_sample=N, aux_in=x, ldaux=D)
                ln2 = ctx.ln2[i]
                ops.layernorm_fwd(xm, P(b + "norm2.weight"), P(b + "norm2.bias"), cfg.eps, ln2, ctx.st2[i][0], ctx.st2[i][1], M, D)
                ops.gemm_nt(ops.EPI_GELU_BF16, ln2, P(b + "mlp.fc1.weight", wb), ctx.h[i], M, Hd, D, bias=P(b + "mlp.fc1.bias"),
                            aux_out=ctx.pre[i], ldaux=Hd)
                xn = ctx.xs[i + 1]
                ops.gemm_nt(ops.EPI_RESID_F32, ctx.h[i], P(b + "mlp.fc2.weight", wb), xn, M, D, Hd, bias=P(b + "mlp.fc2.bias"),
                            row_scale=s2, rows_per_sample=N, aux_in=xm, ldaux=D)
                x = xn
            elif fused_mlp and _FUSED_PROJ:
                # rows without a backward: proj + residual + LN2 + fc1 + GELU + fc2 + residual as ONE launch -- which also writes the NEXT
                # block's norm1 output (the operand of its fused qkv + attention launch) when there is a next block
                nb = "blocks.%d." % (i + 1)
                ln_ready = _FUSED_NEXT_LN and i + 1 < cfg.depth
                # last block: nothing reads its non-class rows of x (_head takes row b * N of image / node b) and a row's values do not depend
                # on the launch that carries it, so row b of the launch = row b * N of x and ao, in place: B rows instead of B * N
                class_rows = _LAST_BLOCK_CLASS_ROWS and i == cfg.depth - 1
                rps, rows, pitch = (1, B, N * D) if class_rows else (N, M, None)
                ops.mlp_fused_proj(x, ao, P(b + "attn.proj.weight", wb), P(b + "attn.proj.bias"), s1, P(b + "norm2.weight"),
                                   P(b + "norm2.bias"), cfg.eps, P(b + "mlp.fc1.weight", wb), P(b + "mlp.fc1.bias"),
                                   P(b + "mlp.fc2.weight", wb), P(b + "mlp.fc2.bias"), s2, rps, rows, D, Hd,
                                   ln_next=ln if ln_ready else None, next_gamma=P(nb + "norm1.weight") if ln_ready else None,
                                   next_beta=P(nb + "norm1.bias") if ln_ready else None, ao_scaled=ao_scaled, row_pitch=pitch,
                                   plan_row=ops.RawRows(plan, i * (1 + B)) if (plan is not None and not class_rows) else None)
            else:
                ops.gemm_nt(ops.EPI_RESID_F32, ao, P(b + "attn.proj.weight", wb), x, M, D, D, bias=P(b + "attn.proj.bias"),
                            row_scale=s1, rows_per_sample=N, **gp)
                if fused_mlp:
                    ops.mlp_fused(x, P(b + "norm2.weight"), P(b + "norm2.bias"), cfg.eps, P(b + "mlp.fc1.weight", wb),
                                  P(b + "mlp.fc1.bias"), P(b + "mlp.fc2.weight", wb), P(b + "mlp.fc2.bias"), s2, N, M, D, Hd)
                else:
                    ops.layernorm_fwd(x, P(b + "norm2.weight"), P(b + "norm2.bias"), cfg.eps, ln, None, None, M, D)
                    ops.gemm_nt(ops.EPI_GELU_BF16, ln, P(b + "mlp.fc1.weight", wb), hbuf, M, Hd, D, bias=P(b + "mlp.fc1.bias"), **gp)
                    ops.gemm_nt(ops.EPI_RESID_F32, hbuf, P(b + "mlp.fc2.weight", wb), x, M, D, Hd, bias=P(b + "mlp.fc2.bias"),
                                row_scale=s2, rows_per_sample=N, **gp)
        return self._head(x, B, out, ctx, tree, tag)

    def _patch_embed(self, img, idx, x, Be, B, tag, precision, plan_M=None):
        """Patch embedding of the ``Be`` images ``idx`` of ``img`` into the residual stream ``x`` (workspaces: those of a launch of B images
        under ``tag``).  plan_M (bf16): the GEMM takes the tile kernel of a launch of that many rows (a pass-prefix tree embeds fewer images
        than the unshared launch; the x3 tile kernels are fixed: no plan to pin)."""
        cfg = self.cfg
        D, Np, Kp = cfg.embed_dim, cfg.num_tokens - 1, cfg.in_chans * cfg.patch_size ** 2
        P = self.p
        if Kp <= 64:                                # CIFAR-style 2x2 / 4x4 patches: direct fp32 kernel (either precision)
            ops.patch_embed_fwd(img, idx, P("patch_embed.proj.weight"), P("patch_embed.proj.bias"), P("cls_token"),
                                P("pos_embed"), x, Be, cfg.in_chans, cfg.img_size, cfg.patch_size, D)
            return
        # ViT-S/16 at 224: unfold -> GEMM with the [D, 768] filter -> + bias / pos / cls
        x3 = precision == "bf16x3"
        col = self._buf(tag + "col", (B * Np, Kp), torch.float32 if x3 else torch.bfloat16)
        tok = self._buf(tag + "tok", (B * Np, D), torch.float32)
        if x3:                                      # fp32 unfold, bf16x3 product with the fp32 filter
            ops.patch_im2col_f32(img, idx, col, Be, cfg.in_chans, cfg.img_size, cfg.patch_size)
            ops.gemm_nt_x3(ops.X3_EPI_F32, col, P("patch_embed.proj.weight"), tok, Be * Np, D, Kp)
        else:
            ops.patch_im2col(img, idx, col, Be, cfg.in_chans, cfg.img_size, cfg.patch_size)
            ops.gemm_nt(ops.EPI_F32, col, P("patch_embed.proj.weight", self.flat_bf16), tok, Be * Np, D, Kp, plan_M=plan_M)
        ops.patch_assemble(tok, P("patch_embed.proj.bias"), P("cls_token"), P("pos_embed"), x, Be, Np, D)

    def _head(self, x, B, out, ctx, tree, tag):
        """Final norm + head over the class rows of the B images (or tree nodes) in ``x``; returns forward_features' triple.
        out = (logits_all, feats_all, rows): the head writes image b's outputs to row rows[b] of the caller's buffers (the step's
        [(pass, image), .] tables) -- no index_copy_ launches behind this forward; the dense outputs are only kept for a backward (``ctx``).
        tree: the head runs over the last block's nodes into dense node tables, then every column's row of the step's tables takes its node's
        outputs (the same head kernel and values as the unshared launch's scatter head)."""
        cfg = self.cfg
        D, N, C = cfg.embed_dim, cfg.num_tokens, cfg.num_classes
        P = self.p
        f32 = torch.float32
        feat = logits = xhat = rstd = None
        if tree is not None:
            feat, logits = self._buf(tag + "tfeat", (tree.n, D), f32), self._buf(tag + "tlogits", (tree.n, C), f32)
        elif ctx is not None or out is None:
            feat, logits = torch.empty(B, D, dtype=f32, device=self.device), torch.empty(B, C, dtype=f32, device=self.device)
        if ctx is not None:
            ctx.feat, xhat, rstd = feat, ctx.xhat, ctx.rstd
        if out is not None and tree is None:
            logits_all, feats_all, rows = out
            ops.cls_head_fwd_scatter(x, P("norm.weight"), P("norm.bias"), cfg.eps, P("head.weight"), P("head.bias"), feat, logits, xhat, rstd,
                                     feats_all, logits_all, rows, B, N, D, C)
        else:
            ops.cls_head_fwd(x, P("norm.weight"), P("norm.bias"), cfg.eps, P("head.weight"), P("head.bias"), feat, logits, xhat, rstd, B, N, D, C)
        if tree is not None:
            logits_all, feats_all, rows = out
            ops.vit_fanout(logits, feat, B, tree.col_node_dev, rows, tree.n, logits_all, feats_all, C, D)
            return None, None, None
        return logits, feat, ctx

    def _forward_x3(self, img, img_index, droppath, B, buftag, out, tree=None, save=False):
        """forward_features in split-bf16 precision (read_rows_precision / grad_rows_precision = bf16x3): every product is hi.hi + hi.lo +
        lo.hi of the bf16 planes of its fp32 operands (csrc/x3.hip), activations stay fp32, LayerNorm / softmax / GELU / residual / head
        in fp32 in the order of vit.py.  The weights are read from the fp32 parameter block.  Own workspaces (tag "p"): the bf16 chain's
        buffers are not touched.  save: the same products and order, every activation kept fp32 in the persistent context of
        _ctx_buffers(B, "bf16x3") (LayerNorm statistics, the fc1 pre-activation, the attention lse) for backward(ctx.precision = "bf16x3")."""
        cfg = self.cfg
        D, N, H, Hd = cfg.embed_dim, cfg.num_tokens, cfg.num_heads, cfg.hidden
        B = tree.n if tree is not None else (int(img_index.numel()) if img_index is not None else (B or img.shape[0]))
        M = B * N
        f32 = torch.float32
        ctx = None
        if save:
            tag = "q"
            ctx = self._ctx_buffers(B, "bf16x3")
            ctx.B, ctx.img, ctx.img_index, ctx.dp = B, img, img_index, droppath
            x = ctx.xs[0]
        else:
            tag = "p" + buftag
            x = self._buf(tag + "x", (M, D), f32)
            ln = ln2 = self._buf(tag + "ln", (M, D), f32)
            ao = self._buf(tag + "ao", (M, D), f32)
            wide = self._buf(tag + "wide", (M * max(3 * D, Hd),), f32)     # qkv [M, 3D], then the MLP hidden [M, Hd] of the same block
            qkv, hbuf = wide[:M * 3 * D].view(M, 3 * D), wide[:M * Hd].view(M, Hd)
            st1 = st2 = (None, None)
        P = self.p
        Be, idx_e = (tree.U, tree.uimg_dev) if tree is not None else (B, img_index)
        self._patch_embed(img, idx_e, x, Be, B, tag, "bf16x3")
        scale = 64 ** -0.5
        dst0, dst1 = (droppath.stride(0), droppath.stride(1)) if droppath is not None else (0, 0)
        for i in range(cfg.depth):
            b = "blocks.%d." % i
            if tree is not None:
                fk = tree.forks[i]
                if fk is not None:
                    ops.vit_fork(x, None, fk[0], fk[1], fk[2], N, D)
                B = tree.level_n[i]
                M = B * N
                tree.launched.append(B)
            s1 = ops.RawRows(droppath, i * dst0) if droppath is not None else None
            s2 = ops.RawRows(droppath, i * dst0 + dst1) if droppath is not None else None
            if save:
                ln, ln2, qkv, ao, hbuf, st1, st2 = ctx.ln1[i], ctx.ln2[i], ctx.qkv[i], ctx.ao[i], ctx.h[i], ctx.st1[i], ctx.st2[i]
            ops.layernorm_fwd_f32(x, P(b + "norm1.weight"), P(b + "norm1.bias"), cfg.eps, ln, st1[0], st1[1], M, D)
            ops.gemm_nt_x3(ops.X3_EPI_F32, ln, P(b + "attn.qkv.weight"), qkv, M, 3 * D, D, bias=P(b + "attn.qkv.bias"))
            if save:
                ops.attn_fwd_x3_lse(qkv, ao, ctx.lse[i], B, N, H, scale)
                xm = ctx.xmid[i]
                xm.copy_(x)                                 # the residual stream of the block input stays for the LayerNorm backward
            else:
                ops.attn_fwd_x3(qkv, ao, B, N, H, scale)
                xm = x                                      # in place when nothing is saved
            ops.gemm_nt_x3(ops.X3_EPI_RESID_F32, ao, P(b + "attn.proj.weight"), xm, M, D, D, bias=P(b + "attn.proj.bias"),
                           row_scale=s1, rows_per_sample=N)
            ops.layernorm_fwd_f32(xm, P(b + "norm2.weight"), P(b + "norm2.bias"), cfg.eps, ln2, st2[0], st2[1], M, D)
            if save:
                ops.gemm_x3(ops.X3B_NT, ops.X3B_EPI_GELU_PRE, ln2, P(b + "mlp.fc1.weight"), hbuf, M, Hd, D, bias=P(b + "mlp.fc1.bias"),
                            aux_out=ctx.pre[i], ldaux=Hd)
                xn = ctx.xs[i + 1]
                xn.copy_(xm)
            else:
                ops.gemm_nt_x3(ops.X3_EPI_GELU_F32, ln2, P(b + "mlp.fc1.weight"), hbuf, M, Hd, D, bias=P(b + "mlp.fc1.bias"))
                xn = xm
            ops.gemm_nt_x3(ops.X3_EPI_RESID_F32, hbuf, P(b + "mlp.fc2.weight"), xn, M, D, Hd, bias=P(b + "mlp.fc2.bias"),
                           row_scale=s2, rows_per_sample=N)
            x = xn
        return self._head(x, B, out, ctx, tree, tag)

    def forward(self, x, only_fc=False, only_feat=False, **kw):
        """Reference-compatible entry (vit.py:285-306): returns {'logits','feat'}.  Inference-style call
        (DropPath active only in train mode, no activations kept)."""
        assert not only_fc, "only_fc is not on the SemiReward hot path"
        dp = self.make_droppath(x.shape[0]) if (self.training and self.cfg.drop_path_rate > 0) else None
        logits, feat, _ = self.forward_features(x.contiguous(), None, dp, save=False)
        return feat if only_feat else {"logits": logits, "feat": feat}

    __call__ = forward

    # ---- backward ---------------------------------------------------------------------------------
    def _bwd_plan(self, M, ctx):
        """Per-layer output-gradient buffers (the A operands of dW = dY^T X, kept until the ONE grouped launch after the layer
        loop) + the descriptor table of that launch (built once per batch size; ``ctx`` buffers are persistent too).
        Operands stay row-major [tokens, features]: srhip_gemm_tn_grouped_f32 gathers the MFMA fragments with LDS transpose
        reads, and sums the bias gradients on the way (no transposes, no column-sum kernels).
        A bf16x3 context: fp32 gradient buffers and the srhip_gemm_tn_x3_grouped table of the same problems."""
        key = ("bwdplan", M, id(ctx))
        if key in self._buf_cache:
            return self._buf_cache[key]
        cfg = self.cfg
        D, Hd = cfg.embed_dim, cfg.hidden
        x3 = ctx.precision == "bf16x3"
        make_desc = ops.make_group_tn_x3_desc if x3 else ops.make_group_tn_desc
        mk = lambda c: torch.empty(M, c, dtype=torch.float32 if x3 else torch.bfloat16, device=self.device)   # noqa: E731
        layers, problems = [], []
        G = lambda n: self.view(n, self.grad)   # noqa: E731
        for i in range(cfg.depth):
            b = "blocks.%d." % i
            t = dict(g2=mk(D), dpre=mk(Hd), g1=mk(D), dqkv=mk(3 * D))
            layers.append(t)
            problems += [(t["g2"], ctx.h[i], G(b + "mlp.fc2.weight"), G(b + "mlp.fc2.bias"), D, Hd, M),
                         (t["dpre"], ctx.ln2[i], G(b + "mlp.fc1.weight"), G(b + "mlp.fc1.bias"), Hd, D, M),
                         (t["g1"], ctx.ao[i], G(b + "attn.proj.weight"), G(b + "attn.proj.bias"), D, D, M),
                         (t["dqkv"], ctx.ln1[i], G(b + "attn.qkv.weight"), G(b + "attn.qkv.bias"), 3 * D, D, M)]
        out = dict(layers=layers, desc=make_desc(problems, self.device))
        # LayerNorm affine gradients: LN_REP partial copies per LayerNorm (same-address atomics of ~500 workgroups serialise), folded into
        # the gradient block by ONE launch after the layer loop.  Order: norm1, norm2 of block 0, 1, ...
        ln_names = lambda lo_l, hi_l: [(G("blocks.%d.norm%d.weight" % (i, j)), G("blocks.%d.norm%d.bias" % (i, j)))   # noqa: E731
                                       for i in range(lo_l, hi_l) for j in (1, 2)]
        out["ln_part"] = torch.zeros(2 * cfg.depth, LN_REP, 2, D, dtype=torch.float32, device=self.device)
        out["ln_desc"] = ops.make_ln_reduce_desc(ln_names(0, cfg.depth), self.device)

        def flat_range(lo_l, hi_l):         # the layers' parameters in the flat block
            names = [n for n, _ in self.names_shapes if n.startswith("blocks.") and lo_l <= int(n.split(".")[1]) < hi_l]
            lo = min(self.offsets[n][0] for n in names)
            hi = max(self.offsets[n][0] + int(torch.Size(self.offsets[n][1]).numel()) for n in names)
            assert sum(int(torch.Size(self.offsets[n][1]).numel()) for n in names) == hi - lo, "block parameters are contiguous in the flat block"
            return lo, hi
        out["flat"] = flat_range(0, cfg.depth)          # the data-parallel hand-over of a chain that launched no group: one whole-range call
        # Data parallel: the same launches cut into DW_GROUPS layer groups (last layers first), so that the all-reduce of a group's slice of the
        # flat gradient block can travel under the backward of the earlier layers (grad_ready_cb, see distributed.py).  (bf16 only.)
        groups = []
        if not x3:
            ng = max(1, min(DW_GROUPS, cfg.depth))
            per = -(-cfg.depth // ng)
            for hi_l in range(cfg.depth, 0, -per):
                lo_l = max(0, hi_l - per)
                groups.append(dict(lo_layer=lo_l, hi_layer=hi_l, flat=flat_range(lo_l, hi_l),
                                   desc=make_desc(problems[4 * lo_l:4 * hi_l], self.device),
                                   ln_desc=ops.make_ln_reduce_desc(ln_names(lo_l, hi_l), self.device)))
        out["groups"] = groups
        self._buf_cache[key] = out
        return out

    def backward(self, ctx, dlogits):
        """Accumulates d(loss)/d(params) into ``self.grad`` given dlogits fp32 [B, C] for a save=True forward (of either precision)."""
        self.backward_rows(ctx, dlogits, 0, ctx.B)
        self.backward_finish(ctx, dlogits)

    def _bwd_views(self, ctx, T, b0, b1):
        """Per-layer operands of the dX chain restricted to the images [b0, b1) (built once per range: a view costs ~3 us of host time).
        The workspaces are per precision (b_* bf16 / fp32, b3_* all fp32): chains of the two precisions never share one."""
        key = ("bwdviews", id(ctx), b0, b1)
        v = self._buf_cache.get(key)
        if v is not None:
            return v
        cfg = self.cfg
        D, N, H = cfg.embed_dim, cfg.num_tokens, cfg.num_heads
        B = ctx.B
        M = B * N
        f32 = torch.float32
        ws, wdt = ("b3_", f32) if ctx.precision == "bf16x3" else ("b_", torch.bfloat16)
        whole = b0 == 0 and b1 == B
        r = (lambda t: t) if whole else (lambda t: t[b0 * N:b1 * N])            # rows of a [M, .] buffer
        im = (lambda t: t) if whole else (lambda t: t[b0:b1])                   # images of a [B, ..] buffer
        v = types.SimpleNamespace()
        v.dx, v.dln, v.dao = r(self._buf(ws + "dx", (M, D), f32)), r(self._buf(ws + "dln", (M, D), wdt)), r(self._buf(ws + "dao", (M, D), wdt))
        v.delta = im(self._buf(ws + "delta", (B, H, N), f32))
        v.xhat, v.rstd = im(ctx.xhat), im(ctx.rstd)
        v.layers = []
        for i in range(cfg.depth):
            Ti = T["layers"][i]
            v.layers.append(types.SimpleNamespace(
                g2=r(Ti["g2"]), dpre=r(Ti["dpre"]), g1=r(Ti["g1"]), dqkv=r(Ti["dqkv"]), pre=r(ctx.pre[i]), xmid=r(ctx.xmid[i]), xs=r(ctx.xs[i]),
                st1=(r(ctx.st1[i][0]), r(ctx.st1[i][1])), st2=(r(ctx.st2[i][0]), r(ctx.st2[i][1])), qkv=r(ctx.qkv[i]), ao=r(ctx.ao[i]),
                lse=im(ctx.lse[i])))
        self._buf_cache[key] = v
        return v

    def backward_rows(self, ctx, dlogits, b0, b1):
        """The input-gradient chain (head -> blocks 11 .. 0) of the images [b0, b1) of a save=True forward: every operand is a row range, rows of
        different images never meet before the weight-gradient products, so disjoint ranges may run on different streams at different times
        (measured in round 5 and not used by the step: profiles/r05_early_sup_backward_ab.txt; backward() runs ONE whole-batch chain).  ``dlogits``
        is the whole [B, C] buffer; only its rows [b0, b1) are read.  LayerNorm / final-norm affine gradients are added with atomics into the
        partial copies; everything that sums over ALL rows -- weight, bias, head and patch-embedding gradients -- is backward_finish.
        A bf16x3 context: the same chain with fp32 gradients, every input-gradient product dY . W a split-bf16 NN product on the fp32
        parameter block (no transposed copies), the attention backward and the LayerNorm backward on fp32 operands."""
        cfg = self.cfg
        D, N, H, Hd, C = cfg.embed_dim, cfg.num_tokens, cfg.num_heads, cfg.hidden, cfg.num_classes
        nb = b1 - b0
        M = nb * N
        P = self.p
        G = lambda n: self.p(n, self.grad)   # noqa: E731
        x3 = ctx.precision == "bf16x3"
        if x3:
            ln_bwd, attn_bwd, NN, X3F = ops.layernorm_bwd_part_f32, ops.attn_bwd_x3, ops.X3B_NN, ops.X3B_EPI_F32
        else:
            ln_bwd, attn_bwd, wT = ops.layernorm_bwd_part, ops.attn_bwd, self.wT
            self.ensure_transposed()
        T = self._bwd_plan(ctx.B * N, ctx)
        v = self._bwd_views(ctx, T, b0, b1)
        dl = dlogits if (b0 == 0 and b1 == ctx.B) else dlogits[b0:b1]
        v.dx.zero_()
        ops.cls_head_bwd(dl, P("head.weight"), P("norm.weight"), None, v.xhat, v.rstd, v.dx, None, None, G("norm.weight"), G("norm.bias"),
                         nb, N, D, C)
        scale = 64 ** -0.5
        dp = ctx.dp
        lnp = T["ln_part"]
        cb = self.grad_ready_cb if (b0 == 0 and b1 == ctx.B and not x3) else None   # data parallel overlap: whole-batch bf16 chains only
        self._groups_launched = cb is not None         # backward_finish: the layer groups' weight / LayerNorm launches already ran inside this chain
        gdone = {g["lo_layer"]: g for g in T["groups"]} if cb is not None else {}
        # dp[i, j, b0:] as a raw pointer (the DropPath factors of this range's images)
        dpr = (lambda i_, j_: ops.RawRows(dp, i_ * dp.stride(0) + j_ * dp.stride(1) + b0)) if dp is not None else (lambda i_, j_: None)
        L = v.layers
        (ops.scale_rows_f32 if x3 else ops.cast_scale_rows)(v.dx, dpr(cfg.depth - 1, 1), N, L[cfg.depth - 1].g2, M, D)
        for i in reversed(range(cfg.depth)):
            b = "blocks.%d." % i
            Li = L[i]
            s1 = dpr(i, 0)
            # ---- MLP branch: x_out = x_mid + s2 * fc2(gelu(fc1(ln2(x_mid))));  g2 = s2 * dx came from the previous LayerNorm backward;
            # dpre = (g2 . W_fc2) * gelu'(pre); dln2 = dpre . W_fc1
            if x3:
                ops.gemm_x3(NN, ops.X3B_EPI_DGELU, Li.g2, P(b + "mlp.fc2.weight"), Li.dpre, M, Hd, D, aux=Li.pre, ldaux=Hd)
                ops.gemm_x3(NN, X3F, Li.dpre, P(b + "mlp.fc1.weight"), v.dln, M, D, Hd)
            else:
                ops.gemm_nt(ops.EPI_DGELU_BF16, Li.g2, wT[b + "mlp.fc2.weight"], Li.dpre, M, Hd, D, aux_in=Li.pre, ldaux=Hd)
                ops.gemm_nt(ops.EPI_BF16, Li.dpre, wT[b + "mlp.fc1.weight"], v.dln, M, D, Hd)
            ln_bwd(v.dln, Li.xmid, Li.st2[0], Li.st2[1], P(b + "norm2.weight"), v.dx, lnp[2 * i + 1], LN_REP, Li.g1, s1, N, M, D)
            # ---- attention branch: x_mid = x_in + s1 * proj(attn(qkv(ln1(x_in))));  g1 = s1 * dx; dao = g1 . W_proj; dqkv; dln1 = dqkv . W_qkv
            if x3:
                ops.gemm_x3(NN, X3F, Li.g1, P(b + "attn.proj.weight"), v.dao, M, D, D)
            else:
                ops.gemm_nt(ops.EPI_BF16, Li.g1, wT[b + "attn.proj.weight"], v.dao, M, D, D)
            attn_bwd(Li.qkv, Li.ao, v.dao, Li.lse, Li.dqkv, v.delta, nb, N, H, scale)
            if x3:
                ops.gemm_x3(NN, X3F, Li.dqkv, P(b + "attn.qkv.weight"), v.dln, M, D, 3 * D)
            else:
                ops.gemm_nt(ops.EPI_BF16, Li.dqkv, wT[b + "attn.qkv.weight"], v.dln, M, D, 3 * D)
            ln_bwd(v.dln, Li.xs, Li.st1[0], Li.st1[1], P(b + "norm1.weight"), v.dx, lnp[2 * i], LN_REP,
                   L[i - 1].g2 if i > 0 else None, dpr(i - 1, 1) if i > 0 else None, N, M, D)
            g = gdone.get(i)
            if g is not None:               # layers [i, g.hi_layer) are finished: their weight / bias / LayerNorm gradients, then the hand-over
                desc, npb, ntiles, flops, nbytes = g["desc"]
                ops.gemm_tn_grouped_f32(desc, npb, ntiles, alpha=1.0, beta=1.0, flops=flops, nbytes=nbytes)
                ops.ln_grad_reduce(g["ln_desc"], lnp[2 * g["lo_layer"]:2 * g["hi_layer"]], 2 * (g["hi_layer"] - g["lo_layer"]), LN_REP, D)
                cb(*g["flat"])

    def backward_finish(self, ctx, dlogits):
        """Everything of the backward that sums over ALL rows, after the chain(s) of backward_rows have covered every image: head weight / bias
        gradients, the LayerNorm partial copies folded into the gradient block, all 4 * depth weight (and bias) gradients in ONE grouped
        launch (dW += dY^T X, db += colsum dY; srhip_gemm_tn_x3_grouped for a bf16x3 context), the data-parallel hand-over of the blocks'
        range when the chain did not hand it over in groups, the patch embedding."""
        cfg = self.cfg
        D, N, C = cfg.embed_dim, cfg.num_tokens, cfg.num_classes
        B = ctx.B
        M = B * N
        f32 = torch.float32
        G = lambda n: self.p(n, self.grad)   # noqa: E731
        x3 = ctx.precision == "bf16x3"
        T = self._bwd_plan(M, ctx)
        dx = self._buf("b3_dx" if x3 else "b_dx", (M, D), f32)
        small_pe = cfg.in_chans * cfg.patch_size ** 2 <= 64    # the two-stage patch-embedding kernels (one thread per feature, the patch in LDS)
        ws = self._buf("b_pe_ws", (ops.patch_embed_bwd_ws_floats(B, cfg.in_chans, cfg.img_size, cfg.patch_size, D),), f32) if small_pe else None
        # (a partial-range chain never launches the groups, callback or not; nor does a bf16x3 chain)
        groups_launched = not x3 and getattr(self, "_groups_launched", False)
        # One launch for the blocks' weight gradients AND the small sums over all rows (head weight, LayerNorm copies, dpos / dcls, stage 1 of the
        # patch-embedding gradient): they ran as latency-bound launches around the product, on the step's own stream with nothing beside them;
        # as extra workgroups they fill the slots the product's last round of tiles leaves empty.  (Not under the per-launch profiler, which times
        # the product alone -- DESIGN.md section 7 -- nor for a table with a slab phase, nor for the x3 product.)
        merged = not x3 and not groups_launched and ops._PROFILE is None and getattr(T["desc"][0], "reduce", None) is None
        desc, npb, ntiles, flops, nbytes = T["desc"]
        if merged:
            pe = (dx, ctx.img, ctx.img_index, G("pos_embed"), G("cls_token"), ws, B, cfg.in_chans, cfg.img_size, cfg.patch_size) if small_pe else None
            ops.gemm_tn_grouped_tail_f32(desc, npb, ntiles, D, ln=(T["ln_desc"], T["ln_part"], 2 * cfg.depth, LN_REP),
                                         head=(dlogits, ctx.feat, G("head.weight"), G("head.bias"), B, C), pe=pe)
        else:
            ops.cls_head_bwd(dlogits, None, None, ctx.feat, None, None, None, G("head.weight"), G("head.bias"), None, None, B, N, D, C)
            if not groups_launched:
                ops.ln_grad_reduce(T["ln_desc"], T["ln_part"], 2 * cfg.depth, LN_REP, D)
                if x3:
                    ops.gemm_tn_x3_grouped(desc, npb, ntiles, flops=flops, nbytes=nbytes)
                else:
                    ops.gemm_tn_grouped_f32(desc, npb, ntiles, alpha=1.0, beta=1.0, flops=flops, nbytes=nbytes)
        if not groups_launched and self.grad_ready_cb is not None:
            self.grad_ready_cb(*T["flat"])              # the blocks' range in one piece (the chain did not hand it over in groups)
        self._groups_launched = False
        # dpos / dcls and stage 1 rode in the merged launch: only the fold is left
        self._patch_embed_bwd(ctx, dx, ws, x3, part_done=merged)

    def _patch_embed_bwd(self, ctx, dx, ws, x3, part_done):
        """Patch-embedding gradients from the residual stream's gradient ``dx``: the workspace kernels (``ws``; part_done: see
        ops.patch_embed_bwd_ws), else dWp += dx_tok^T col, dbp += colsum dx_tok as a one-problem TN grouped GEMM (operands and table built
        once per batch size and precision) behind the dpos / dcls launch."""
        cfg = self.cfg
        D, Np, B = cfg.embed_dim, cfg.num_tokens - 1, ctx.B
        G = lambda n: self.p(n, self.grad)   # noqa: E731
        if ws is not None:
            ops.patch_embed_bwd_ws(dx, ctx.img, ctx.img_index, G("patch_embed.proj.weight"), G("patch_embed.proj.bias"), G("cls_token"),
                                   G("pos_embed"), ws, B, cfg.in_chans, cfg.img_size, cfg.patch_size, D, part_done)
            return
        key = ("pebwd3" if x3 else "pebwd", B)
        if key not in self._buf_cache:
            Kp = cfg.in_chans * cfg.patch_size ** 2
            dt = torch.float32 if x3 else torch.bfloat16
            col = torch.empty(B * Np, Kp, dtype=dt, device=self.device)
            dxt = torch.empty(B * Np, D, dtype=dt, device=self.device)
            gw = self.view("patch_embed.proj.weight", self.grad).view(D, Kp)
            problem = [(dxt, col, gw, self.view("patch_embed.proj.bias", self.grad), D, Kp, B * Np)]
            self._buf_cache[key] = (col, dxt, (ops.make_group_tn_x3_desc if x3 else ops.make_group_tn_desc)(problem, self.device))
        col, dxt, desc = self._buf_cache[key]
        if x3:
            ops.patch_im2col_f32(ctx.img, ctx.img_index, col, B, cfg.in_chans, cfg.img_size, cfg.patch_size)
            ops.patch_grad_operands_f32(dx, dxt, G("pos_embed"), G("cls_token"), B, Np, D)
            ops.gemm_tn_x3_grouped(desc[0], desc[1], desc[2], flops=desc[3], nbytes=desc[4])
        else:
            ops.patch_im2col(ctx.img, ctx.img_index, col, B, cfg.in_chans, cfg.img_size, cfg.patch_size)
            ops.patch_grad_operands(dx, dxt, G("pos_embed"), G("cls_token"), B, Np, D)
            ops.gemm_tn_grouped_f32(desc[0], desc[1], desc[2], alpha=1.0, beta=1.0, flops=desc[3], nbytes=desc[4])


# ---- builders with the reference's names (vit.py:323-408); pretrained=True loads pretrained_path as the reference's load_checkpoint does ----
def _build(num_classes, kw, **cfg):
    kw = dict(kw)
    pretrained, path = kw.pop("pretrained", False), kw.pop("pretrained_path", None)
    device = kw.pop("device", "cuda")
    m = VisionTransformer(VitConfig(num_classes=num_classes, **cfg), device=device)
    m.init_weights(kw.pop("seed", 0))
    if pretrained:
        load_checkpoint(m, path)          # a file or the torch-hub cache entry of the URL; not found: random init + one warning line
    return m


def vit_tiny_test(num_classes=10, **kw):
    return _build(num_classes, kw, img_size=8, patch_size=2, embed_dim=128, depth=2, num_heads=2, drop_path_rate=0.2)


def vit_small_patch16_224(num_classes=1000, **kw):
    """vit.py:358-371: ViT-S/16, 197 tokens."""
    return _build(num_classes, kw, img_size=224, patch_size=16, embed_dim=384, depth=12, num_heads=6, drop_path_rate=0.2)


def vit_base_patch16_96(num_classes=1000, **kw):
    """vit.py:374-390: ViT-B/16 on 96x96 images, 37 tokens (the stl10 / eurosat-style usb_cv configs)."""
    return _build(num_classes, kw, img_size=96, patch_size=16, embed_dim=768, depth=12, num_heads=12, drop_path_rate=0.2)


def vit_small_patch2_32(num_classes=1000, **kw):
    return _build(num_classes, kw, img_size=32, patch_size=2, embed_dim=384, depth=12, num_heads=6, drop_path_rate=0.2)


