"""WideResNet on the HIP kernels (classic_cv backbone: ``wrn_28_2``), reference semilearn/nets/wrn/wrn.py.

This is the CPU-reference PARITY configuration of BASELINE.json (configs[0]: CIFAR-100 WRN-28-2 PseudoLabel + SemiReward).  Feature maps
are NHWC = row-major [B*H*W, C].  Forward: ONE launch per BasicBlock convolution (csrc/wrn_conv.hip): the convolution reads its fp32 input
through the BatchNorm + LeakyReLU in front of it (implicit GEMM, no im2col, no separate normalisation pass) and its epilogue leaves mean /
invstd / running statistics of the BatchNorm behind it -- SRPseudoLabel runs this forward K + 1 >= 9 times per step.  Backward (two of those
forwards have one): the bf16 activation and its im2col are recomputed from the kept fp32 tensors; a filter gradient is one problem (K slices)
of the grouped TN GEMM, an input gradient a GEMM with the transposed filter + col2im; BatchNorm backward is a statistics pass + an apply pass.
Parameter names / order, BatchNorm buffers and state_dict keys are the reference's.

BatchNorm semantics (wrn.py:32-38, core/utils/misc.py:105-129): every forward in training mode normalises with the statistics of
ITS OWN batch, so -- unlike the ViT engine -- the passes of a step cannot be batched into one launch train; ``update_stats=False``
is Bn_Controller.freeze_bn ... unfreeze_bn (running statistics untouched).
"""
import torch

from .. import ops
from .pretrained import load_checkpoint
from .surface import ModuleSurface

MOMENTUM, SLOPE = 0.001, 0.1
# Filter gradients (32 x 288 .. 128 x 1152 outputs over 8 192 .. 131 072 pixels) are sliced along the pixel axis to fill the chip; the slices write
# scratch slabs of their own that one reduce launch adds into the gradients: the sums no longer depend on the order fp32 atomics arrive in, and
# slices of 4 096 pixels measured best once the descriptor lookup was a binary search (profiles/r06_wrn_dw_slices_ab.txt).
_DW_SPLIT = 4096
_DW_SLABS = True
_FUSED_DX = True      # input gradients of the stride-1 3x3 layers as implicit-GEMM convolutions with the rotated / transposed filter


def _round_up(a, b):
    return (a + b - 1) // b * b


class WrnContext:
    """Activations of one ``save=True`` forward."""
    __slots__ = ("B", "H", "W", "stem", "blocks", "final", "feat", "tag")


class WideResNet(ModuleSurface):
    couples_batch_rows = True     # BatchNorm: every forward call is its own statistics group (no cross-pass batching)

    def __init__(self, num_classes, depth=28, widen_factor=2, first_stride=1, device="cuda", **kw):
        assert (depth - 4) % 6 == 0
        self.num_classes, self.depth, self.widen, self.first_stride = num_classes, depth, widen_factor, first_stride
        self.device = torch.device(device)
        ch = [16, 16 * widen_factor, 32 * widen_factor, 64 * widen_factor]
        self.channels, self.num_features = ch, ch[3]
        n = (depth - 4) // 6
        self.blocks = []
        for g, stride in enumerate((first_stride, 2, 2)):
            for i in range(n):
                self.blocks.append(("block%d.layer.%d." % (g + 1, i), ch[g] if i == 0 else ch[g + 1], ch[g + 1], stride if i == 0 else 1, g == 0))
        s = [("conv1.weight", (ch[0], 3, 3, 3)), ("conv1.bias", (ch[0],))]
        for p, cin, cout, stride, _ in self.blocks:
            s += [(p + "bn1.weight", (cin,)), (p + "bn1.bias", (cin,)), (p + "conv1.weight", (cout, cin, 3, 3)),
                  (p + "bn2.weight", (cout,)), (p + "bn2.bias", (cout,)), (p + "conv2.weight", (cout, cout, 3, 3))]
            if cin != cout:
                s.append((p + "convShortcut.weight", (cout, cin, 1, 1)))
        s += [("bn1.weight", (ch[3],)), ("bn1.bias", (ch[3],)), ("classifier.weight", (num_classes, ch[3])), ("classifier.bias", (num_classes,))]
        self._init_block(s, align=4, bf16=False)          # 16-byte aligned starts (TN GEMM writes dW in place)
        f32 = torch.float32
        self.bn = [(p + "bn1", cin, 1e-5) for p, cin, _, _, _ in self.blocks]       # forward order is interleaved; names only matter
        self.bn = []
        for p, cin, cout, _, _ in self.blocks:
            self.bn += [(p + "bn1", cin, 1e-5), (p + "bn2", cout, 1e-5)]
        self.bn.append(("bn1", ch[3], 1e-3))
        for nme, c, _ in self.bn:
            self.buffers[nme + ".running_mean"] = torch.zeros(c, dtype=f32, device=self.device)
            self.buffers[nme + ".running_var"] = torch.ones(c, dtype=f32, device=self.device)
            self.buffers[nme + ".num_batches_tracked"] = None         # (views of one int64 block, below)
        # every BatchNorm is visited exactly once by a forward, so the 25 counters move together: one block, one add per updating forward
        self._nbt = torch.zeros(len(self.bn), dtype=torch.int64, device=self.device)
        for i, (nme, _, _) in enumerate(self.bn):
            self.buffers[nme + ".num_batches_tracked"] = self._nbt[i]
        self.eps = {nme: e for nme, _, e in self.bn}
        # bf16 GEMM operands of every convolution: W [Cout, Kpad] and W^T [Kpad, Cout]
        self.convs = {}
        for nme, shp in s:
            if len(shp) == 4:
                cout, cin, k, _ = shp
                K = cin * k * k
                Kp = _round_up(K, 32)
                self.convs[nme] = dict(cout=cout, cin=cin, k=k, K=K, Kp=Kp,
                                       Wb=torch.zeros(cout, Kp, dtype=torch.bfloat16, device=self.device),
                                       WbT=torch.zeros(Kp, cout, dtype=torch.bfloat16, device=self.device))
        # Every block convolution runs as srhip_wrn_conv_bn and the tail as srhip_wrn_head (no generic fall-back chain): refuse at construction,
        # with the reason, the widths those launches are not built for (e.g. widen_factor 4: block3 has Cin = 256; the reference's wrn_28_8 /
        # wrn_var_37_2, which no config/SemiReward yaml names) instead of failing with SR_EINVAL in the middle of a forward.
        bad = ["%s [Cout %d, Cin %d, %dx%d]" % (nme, c["cout"], c["cin"], c["k"], c["k"]) for nme, c in self.convs.items()
               if nme != "conv1.weight" and not ops.wrn_conv_supported(c["cin"], c["cout"], c["k"])]
        if bad or ch[3] > 256:
            raise NotImplementedError(
                "WideResNet(depth=%d, widen_factor=%d): the fused convolution launches (csrc/wrn_conv.hip) take Cin a power of two in 8..128 and "
                "Cout in {16, 32, 64 k <= 256}, the tail launch (wrn_head_kernel) at most 256 channels; not supported here: %s" % (
                    depth, widen_factor, ", ".join(bad) or "final width %d" % ch[3]))
        self.ws = torch.zeros(ops.bn_ws_doubles(), dtype=torch.float64, device=self.device)      # (zeroed once: srhip_bn_fwd keeps its counter at 0)
        # per-BatchNorm statistics accumulators (16 copies x (sum | sum of squares)), filled by the convolution in front of the BatchNorm and
        # folded by the one behind it; one arena so that a forward zeroes them with one launch
        # Data parallel: two more doubles ride behind the FIRST accumulator a forward exchanges -- (rows, ranks * rows^2) of this rank -- so the
        # per-rank row counts are compared by the all-reduce that is issued anyway (_sync_acc / check_equal_rows): no collective of its own.
        offs, o = {}, 0
        first = self.blocks[0][0] + "bn1"
        for nme, c, _ in self.bn:
            offs[nme] = (o, ops.bn_acc_doubles(c))
            o += ops.bn_acc_doubles(c) + (2 if nme == first else 0)
        self.bn_acc_arena = torch.zeros(o, dtype=torch.float64, device=self.device)
        self.bn_acc = {nme: self.bn_acc_arena[a:a + n] for nme, (a, n) in offs.items()}
        a_, n_ = offs[first]
        self._acc_first_with_rows = self.bn_acc_arena[a_:a_ + n_ + 2]
        self._rows_cell = self.bn_acc_arena[a_ + n_:a_ + n_ + 2]
        self._rows_const, self._rows_dev, self._rows_tmp = {}, None, None
        self._prep_desc = None
        self._flip_desc = None
        self.conv_stride = {"conv1.weight": 1}
        for p_, _, _, st_, _ in self.blocks:
            self.conv_stride.update({p_ + "conv1.weight": st_, p_ + "conv2.weight": 1, p_ + "convShortcut.weight": st_})

    def init_weights(self, seed=0):
        """wrn.py:108-117: Conv2d kaiming_normal(fan_out, leaky_relu: gain sqrt(2 / (1 + 0.01^2))), BatchNorm 1 / 0, Linear xavier_normal
        with zero bias; conv1.bias keeps torch's default U(+-1/sqrt(fan_in))."""
        g = torch.Generator(device="cpu").manual_seed(seed)
        sd = {}
        for n, s_ in self.names_shapes:
            if len(s_) == 4:
                fan_out = s_[0] * s_[2] * s_[3]
                sd[n] = torch.randn(s_, generator=g) * ((2.0 / (1.0 + 0.01 ** 2)) ** 0.5 / fan_out ** 0.5)
            elif len(s_) == 2:
                sd[n] = torch.randn(s_, generator=g) * (2.0 / (s_[0] + s_[1])) ** 0.5
            elif ".bn" in n or n.startswith("bn"):
                sd[n] = torch.ones(s_) if n.endswith("weight") else torch.zeros(s_)
            elif n == "conv1.bias":
                sd[n] = (torch.rand(s_, generator=g) * 2 - 1) / 27 ** 0.5
            else:
                sd[n] = torch.zeros(s_)
        self.load_state_dict(sd, strict=False)

    def refresh_operands(self):
        """bf16 operands of every convolution from the fp32 parameters: one grouped launch (28 separate ones were 0.15 ms per step)."""
        if self._prep_desc is None:
            self._prep_desc = ops.make_conv_desc([(self.p(n), c["Wb"], c["WbT"], c["cout"], c["cin"], c["k"], c["Kp"]) for n, c in self.convs.items()],
                                                 self.device, lambda Cout, C, kk, Kpad: Cout * Kpad)
        ops.conv_weight_prep_grouped(*self._prep_desc)
        if self._flip_desc is None:        # stride-1 3x3 layers: the input gradient is one more implicit-GEMM convolution (filter rotated / transposed)
            ent = []
            for n, c in self.convs.items():
                if c["k"] == 3 and self.conv_stride.get(n, 1) == 1 and ops.wrn_conv_supported(c["cout"], c["cin"], 3):
                    c["Kp2"] = _round_up(9 * c["cout"], 32)
                    c["Wfl"] = torch.zeros(c["cin"], c["Kp2"], dtype=torch.bfloat16, device=self.device)
                    ent.append((self.p(n), c["Wfl"], None, c["cout"], c["cin"], 3, c["Kp2"]))
            self._flip_desc = ops.make_conv_desc(ent, self.device, lambda Cout, C, kk, Kpad: C * Kpad) if ent else ()
        if self._flip_desc:
            ops.conv_weight_flip_grouped(*self._flip_desc)

    def no_weight_decay(self):
        return [n for n, _ in self.names_shapes if "bn" in n or "bias" in n]            # wrn.py:143-148

    # ---- forward ----------------------------------------------------------------------------------------------------------------
    def _conv(self, name, act, B, H, W, stride, out, tag, bias=None, resid=None):
        """act bf16 NHWC [B,H,W,Cin] -> out fp32 [B*Ho*Wo, Cout] (= resid + conv when resid is given).  Returns (col, Ho, Wo)."""
        c = self.convs[name]
        k = c["k"]
        pad = k // 2
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        rows = B * Ho * Wo
        col = self._buf((tag, name, "col"), (rows, c["Kp"]), torch.bfloat16)
        ops.im2col(act, col, B, H, W, c["cin"], k, stride, c["Kp"])
        if resid is None:
            ops.gemm_nt(ops.EPI_F32, col, c["Wb"], out, rows, c["cout"], c["Kp"], bias=bias)
        else:
            ops.gemm_nt(ops.EPI_RESID_F32, col, c["Wb"], out, rows, c["cout"], c["Kp"], bias=bias, aux_in=resid, ldaux=c["cout"])
        return col, Ho, Wo

    # ---- one launch per convolution (csrc/wrn_conv.hip) ------------------------------------------------------------------------------
    def _stats_bufs(self, name, C, tag, passes=1):
        shape = (C,) if passes == 1 else (passes, C)
        return (self._buf((tag, name, "mean"), shape, torch.float32), self._buf((tag, name, "invstd"), shape, torch.float32))

    # SyncBatchNorm.  Under DDP the reference converts every BatchNorm of this backbone (core/utils/misc.py:55): in training mode the batch
    # statistics are those of ALL ranks' rows.  Statistics are sums here, so the ranks exchange the accumulator of a BatchNorm between the
    # launch that fills it and the launch that folds it, and the backward exchanges its two column sums between reduce and apply -- one small
    # all-reduce per BatchNorm per pass, as torch's SyncBatchNorm does.  ``dp`` is set by the algorithm (core/algorithmbase.py).
    dp = None

    @property
    def stat_ranks(self):
        return self.dp.world_size if (self.dp is not None and self.dp.active) else 1

    @property
    def stat_sync(self):
        """The statistics are exchanged (data parallel engaged -- also with ONE rank forced through it: distributed.DataParallel.force)."""
        return self.dp is not None and self.dp.active

    def _sync_acc(self, bn, acc=None):
        if self.stat_sync:
            import torch.distributed as dist
            dist.all_reduce((acc or self.bn_acc)[bn])

    def _pass_acc(self, passes):
        """Statistics accumulators of ``passes`` forwards that share their launches (forward_features(passes=...)): per BatchNorm a contiguous
        [passes, srhip_bn_acc_doubles(C)] block (the layout srhip_wrn_conv_bn_passes indexes by blockIdx.z), all in one arena that a forward
        zeroes with one fill launch.  The arena starts with the two row-count cells of the SyncBatchNorm check, directly in front of the FIRST
        BatchNorm's block: cells + block are one contiguous range, so the counts ride on that block's exchange exactly as on the single-pass
        path (_sync_first_acc).  Returns (arena, {name: [passes, n] view}, cells, cells + first block)."""
        key = ("pass_acc", passes)
        if key not in self._buf_cache:
            first = self.blocks[0][0] + "bn1"
            sizes = [(nme, ops.bn_acc_doubles(c)) for nme, c, _ in self.bn]
            sizes = [e for e in sizes if e[0] == first] + [e for e in sizes if e[0] != first]
            arena = torch.zeros(2 + passes * sum(n for _, n in sizes), dtype=torch.float64, device=self.device)
            views, o = {}, 2
            for nme, n in sizes:
                views[nme] = arena[o:o + passes * n].view(passes, n)
                o += passes * n
            self._buf_cache[key] = (arena, views, arena[:2], arena[:2 + passes * sizes[0][1]])
        return self._buf_cache[key]

    def _sync_first_acc(self, B, cell=None, acc_with_rows=None):
        """The exchange of the first accumulator of a training forward, with this rank's row count riding along.  The statistics are sums over
        rows and the kernels divide by rows * ranks (torch's SyncBatchNorm exchanges the counts as well), so every rank must forward the same
        number of images.  EVERY rank enters the SAME collective in EVERY training forward -- whether the counts agree is decided from its
        result ON THE DEVICE (sum B and ranks * sum B^2: equal rows <=> ranks * sum B^2 == (sum B)^2), accumulated into a flag the host
        reads where it may wait (check_equal_rows: AlgorithmBase.train at the logging cadence and before a checkpoint; every forward in the
        test suite).  A rank-local decision to enter a collective of its own (a per-batch-size cache) would pair that collective with another
        rank's next statistics exchange when the counts DO differ -- a hang instead of the error."""
        import torch.distributed as dist
        R = self.stat_ranks
        c = self._rows_const.get((B, R))
        if c is None:
            c = self._rows_const[(B, R)] = torch.tensor([float(B), float(R) * B * B], dtype=torch.float64, device=self.device)
            if self._rows_dev is None:
                self._rows_dev = torch.zeros((), dtype=torch.float64, device=self.device)
                self._rows_tmp = torch.zeros((), dtype=torch.float64, device=self.device)
        cell = self._rows_cell if cell is None else cell                    # (shared-launch forwards: the cells of their own arena, _pass_acc)
        cell.copy_(c)
        dist.all_reduce(self._acc_first_with_rows if acc_with_rows is None else acc_with_rows)
        torch.addcmul(cell[1], cell[0], cell[0], value=-1.0, out=self._rows_tmp)      # R sum B^2 - (sum B)^2 >= 0
        torch.maximum(self._rows_dev, self._rows_tmp, out=self._rows_dev)
        if ops._CHECK_ARGS and not torch.cuda.is_current_stream_capturing():
            self.check_equal_rows()

    def check_equal_rows(self):
        """Raises if any training forward since the last call saw different per-rank batch sizes (synchronises: one scalar read)."""
        if self._rows_dev is not None and float(self._rows_dev) > 0.5:
            self._rows_dev.zero_()
            raise RuntimeError("WideResNet under data parallel (SyncBatchNorm): the per-rank batches of a training forward differed; the statistics "
                               "exchange assumes equal row counts on every rank (a last partial batch or an uneven split)")

    def _conv_bn(self, wname, xin, in_bn, raw, B, H, W, stride, out, tag, train, update, resid=None, next_bn=None, publish=False, passes=1,
                 accs=None, chain=None):
        """out = conv(LeakyReLU(BN_in(xin))) (+ resid) -- or conv(xin) when ``raw`` -- and, in training mode, the sums of ``out`` added into the
        accumulator of ``next_bn`` (then exchanged between the ranks).  Training mode folds in_bn's statistics from its accumulator; ``publish``:
        this launch also writes in_bn's (mean, invstd) for the backward and moves its running statistics.  Returns in_bn's statistics buffers
        (None in eval mode).  ``chain``: a list that collects (BatchNorm, channels, statistics rows) of the publishing launches for
        _running_chain."""
        c = self.convs[wname]
        P = self.p
        g, bt, eps = P(in_bn + ".weight"), P(in_bn + ".bias"), self.eps[in_bn]
        accs = accs if accs is not None else self.bn_acc
        acc_out = accs[next_bn] if (next_bn is not None and train) else None
        if not train:
            stats, acc, mode, pub, st = (self.buffers[in_bn + ".running_mean"], self.buffers[in_bn + ".running_var"]), None, 1, None, None
        else:
            stats, acc, mode = None, accs[in_bn], 3
            st = self._stats_bufs(in_bn, c["cin"], tag, passes)
            pub = st if publish else None
        if raw:
            mode = 2
        ops.wrn_conv_bn(xin, mode, stats, acc, g, bt, eps, SLOPE, c["Wb"], resid, out, B, H, W, c["cin"], c["cout"], c["k"], stride, c["Kp"],
                        publish=pub, running=(self.buffers[in_bn + ".running_mean"], self.buffers[in_bn + ".running_var"]) if pub else None,
                        momentum=MOMENTUM, update_running=update, acc_out=acc_out, stat_ranks=self.stat_ranks, passes=passes)
        if pub and chain is not None:
            chain.append((in_bn, c["cin"], B * H * W * self.stat_ranks))
        if acc_out is not None:
            self._sync_acc(next_bn, accs)
        return st

    def _running_chain(self, chain, accs, G, tag):
        """All G statistics groups of a shared-launch forward move the running statistics, in pass order: one launch over a table of this
        forward's BatchNorms (ops.bn_running_chain), enqueued behind the forward -- every accumulator is complete (and exchanged) by then."""
        key = ("bn_chain", tag, G)
        sig = tuple((n, C, rows, int(accs[n].data_ptr()), int(self.buffers[n + ".running_mean"].data_ptr()),
                     int(self.buffers[n + ".running_var"].data_ptr())) for n, C, rows in chain)
        ent = self._buf_cache.get(key)
        if ent is None or ent[0] != sig:          # (raw addresses and row counts: rebuilt when any of them changes)
            ent = (sig, ops.make_bn_chain_desc([(accs[n], self.buffers[n + ".running_mean"], self.buffers[n + ".running_var"], C, rows)
                                                for n, C, rows in chain], self.device))
            self._buf_cache[key] = ent
        self.chain_rows = {n: rows for n, _, rows in chain}      # (tests: the statistics rows of every BatchNorm of the latest forward)
        ops.bn_running_chain(ent[1][0], ent[1][1], G, MOMENTUM)

    def forward_features(self, img, img_index=None, droppath=None, save=False, update_stats=True, tag=None, B=None, passes=1, first_img=None,
                         all_groups=False, keep_first=False):
        """img fp32 [B,3,H,W] (NCHW as the loaders deliver it).  Returns (logits [B,C], feat [B,F], ctx or None).
        ``update_stats=False`` = forward under Bn_Controller.freeze_bn.  ``tag`` names the activation buffer set (two saved graphs of
        a step must not share buffers).
        Launches: stem (layout + im2col + GEMM + statistics), then ONE per convolution -- each reads its input through the BatchNorm +
        LeakyReLU in front of it and leaves the statistics of the BatchNorm behind it --, then the final BatchNorm, pooling, classifier.
        ``passes`` = G > 1: G forwards of the SAME batch under frozen running statistics share every launch behind the stem (pass-major
        activations [G * rows, C]; each pass is its own BatchNorm statistics group, as G separate model() calls are in the reference:
        srpseudolabel.py:59-90 forwards x_ulb_w K + 1 times per step).  Returns logits [G * B, C], feat [G * B, F] in pass order;
        ``save`` keeps the LAST pass for a backward.  ``first_img`` (same shape as img): pass 0 forwards THAT batch instead -- the labelled
        batch of the step, the one model() call that moves the running statistics (``update_stats`` then applies to pass 0 alone, which is
        what the kernels implement) -- and ``save`` keeps it as well: ctx = (ctx of pass 0, ctx of the last pass).
        ``all_groups`` (with update_stats, no first_img): EVERY pass moves the running statistics, in pass order, and num_batches_tracked
        advances by G -- G model() calls in training mode with no Bn_Controller (srfixmatch / srflexmatch / srfreematch / srsoftmatch).  The
        convolution launches then leave the running statistics alone and one launch behind the forward walks the groups (_running_chain).
        ``keep_first`` (save, G > 1): pass 0 is kept for a backward too, ctx = (ctx of pass 0, ctx of the last pass) as for first_img."""
        assert img_index is None and droppath is None, "WideResNet has no DropPath and takes whole batches (BatchNorm couples the rows)"
        B, _, H, W = img.shape
        G = int(passes)
        tag = tag or ("s" if save else "i")
        train = self.training
        upd = bool(train and update_stats)
        assert train or not save, "the backward needs a training-mode forward (batch statistics)"
        allg = bool(all_groups)
        assert not allg or (upd and first_img is None), "all_groups: a training-mode forward that moves the running statistics, without first_img"
        assert G == 1 or (train and (not upd or first_img is not None or allg)), \
            "passes > 1: batch statistics per pass; a first_img pass or all_groups may move the running statistics (else Bn_Controller.freeze_bn)"
        assert first_img is None or (G > 1 and tuple(first_img.shape) == tuple(img.shape))
        keep_first = bool(keep_first and save and G > 1 and first_img is None)
        two = first_img is not None or keep_first
        chain = [] if allg else None
        kupd = upd and not allg                               # what the convolution / head launches do to the running statistics themselves
        f32 = torch.float32
        last = (lambda t, rows: t) if G == 1 else (lambda t, rows: t[(G - 1) * rows:])      # the pass a save=True forward keeps
        a0 = self._buf((tag, "in"), (B, H, W, 3), torch.bfloat16)
        out = self._buf((tag, "stem.out"), (G * B * H * W, self.channels[0]), f32)
        col0 = colf = None
        for g_ in range(G):                                   # the stem convolution of every pass (layout + im2col + GEMM: three small launches)
            src, stag = (first_img, tag + ":first") if (g_ == 0 and first_img is not None) else (img, tag)      # (pass 0's col is a backward operand of its own)
            ops.nchw_to_nhwc_bf16(src.contiguous(), a0, B, 3, H, W)
            col0, _, _ = self._conv("conv1.weight", a0, B, H, W, 1, out[g_ * B * H * W:(g_ + 1) * B * H * W], stag, bias=self.p("conv1.bias"))
            if g_ == 0:
                colf = col0
        ctx = ctx_f = None
        if save:
            ctx = WrnContext()
            ctx.B, ctx.H, ctx.W, ctx.tag, ctx.stem, ctx.blocks = B, H, W, tag, dict(col=col0), []
            if two:
                ctx_f = WrnContext()
                ctx_f.B, ctx_f.H, ctx_f.W, ctx_f.tag, ctx_f.stem, ctx_f.blocks = B, H, W, tag + ":first", dict(col=colf), []
        h, w = H, W
        accs = None
        if train:
            # the accumulators of every BatchNorm of this forward: one fill launch
            if G == 1:
                self.bn_acc_arena.zero_()
                accs = self.bn_acc
            else:
                arena, accs, pcell, pfirst = self._pass_acc(G)
                arena.zero_()
            # sums of the stem's output for the first block's bn1 (every later BatchNorm gets them from the convolution in front of it)
            first = self.blocks[0][0] + "bn1"
            for g_ in range(G):
                ops.bn_accumulate(out[g_ * B * h * w:(g_ + 1) * B * h * w], accs[first] if G == 1 else accs[first][g_], B * h * w, self.channels[0])
            if self.stat_sync:
                # (+ the row counts of the ranks, compared on the device -- on the shared-launch path as well: SRPseudoLabel's default)
                if G == 1:
                    self._sync_first_acc(B)
                else:
                    self._sync_first_acc(B, pcell, pfirst)
        for bi, (p, cin, cout, stride, abr) in enumerate(self.blocks):
            equal = cin == cout
            raw = not (equal or abr)                          # wrn.py:50: conv1 / convShortcut take the RAW x; bn1's statistics still move
            ho, wo = (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1
            rows_out = B * ho * wo
            c1 = self._buf((tag, p, "c1"), (G * rows_out, cout), f32)
            kw = dict(passes=G, accs=accs, chain=chain)
            # conv1 reads x through bn1 (folding / publishing its statistics) and leaves the sums of its output for bn2
            st1 = self._conv_bn(p + "conv1.weight", out, p + "bn1", raw, B, h, w, stride, c1, tag, train, kupd, next_bn=p + "bn2", publish=True, **kw)
            if equal:
                sc = out
            else:
                sc = self._buf((tag, p, "sc"), (G * rows_out, cout), f32)
                self._conv_bn(p + "convShortcut.weight", out, p + "bn1", raw, B, h, w, stride, sc, tag, train, kupd, **kw)
            y = self._buf((tag, p, "y"), (G * rows_out, cout), f32)
            nxt = self.blocks[bi + 1][0] + "bn1" if bi + 1 < len(self.blocks) else "bn1"        # (the last block feeds the final BatchNorm)
            st2 = self._conv_bn(p + "conv2.weight", c1, p + "bn2", False, B, ho, wo, 1, y, tag, train, kupd, resid=sc, next_bn=nxt, publish=True, **kw)
            if save:
                pick = (lambda st: st) if G == 1 else (lambda st: (st[0][G - 1], st[1][G - 1]))
                ctx.blocks.append(dict(x=last(out, B * h * w), st1=pick(st1), c1=last(c1, rows_out), st2=pick(st2), raw=raw, h=h, w=w, ho=ho, wo=wo))
                if ctx_f is not None:
                    ctx_f.blocks.append(dict(x=out[:B * h * w], st1=(st1[0][0], st1[1][0]), c1=c1[:rows_out], st2=(st2[0][0], st2[1][0]), raw=raw,
                                             h=h, w=w, ho=ho, wo=wo))
            out, h, w = y, ho, wo
        rows = B * h * w
        C3 = self.channels[3]
        # final BatchNorm + LeakyReLU + average pooling + classifier: one launch (it folds the sums the last convolution left and publishes)
        feat = torch.empty(G * B, C3, dtype=f32, device=self.device)
        logits = torch.empty(G * B, self.num_classes, dtype=f32, device=self.device)
        run = (self.buffers["bn1.running_mean"], self.buffers["bn1.running_var"])
        if train:
            stf = self._stats_bufs("bn1", C3, tag, G)
            ops.wrn_head(out, 3, None, accs["bn1"], self.p("bn1.weight"), self.p("bn1.bias"), self.eps["bn1"], SLOPE,
                         self.p("classifier.weight"), self.p("classifier.bias"), feat, logits, B, h * w, C3, self.num_classes, publish=stf,
                         running=run, momentum=MOMENTUM, update_running=kupd, stat_ranks=self.stat_ranks, passes=G)
            stf_first = (stf[0][0], stf[1][0]) if G > 1 else None
            if G > 1:
                stf = (stf[0][G - 1], stf[1][G - 1])
            if allg:
                chain.append(("bn1", C3, rows * self.stat_ranks))
                self._running_chain(chain, accs, G, tag)
                self._nbt += G                                  # (every pass is a model() call of its own)
            elif upd:
                self._nbt += 1                                  # num_batches_tracked of all BatchNorms (each was visited once)
        else:
            stf = None
            ops.wrn_head(out, 1, run, None, self.p("bn1.weight"), self.p("bn1.bias"), self.eps["bn1"], SLOPE, self.p("classifier.weight"),
                         self.p("classifier.bias"), feat, logits, B, h * w, C3, self.num_classes)
        if save:
            ctx.final, ctx.feat = dict(x=last(out, rows), st=stf, h=h, w=w), feat[(G - 1) * B:]
            if ctx_f is not None:
                ctx_f.final, ctx_f.feat = dict(x=out[:rows], st=stf_first, h=h, w=w), feat[:B]
                return logits, feat, (ctx_f, ctx)
        return logits, feat, ctx

    # ---- the two kinds of pass of an SRPseudoLabel step (srpseudolabel.py:59-90) ---------------------------------------------------------------
    def forward_frozen(self, img, tag="ulb_inf"):
        """A data_generator pass: forward_features(img, save=False, update_stats=False) -> (logits, feat)."""
        lg, ft, _ = self.forward_features(img, save=False, update_stats=False, tag=tag)
        return lg, ft

    def forward_saved(self, img, update_stats, tag):
        """forward_features(img, save=True, ...) -> (logits, feat, ctx) for a later backward(ctx, .)."""
        return self.forward_features(img, save=True, update_stats=update_stats, tag=tag)

    def forward_passes(self, img, passes, tag="ulb", first_img=None):
        """The K + 1 forwards of one batch under frozen running statistics (data_generator's K passes + the pass the unsupervised loss
        back-propagates through, srpseudolabel.py:59-90, :104-110) with shared launches: (logits [passes * B, C], feat, ctx of the LAST pass).
        ``first_img``: the labelled batch's forward (the call that moves the running statistics, :96) rides in the same launches as pass 0 of
        passes + 1: (logits [(passes + 1) * B, C], feat, (ctx of the labelled pass, ctx of the last pass))."""
        if first_img is not None:
            return self.forward_features(img, save=True, update_stats=True, tag=tag, passes=passes + 1, first_img=first_img)
        return self.forward_features(img, save=True, update_stats=False, tag=tag, passes=passes)

    MAX_SHARED_PASSES = 64        # (srhip_wrn_conv_bn_passes refuses more statistics groups per launch)

    def forward_cat_passes(self, img, passes, tag="cat"):
        """``passes`` model() calls on the SAME batch in training mode with no Bn_Controller (the K + 1 calls on cat(x_lb, x_ulb_w, x_ulb_s) of
        an SRFixMatch / SRFlexMatch / SRFreeMatch / SRSoftMatch step, fixmatch.py:62-146): every pass is one BatchNorm statistics group over
        the whole batch and every pass moves the running statistics and num_batches_tracked, in pass order.  Shared launches; more than
        MAX_SHARED_PASSES run as chunks in pass order (the running chain continues across them).  Returns (logits [passes * B, C], feat
        [passes * B, F], ctxs): ctxs = (ctx of pass 0, ctx of the last pass), or (ctx,) for one pass."""
        G, M = int(passes), self.MAX_SHARED_PASSES
        assert G >= 1
        if G <= M:
            lg, ft, ctx = self.forward_features(img, save=True, update_stats=True, tag=tag, passes=G, all_groups=True, keep_first=True)
            return lg, ft, (ctx if G > 1 else (ctx,))
        # Chunks in pass order: the first keeps pass 0, the last keeps the last pass, the ones between keep nothing -- so all of THOSE may
        # forward through ONE buffer set (':mid'; their logits / features are fresh tensors per call).  The first chunk is forwarded with
        # keep_first, which also fills a ctx for that chunk's own last pass: views of buffers that exist anyway, dropped here.
        sizes = [M] * (G // M) + ([G % M] if G % M else [])
        lgs, fts, ctx0, ctxl = [], [], None, None
        for i, n in enumerate(sizes):
            first, lastc = i == 0, i == len(sizes) - 1
            lg, ft, ctx = self.forward_features(img, save=first or lastc, update_stats=True, passes=n, all_groups=True, keep_first=first,
                                                tag=tag + (":head" if first else "" if lastc else ":mid"))
            if first:
                ctx0 = ctx[0]
            if lastc:
                ctxl = ctx[-1] if isinstance(ctx, tuple) else ctx
            lgs.append(lg)
            fts.append(ft)
        return torch.cat(lgs), torch.cat(fts), (ctx0, ctxl)

    def forward(self, x, only_fc=False, only_feat=False, **kw):
        assert not only_fc
        logits, feat, _ = self.forward_features(x.contiguous(), save=False)
        return feat if only_feat else {"logits": logits, "feat": feat}

    __call__ = forward

    # ---- backward ---------------------------------------------------------------------------------------------------------------
    def backward(self, ctx, dlogits):
        """Accumulates d(loss)/d(params) into ``self.grad`` given dlogits fp32 [B, C] for a save=True forward."""
        B, tag = ctx.B, ctx.tag
        f32, bf16 = torch.float32, torch.bfloat16
        P, G = self.p, (lambda n: self.p(n, self.grad))
        C3, K = self.channels[3], self.num_classes
        problems, unpad = [], []
        dy_bf16 = {}        # fp32 gradient tensor (by address) -> its bf16 copy, the operand of the filter- and input-gradient GEMMs
        # padded filter gradients of all convolutions: slices of ONE arena per buffer set, zeroed by one launch
        dwk = ("dwpad", tag)
        if dwk not in self._buf_cache:
            need = [(n, c) for n, c in self.convs.items() if not (c["Kp"] == c["K"] and c["k"] == 1)]
            arena = torch.zeros(sum(c["cout"] * c["Kp"] for _, c in need), dtype=f32, device=self.device)
            views, o = {}, 0
            for n, c in need:
                views[n] = arena[o:o + c["cout"] * c["Kp"]].view(c["cout"], c["Kp"])
                o += c["cout"] * c["Kp"]
            self._buf_cache[dwk] = (arena, views)
        dw_arena, dwpad = self._buf_cache[dwk]
        dw_arena.zero_()

        def conv_bwd(name, dy, rows_out, col, need_dx, Hin, Win, stride, din=None, accumulate=False):
            """dy fp32 [rows_out, Cout] -> dW problem (deferred) and, if need_dx, d(conv input) fp32 [B*Hin*Win, Cin] (into din)."""
            c = self.convs[name]
            dyb = dy_bf16.get(dy.data_ptr())                  # written by the BatchNorm backward that produced dy
            if dyb is None:
                dyb = self._buf((tag, name, "dyb"), (rows_out, c["cout"]), bf16)
                ops.cast_f32_bf16(dy, dyb, rows_out * c["cout"])
                dy_bf16[dy.data_ptr()] = dyb
            if c["Kp"] == c["K"] and c["k"] == 1:          # (a 1x1 filter: the tap-major K axis IS the parameter's layout)
                dst = self.view(name, self.grad).view(c["cout"], c["K"])
            else:
                dst = dwpad[name]                               # (a slice of one arena, zeroed with one launch above)
                unpad.append((dst, name))
            problems.append((dyb, col, dst, G("conv1.bias") if name == "conv1.weight" else None, c["cout"], c["Kp"], rows_out))
            if not need_dx:
                return None
            if "Wfl" in c and stride == 1 and not accumulate and _FUSED_DX:
                # dX = conv(dY, W'): the adjoint of a stride-1 3x3 convolution is one implicit-GEMM launch (raw fp32 dY in, bf16 on load)
                if din is None:
                    din = self._buf((tag, name, "din"), (B * Hin * Win, c["cin"]), f32)
                ops.wrn_conv_bn(dy, 2, None, None, None, None, 0.0, SLOPE, c["Wfl"], None, din, B, Hin, Win, c["cout"], c["cin"], 3, 1, c["Kp2"])
                return din
            dcol = self._buf((tag, name, "dcol"), (rows_out, c["Kp"]), f32)
            ops.gemm_nt(ops.EPI_F32, dyb, c["WbT"], dcol, rows_out, c["Kp"], c["cout"])
            if din is None:
                din = self._buf((tag, name, "din"), (B * Hin * Win, c["cin"]), f32)
            ops.col2im(dcol, din, B, Hin, Win, c["cin"], c["k"], stride, c["Kp"], accumulate=accumulate)
            return din

        # classifier, pooling, final BatchNorm
        fin = ctx.final
        rows = B * fin["h"] * fin["w"]
        dfeat = self._buf((tag, "dfeat"), (B, C3), f32)
        ops.fc_bwd(dlogits.contiguous(), ctx.feat, P("classifier.weight"), dfeat, G("classifier.weight"), G("classifier.bias"), B, C3, K)
        dact = self._buf((tag, "dactf"), (rows, C3), f32)
        ops.avgpool_bwd(dfeat, dact, B, fin["h"] * fin["w"], C3)
        dy = self._buf((tag, "dy.final"), (rows, C3), f32)
        ranks, sync = self.stat_ranks, self.stat_sync

        def bn_bwd(dact, x, st, bn, resid, dx, rows_, C_):
            """BatchNorm + LeakyReLU backward: the two column sums (this rank's, then every rank's under SyncBatchNorm), then the apply pass."""
            ops.bn_bwd_reduce(dact, x, st[0], st[1], P(bn + ".weight"), P(bn + ".bias"), SLOPE, self.ws, rows_, C_)
            local = None
            if sync:
                import torch.distributed as dist
                local = self._buf((tag, "bn.local_sums"), (512,), torch.float64)
                local[:2 * C_].copy_(self.ws[:2 * C_])
                dist.all_reduce(self.ws[:2 * C_])
            dxb = self._buf((tag, bn, "dx.bf16"), (rows_, C_), bf16)         # (saves the cast launch of the convolution backward that reads dx)
            ops.bn_bwd_apply(dact, x, st[0], st[1], P(bn + ".weight"), P(bn + ".bias"), SLOPE, resid, dx, G(bn + ".weight"), G(bn + ".bias"),
                             self.ws, local, rows_ * ranks, rows_, C_, dx_bf16=dxb)
            dy_bf16[dx.data_ptr()] = dxb

        bn_bwd(dact, fin["x"], fin["st"], "bn1", None, dy, rows, C3)

        def col_of(name, src, bn, st, raw, rows_src, Hs, Ws, stride):
            """The im2col operand of a convolution's filter gradient, recomputed from what the forward kept (its fp32 input and the statistics of
            the BatchNorm in front of it) instead of stored by every forward: one launch, BatchNorm + LeakyReLU applied on load."""
            c = self.convs[name]
            k, pad = c["k"], c["k"] // 2
            Ho, Wo = (Hs + 2 * pad - k) // stride + 1, (Ws + 2 * pad - k) // stride + 1
            col = self._buf((tag, name, "col"), (B * Ho * Wo, c["Kp"]), bf16)
            if raw:
                ops.im2col_bn(src, None, None, None, SLOPE, 2, col, B, Hs, Ws, c["cin"], k, stride, c["Kp"])
            else:
                ops.im2col_bn(src, st, P(bn + ".weight"), P(bn + ".bias"), SLOPE, 0, col, B, Hs, Ws, c["cin"], k, stride, c["Kp"])
            return col

        for (p, cin, cout, stride, abr), r in zip(reversed(self.blocks), reversed(ctx.blocks)):
            equal = cin == cout
            rows_out, rows_in = B * r["ho"] * r["wo"], B * r["h"] * r["w"]
            col2 = col_of(p + "conv2.weight", r["c1"], p + "bn2", r["st2"], False, rows_out, r["ho"], r["wo"], 1)
            col1 = col_of(p + "conv1.weight", r["x"], p + "bn1", r["st1"], r["raw"], rows_in, r["h"], r["w"], stride)
            r = dict(r, col2=col2, col1=col1)
            if not equal:
                r["colS"] = col_of(p + "convShortcut.weight", r["x"], p + "bn1", r["st1"], r["raw"], rows_in, r["h"], r["w"], stride)
            do2 = conv_bwd(p + "conv2.weight", dy, rows_out, r["col2"], True, r["ho"], r["wo"], 1)
            dc1 = self._buf((tag, p, "dc1"), (rows_out, cout), f32)
            bn_bwd(do2, r["c1"], r["st2"], p + "bn2", None, dc1, rows_out, cout)
            din = conv_bwd(p + "conv1.weight", dc1, rows_out, r["col1"], True, r["h"], r["w"], stride)
            dx = self._buf((tag, p, "dx"), (rows_in, cin), f32)
            if equal:
                bn_bwd(din, r["x"], r["st1"], p + "bn1", dy, dx, rows_in, cin)
            else:
                conv_bwd(p + "convShortcut.weight", dy, rows_out, r["colS"], True, r["h"], r["w"], stride, din=din, accumulate=True)
                if abr:
                    bn_bwd(din, r["x"], r["st1"], p + "bn1", None, dx, rows_in, cin)
                else:
                    dx = din                                   # raw-x path; this bn1 feeds nothing (no gradient, as in the reference)
            dy = dx
        conv_bwd("conv1.weight", dy, B * ctx.H * ctx.W, ctx.stem["col"], False, ctx.H, ctx.W, 1)
        # 32 x 288 .. 128 x 1152 outputs over 8192 .. 131072 pixels: slices of _DW_SPLIT pixels fill the chip (each writes a slab of its own; one reduce launch)
        # Descriptor tables hold raw addresses AND row counts: the key carries the operands' addresses, the batch size and every problem's shape
        # (a batch-size change under the same tag makes _buf reallocate; an address recycled by the caching allocator must not replay a table with
        # stale row counts), and ONE table per tag is kept -- the previous one is dropped when the key changes.
        sig = (B,) + tuple((int(pr[4]), int(pr[5]), int(pr[6])) for pr in problems) + tuple(int(t.data_ptr()) for pr in problems for t in pr[:3])
        ent_tn = self._buf_cache.get(("tn_desc", tag))
        if ent_tn is None or ent_tn[0] != sig:         # (one host-to-device copy per buffer set, not per backward: the operands are persistent)
            ent_tn = (sig, ops.make_group_tn_desc(problems, self.device, split_k=_DW_SPLIT, slabs=_DW_SLABS))
            self._buf_cache[("tn_desc", tag)] = ent_tn
        desc, npb, ntiles, flops, nbytes = ent_tn[1]
        ops.gemm_tn_grouped_f32(desc, npb, ntiles, alpha=1.0, beta=1.0, flops=flops, nbytes=nbytes)
        usig = tuple((int(src.data_ptr()), name) for src, name in unpad) + (int(self.grad.data_ptr()),)
        ent_up = self._buf_cache.get(("unpad_desc", tag))
        if ent_up is None or ent_up[0] != usig:        # dW[Cout, C, k, k] += dWpad[Cout, Kpad] (tap-major) for every padded gradient: one launch
            ent = [(src, self.p(name, self.grad), None, self.convs[name]["cout"], self.convs[name]["cin"], self.convs[name]["k"],
                    self.convs[name]["Kp"]) for src, name in unpad]
            ent_up = (usig, ops.make_conv_desc(ent, self.device, lambda Cout, C, kk, Kpad: Cout * C * kk))
            self._buf_cache[("unpad_desc", tag)] = ent_up
        ops.add_unpad_grouped(*ent_up[1])


def wrn_28_2(num_classes=100, pretrained=False, pretrained_path=None, **kw):
    m = WideResNet(num_classes=num_classes, depth=28, widen_factor=2, first_stride=1, **kw)           # wrn.py:160-164
    m.init_weights()
    if pretrained:
        load_checkpoint(m, pretrained_path)     # a file or the torch-hub cache entry of the URL; not found: random init + one warning line
    return m


def wrn_tiny_test(num_classes=10, **kw):
    m = WideResNet(num_classes=num_classes, depth=10, widen_factor=2, first_stride=1, **kw)
    m.init_weights()
    return m
