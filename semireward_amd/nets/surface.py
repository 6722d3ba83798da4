"""What the reference's DRIVER touches on ``model.model`` before training starts, for the engine backbones (flat parameter block + launches, no
nn.Module): train.py:396 ``count_parameters(model.model)`` (semilearn/core/utils/misc.py:73-75 iterates ``model.parameters()`` and reads
``requires_grad`` / ``numel()``) and train.py:399-400 ``send_model_cuda`` (misc.py:39-70: ``model.cuda(gpu)``,
``nn.SyncBatchNorm.convert_sync_batchnorm(model)`` which walks ``named_children()``, then the DistributedDataParallel wrap -- the one step an engine
model cannot take and ``semireward_amd.core.utils.send_model_cuda`` replaces; INTEGRATION.md names the two lines of train.py)."""
import torch

from .. import ops


class ModuleSurface:
    """Base of every engine backbone: the flat parameter block (fp32 parameters, their gradient twin and, for the GEMM backbones, a bf16
    operand copy), its accessors and mode switches, the workspace cache, the refresh of the derived operand copies, and the capabilities the
    algorithms read.  A backbone calls ``_init_block`` from its ``__init__`` and supplies ``transpose_items()`` when it keeps transposed copies."""
    frozen_params = ()          # names whose gradient is None in the reference (no path to the loss): requires_grad False here
    # Capabilities, read by the algorithms and the optimizer; a backbone sets the ones it has
    rows_independent = False    # no batch statistics: a row's outputs do not depend on which other rows share the launch
    scatter_outputs = False     # forward_features(out=...) writes logits / features at the caller's row numbers (no index_copy_)
    droppath_by_cols = False    # make_droppath(cols=...) lays the DropPath table out in the caller's column order (no index_select)
    precise_rows = False        # forward_features(precision="bf16x3"): split-bf16 products, fp32 activations (read_rows_precision)
    precise_grad_rows = False   # forward_features(save=True, precision="bf16x3") and its backward (grad_rows_precision)
    pass_prefix_sharing = False  # forward_features(tree=...): passes whose DropPath draws agree so far share rows (share_pass_prefixes)
    couples_batch_rows = False  # BatchNorm: every forward call is its own statistics group (no cross-pass batching)
    takes_tokens = False        # inputs are token batches (dicts of input_ids / attention_mask), not image tensors
    lazy_transposed = False     # after an optimizer step the transposed copies are only marked stale (ensure_transposed)

    def _init_block(self, names_shapes, align, bf16):
        """Lays out the flat block in ``names_shapes`` order: the next tensor starts at round_up(end of this one, align) and ``numel`` is the
        last end rounded the same way.  With ``bf16`` the block gets a bf16 operand copy, whose 2-D GEMM weights must start on a 16-byte
        boundary (8 elements).  The offsets also fix the optimizer's chunk tables and the data-parallel exchange ranges."""
        self.names_shapes = names_shapes
        self.offsets, o = {}, 0
        for n, s in names_shapes:
            self.offsets[n] = (o, s)
            o = (o + int(torch.Size(s).numel()) + align - 1) // align * align
        self.numel = o
        assert not bf16 or all(o_ % 8 == 0 for o_, s in self.offsets.values() if len(s) == 2)
        self.flat = torch.zeros(o, dtype=torch.float32, device=self.device)
        self.grad = torch.zeros(o, dtype=torch.float32, device=self.device)
        self.flat_bf16 = torch.zeros(o, dtype=torch.bfloat16, device=self.device) if bf16 else None
        self.buffers = {}           # non-parameter state_dict entries (BatchNorm running statistics), after the parameters
        self.training = True
        self._buf_cache, self._pviews = {}, {}
        self._wT_desc, self._wT_stale = None, False

    # ---- parameter plumbing ---------------------------------------------------------------------------------------------------------
    def p(self, name, buf=None):
        """Flat view of parameter ``name`` inside ``buf`` (default: the parameter block).  Cached per (name, buffer): building a slice view costs
        ~3 us of host time and a step asks for ~500 of them -- more than half of the step's enqueue time before the cache."""
        b = self.flat if buf is None else buf
        if not (b is self.flat or b is self.grad or b is self.flat_bf16):
            o, s = self.offsets[name]                     # some other block (optimizer state, a test's copy): no entry is kept for it
            return b[o:o + int(torch.Size(s).numel())]
        ent = self._pviews.get((name, id(b)))
        if ent is None:
            o, s = self.offsets[name]
            ent = self._pviews[(name, id(b))] = (b, b[o:o + int(torch.Size(s).numel())])     # (holds ``b``: its id stays unique)
        return ent[1]

    def view(self, name, buf=None):
        return self.p(name, buf).view(self.offsets[name][1])

    def named_parameters(self):
        return [(n, self.view(n)) for n, _ in self.names_shapes]

    def named_grads(self):
        return [(n, self.view(n, self.grad)) for n, _ in self.names_shapes]

    def state_dict(self):
        d = {n: self.view(n).detach().clone() for n, _ in self.names_shapes}
        d.update({k: v.detach().clone() for k, v in self.buffers.items()})
        return d

    def load_state_dict(self, sd, strict=True):
        for n, s in self.names_shapes:
            if n in sd:
                self.view(n).copy_(torch.as_tensor(sd[n]).to(self.device, torch.float32).reshape(s))
            elif strict:
                raise KeyError(n)
        for k in self.buffers:
            if k in sd:
                self.buffers[k].copy_(torch.as_tensor(sd[k]).to(self.device))
        self.refresh_operands()

    def no_weight_decay(self):
        return []

    def train(self, mode=True):
        self.training = mode
        return self

    def eval(self):
        return self.train(False)

    def zero_grad(self):
        self.grad.zero_()

    def _buf(self, key, shape, dtype, zero=False):
        """Workspace ``key``, reallocated when its shape or dtype changes (``zero``: a fresh one starts zeroed)."""
        t = self._buf_cache.get(key)
        if t is None or t.shape != torch.Size(shape) or t.dtype != dtype:
            t = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.device)
            self._buf_cache[key] = t
        return t

    # ---- derived operand copies -----------------------------------------------------------------------------------------------------
    def refresh_operands(self):
        """bf16 operand copy of the whole block + transposed GEMM weights (after any parameter change)."""
        ops.cast_f32_bf16(self.flat, self.flat_bf16, self.numel)
        self.refresh_transposed()

    def refresh_transposed(self):
        """W [out,in] fp32 -> W^T [in,out] bf16 for every ``transpose_items()`` entry: one batched launch."""
        self._wT_stale = False
        if self._wT_desc is None:
            self._wT_desc = ops.make_transpose_desc(self.transpose_items(), self.device)
        ops.transpose_batched(*self._wT_desc)

    def params_updated(self):
        """Called by the optimizer after its launch rewrote ``flat`` (and ``flat_bf16``): the transposed copies are refreshed now, or only
        marked stale on a ``lazy_transposed`` backbone."""
        if self.lazy_transposed:
            self._wT_stale = True
        else:
            self.refresh_transposed()

    def ensure_transposed(self):
        """The transposed bf16 weight copies are operands of the BACKWARD only (dX products).  On a ``lazy_transposed`` backbone they are
        refreshed after an optimizer step where it costs nothing -- the step's second stream, before the gradient rows' forward
        (srflexmatch._forward_plan) -- instead of at the end of the optimizer step, on the critical path (40 us per step); the backward calls
        this again as the safety net."""
        if self._wT_stale:
            self.refresh_transposed()

    def parameters(self, recurse=True):
        """Leaf views of the flat parameter block, one per reference parameter, in ``named_parameters()`` order: ``requires_grad`` as in the
        reference module, ``.grad`` = the matching view of the flat gradient block (so ``p.grad`` reads what the hand-written backward
        accumulated).  Fresh view objects per call -- the engine itself never touches them (its launches take raw pointers)."""
        for n, s in self.names_shapes:
            o = self.offsets[n][0]
            k = int(torch.Size(s).numel())
            p = self.flat[o:o + k].view(s)
            if n not in self.frozen_params:
                p.requires_grad_(True)
                p.grad = self.grad[o:o + k].view(s)
            yield p

    def _same_device(self, device):
        if device is None:
            return
        d = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if d.type != self.device.type or (d.index is not None and self.device.index is not None and d.index != self.device.index):
            raise RuntimeError("%s lives on %s (its blocks are allocated where it is built: pass device= to the builder); it cannot be moved to %s"
                               % (type(self).__name__, self.device, d))

    def cuda(self, device=None):
        """nn.Module.cuda(gpu) of misc.py:50/59/65: the engine model is built on its GPU already -- checked, not moved."""
        self._same_device(device if device is not None else "cuda")
        return self

    def to(self, *args, **kwargs):
        dev = kwargs.get("device", next((a for a in args if isinstance(a, (str, int, torch.device))), None))
        if any(isinstance(a, torch.dtype) for a in args) or kwargs.get("dtype") is not None:
            raise RuntimeError("the engine has one numeric mode (fp32 master block, bf16 operands): .to(dtype) is not supported")
        self._same_device(dev)
        return self

    # nn.SyncBatchNorm.convert_sync_batchnorm(model) (misc.py:55) walks named_children() and returns the module itself when there is no
    # nn.BatchNorm child: the engine's BatchNorm backbone exchanges its statistics itself under data parallel (nets/wrn.py ``dp``)
    def named_children(self):
        return iter(())

    def children(self):
        return iter(())

    def modules(self):
        return iter((self,))
