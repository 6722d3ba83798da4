"""What the reference's DRIVER touches on ``model.model`` before training starts, for the engine backbones (flat parameter block + launches, no
nn.Module): train.py:396 ``count_parameters(model.model)`` (semilearn/core/utils/misc.py:73-75 iterates ``model.parameters()`` and reads
``requires_grad`` / ``numel()``) and train.py:399-400 ``send_model_cuda`` (misc.py:39-70: ``model.cuda(gpu)``,
``nn.SyncBatchNorm.convert_sync_batchnorm(model)`` which walks ``named_children()``, then the DistributedDataParallel wrap -- the one step an engine
model cannot take and ``semireward_amd.core.utils.send_model_cuda`` replaces; INTEGRATION.md names the two lines of train.py)."""
import torch

from .. import ops


class RowArena:
    """One grow-only device allocation cut into blocks whose sizes follow two capacities: token rows (B * L) and sequences (B).  The token
    engines take their saved activations and output-gradient buffers from one: a call at (B, L) gets views of the first B * L rows of every
    block, so a run over batches of many padded lengths holds the memory of its largest batch, not one buffer set per length.

    ``spec``: [(name, count, unit, width, dtype)] -- ``count`` blocks called ``name``, each ``capacity[unit] * width`` elements (unit "row" or
    "seq").  Every block starts at a multiple of 256 bytes of an allocation that is itself that aligned, the alignment a fresh ``torch.empty``
    gives, so a launcher's 16-byte paths are the ones it takes on separate buffers; a block of 1 MiB or more starts at a multiple of 2 MiB, where
    the allocator puts a large tensor of its own (packed at 256 bytes the BERT-base bench step ran 0.5 % slower than on separate buffers, at
    2 MiB within 0.1 %: profiles/token_buckets.txt).  ``reserve`` only grows: when a call needs more rows or
    sequences the ``on_release`` hooks run (whoever keeps views or pointers into the arena drops them), the old allocation is released, and
    then one of the new maxima is made -- the two never coexist.  Contents never outlive a step, so nothing is copied.  Works on any
    device (the bookkeeping is tested with CPU tensors)."""
    ALIGN = 256
    BIG, BIG_ALIGN = 1 << 20, 2 << 20   # a block of 1 MiB or more starts at a multiple of 2 MiB, where the allocator puts a large tensor of its own

    def __init__(self, device, spec, on_alloc=None, alloc=None):
        self.device, self.spec = torch.device(device), [tuple(s) for s in spec]
        assert all(u in ("row", "seq") and c > 0 and w > 0 for _, c, u, w, _ in self.spec) and len({s[0] for s in self.spec}) == len(self.spec)
        self.rows = self.seqs = self.nbytes = 0
        self.store, self.offsets = None, {}
        self.allocations = 0            # how often the arena was (re)made
        self.on_release = []            # callables run before the allocation is released
        self._on_alloc = on_alloc
        self._alloc = alloc if alloc is not None else self._aligned_empty
        self._dtype = {n: dt for n, _, _, _, dt in self.spec}
        self._unit = {n: (u, w) for n, _, u, w, _ in self.spec}
        self._esize = {n: torch.empty(0, dtype=dt).element_size() for n, _, _, _, dt in self.spec}

    def _aligned_empty(self, n):
        al = self.BIG_ALIGN if n >= self.BIG else self.ALIGN
        raw = torch.empty(n + al, dtype=torch.uint8, device=self.device)    # (the device allocator's large blocks are aligned already: skip = 0)
        skip = -raw.data_ptr() % al
        return raw[skip:skip + n]

    def layout(self, rows, seqs):
        """({name: [byte offset of block 0, 1, ...]}, total bytes) at these capacities."""
        cap, off, o = dict(row=int(rows), seq=int(seqs)), {}, 0
        for name, count, unit, width, dt in self.spec:
            nb = cap[unit] * width * self._esize[name]
            al = self.BIG_ALIGN if nb >= self.BIG else self.ALIGN
            nb, o = (nb + al - 1) // al * al, (o + al - 1) // al * al
            off[name] = [o + i * nb for i in range(count)]
            o += count * nb
        return off, o

    def reserve(self, rows, seqs):
        """Makes room for ``rows`` token rows and ``seqs`` sequences.  True when the arena was replaced (every earlier view is void)."""
        if rows <= self.rows and seqs <= self.seqs and self.store is not None:
            return False
        rows, seqs = max(int(rows), self.rows), max(int(seqs), self.seqs)
        for hook in self.on_release:
            hook()
        self.store = None               # released BEFORE the larger one is made
        self.offsets, self.nbytes = self.layout(rows, seqs)
        store = self._alloc(max(self.nbytes, self.ALIGN))
        assert store.dtype == torch.uint8 and store.data_ptr() % self.ALIGN == 0
        self.store, self.rows, self.seqs = store, rows, seqs
        self.allocations += 1
        if self._on_alloc is not None:
            self._on_alloc(self)
        return True

    def view(self, name, i, shape):
        """The leading ``shape`` elements of block ``i`` of ``name`` (they must fit the block's capacity)."""
        unit, width = self._unit[name]
        dt = self._dtype[name]
        n = int(torch.Size(shape).numel())
        assert n <= (self.rows if unit == "row" else self.seqs) * width, (name, shape, self.rows, self.seqs)
        o = self.offsets[name][i]
        return self.store[o:o + n * self._esize[name]].view(dt).view(shape)

    def release(self):
        for hook in self.on_release:
            hook()
        self.store, self.offsets, self.rows, self.seqs, self.nbytes = None, {}, 0, 0, 0


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
        self._arenas = {}                # RowArena per key (token engines: saved context per tag, output-gradient buffers per context)
        self.arena_allocations = 0       # how often any of them was (re)made: constant once a run has met (or reserved) its largest batch
        self._reserved = (0, 0)          # token rows, sequences every arena and rows-capacity workspace starts from (reserve_tokens)
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

    def _buf_rows(self, key, shape, dtype, rows):
        """Rows-capacity variant of ``_buf`` for workspaces whose size follows the token rows of the call (``shape`` holds ``rows`` rows): the
        largest allocation seen under ``key`` is kept -- at least the reserved rows (reserve_tokens) -- and the leading ``shape`` elements are
        returned, so batches of many padded lengths share one buffer.  A fresh allocation is as aligned as ``_buf``'s."""
        n = int(torch.Size(shape).numel())
        ent = self._buf_cache.get(key)
        if ent is not None and ent[1] == shape and ent[0].dtype == dtype:
            return ent[2]
        if ent is None or ent[0].dtype != dtype or ent[0].numel() < n:
            self._buf_cache.pop(key, None)
            ent = None                                                       # (released before the larger one is made)
            flat = torch.empty(max(n, n // max(rows, 1) * self._reserved[0]), dtype=dtype, device=self.device)
        else:
            flat = ent[0]
        self._buf_cache[key] = (flat, shape, flat[:n].view(shape))
        return self._buf_cache[key][2]

    def _arena(self, key, spec, rows, seqs):
        """The RowArena ``key`` (made from ``spec`` when first asked for) with room for ``rows`` token rows and ``seqs`` sequences."""
        a = self._arenas.get(key)
        if a is None:
            a = self._arenas[key] = RowArena(self.device, spec, on_alloc=self._count_arena)
        a.reserve(max(rows, self._reserved[0]), max(seqs, self._reserved[1]))
        return a

    def _count_arena(self, arena):
        self.arena_allocations += 1

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
