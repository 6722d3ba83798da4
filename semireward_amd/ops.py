"""Torch-tensor front end of the C ABI (include/srhip.h).  Torch is plumbing only: it owns device
memory and the stream; every op below is a hand-written HIP kernel in libsrhip.so.  No fallbacks."""
import collections
import ctypes
import os

import torch

from . import _lib
from ._lib import EPI_BF16, EPI_DGELU_BF16, EPI_F32, EPI_GELU_BF16, EPI_RESID_F32  # noqa: F401
from ._lib import X3_EPI_F32, X3_EPI_GELU_F32, X3_EPI_RESID_F32  # noqa: F401
from ._lib import X3B_NT, X3B_NN, X3B_EPI_F32, X3B_EPI_ACC, X3B_EPI_DGELU, X3B_EPI_GELU_PRE  # noqa: F401
from ._lib import REDUCE_NONE, REDUCE_MEAN, REDUCE_SUM  # noqa: F401


# Argument checks cost 0.3 us per pointer x ~4500 pointers per training step = 1.3 ms of host time, which is what bounds the step once the GPU
# side drops below ~5 ms (bench.py --elide-unread-rows).  The engine only passes tensors it allocated itself; SRHIP_CHECK_ARGS=1 (set by
# tests/conftest.py, so every test run validates every call) turns the contiguity / device asserts back on.
_CHECK_ARGS = os.environ.get("SRHIP_CHECK_ARGS", "0") != "0"


def _p_checked(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "libsrhip needs contiguous device tensors"
    return t.data_ptr()


def _p_fast(t):
    return None if t is None else t.data_ptr()


_p = _p_checked if _CHECK_ARGS else _p_fast


class RawRows:
    """Element ``off`` (in elements from ``base.data_ptr()``; rows of a strided view are fine, the last dimension must be dense) .. of a device
    tensor as a bare pointer argument (a per-sample scale row of a [depth, 2, B] table, ...): what
    ``t[i, j]`` would hand to a launch without building a tensor view (~2 us of host time each, ~100 of them per step).  Holds the base tensor."""
    __slots__ = ("base", "ptr")
    is_cuda = True

    def __init__(self, base, off):
        if _CHECK_ARGS:
            assert base.is_cuda and base.stride(-1) == 1 and off >= 0
        self.base, self.ptr = base, base.data_ptr() + off * base.element_size()

    def data_ptr(self):
        return self.ptr

    def is_contiguous(self):
        return True


_STREAM = None


def _s():
    return _STREAM if _STREAM is not None else torch.cuda.current_stream().cuda_stream


# ---- streams that really run beside each other --------------------------------------------------------------------------------------
# HIP multiplexes its streams onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default); two streams that land on the SAME queue execute
# their launches one after the other, whatever the events between them say.  Which queue a new stream gets depends on how many streams the
# process has created before -- under data parallel the communicator's own streams shift the count, and the step's second stream then shared
# the queue of the step's stream: the two launch trains of a step serialised, 6.8 instead of 4.9 ms per step (profiles/r06_hw_queue_aliasing.txt).
# So the engine does not take "a new stream" on trust: it takes one that has been SEEN to overlap with the streams it must run beside.
_SPIN_CYCLES = None


def _spin_ms(cycles, streams):
    """Wall time (ms) of one spin kernel of ``cycles`` on each of ``streams``, all enqueued at once from a drained device."""
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in streams:
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def streams_overlap(a, b):
    """True when launches on the streams ``a`` and ``b`` execute concurrently (measured: two ~2 ms spin kernels take ~2, not ~4 ms)."""
    global _SPIN_CYCLES
    if _SPIN_CYCLES is None:
        c = 1 << 20
        _spin_ms(c, [a])                                    # (first launch: module load)
        one = min(_spin_ms(c, [a]) for _ in range(2))
        _SPIN_CYCLES = int(c * max(1.0, 2.0 / max(one, 1e-3)))     # ~2 ms
    one = min(_spin_ms(_SPIN_CYCLES, [a]) for _ in range(2))
    both = min(_spin_ms(_SPIN_CYCLES, [a, b]) for _ in range(2))
    return both < 1.5 * one


def concurrent_stream(device, beside=(), tries=16, priority=0):
    """A new stream that overlaps with the CURRENT stream and with every stream in ``beside`` (see above).  Falls back to the last candidate --
    with a warning on stderr -- when none of ``tries`` new streams does (a process pinned to one hardware queue: GPU_MAX_HW_QUEUES=1)."""
    import sys
    ref = [torch.cuda.current_stream(device)] + [s for s in beside if s is not None]
    cand, rejected = None, 0
    for _ in range(tries):
        cand = torch.cuda.Stream(device=device, priority=priority)
        if all(streams_overlap(r, cand) for r in ref):
            return cand
        rejected += 1
    print("semireward_amd: no stream that runs beside the step's stream among %d candidates (hardware queues exhausted? GPU_MAX_HW_QUEUES=%s): "
          "the step's launch trains will serialise" % (rejected, os.environ.get("GPU_MAX_HW_QUEUES", "default")), file=sys.stderr)
    return cand


class stream_scope:
    """Pin the hipStream_t for a burst of launches (torch.cuda.current_stream() costs ~2.5 us per call, 40 % of the host
    time of a training step).  Use as a context manager around code that does not switch streams."""

    def __enter__(self):
        global _STREAM
        self.prev = _STREAM
        _STREAM = torch.cuda.current_stream().cuda_stream
        return self

    def __exit__(self, *a):
        global _STREAM
        _STREAM = self.prev


_FN = {}


def _call(name, *args):
    fn = _FN.get(name)
    if fn is None:
        fn = _FN[name] = getattr(_lib.lib(), name)
    rc = fn(*args)
    if rc != 0:
        _lib.check(rc, name)


# ---- optional live profiling of the dominant kernel (bench.py roofline object) -------------------
class _GemmProfile:
    """Timing of every instrumented launch, keyed by the device kernel the C dispatcher picks.  Two clocks per launch:
      * the library's own dispatch-bound event pair (srhip_prof_*, csrc/prof.hip): the kernel's EXECUTION time, the quantity rocprofv3
        --kernel-trace reports -- this is what the roofline object uses;
      * a torch.cuda.Event pair recorded on the launch stream around the call: execution + dispatch latency + the event packets
        (reported beside it as ``avg_launch_us_event_pair``, never used for a roofline fraction)."""
    EPI = {0: "bf16", 1: "gelu_bf16", 2: "resid_f32", 3: "dgelu_bf16", 4: "f32"}

    def __init__(self):
        self.recs = []          # (event0, event1, flops, kernel name, algorithmic bytes, first launch index, last launch index)
        _lib.lib().srhip_prof_enable(1)

    def timed(self, name, args, flops, kernel, nbytes):
        """One instrumented C call (it may issue helper launches besides its main kernel: all of them are summed)."""
        i0 = _lib.lib().srhip_prof_count()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _call(name, *args)
        e1.record()
        if callable(kernel):                # the dispatcher's choice, asked after the launch
            kernel = kernel()
        self.recs.append((e0, e1, flops, kernel, nbytes, i0, _lib.lib().srhip_prof_count()))

    _KERNEL = {"tile128": "gemm_nt_kernel<%d>", "small64": "gemm_small_kernel<%d>", "big256": "gemm_big_kernel<%d, 8, 2>",
               "big128": "gemm_big_kernel<%d, 4, 2>", "big2wg": "gemm_big_kernel<%d, 8, 1>", "pp256": "gemm_pp_kernel<%d, 10>"}

    @classmethod
    def kernel_name(cls, epi, M, N, K):
        """The device kernel srhip_gemm_nt launches for this product: asked of the library itself (srhip_gemm_nt_plan, incl. the run-time
        small-tile threshold the step has set), not mirrored here."""
        return cls._KERNEL[gemm_nt_plan(epi, M, N, K, 1.0 if epi == EPI_F32 else 0.0)] % epi

    @staticmethod
    def gemm_bytes(epi, M, N, K, aux_in, aux_out, beta):
        """ALGORITHMIC HBM bytes of one product: bf16 operands once + the epilogue's reads/writes of C (and aux)."""
        b = 2.0 * (M * K + N * K)
        if epi == EPI_BF16:
            b += 2.0 * M * N
        elif epi == EPI_GELU_BF16:
            b += 2.0 * M * N * (2 if aux_out is not None else 1)
        elif epi == EPI_RESID_F32:
            b += 8.0 * M * N                                   # residual read + write, fp32
        elif epi == EPI_DGELU_BF16:
            b += 4.0 * M * N                                   # pre-activation read + bf16 write
        else:
            b += 4.0 * M * N * (2 if beta != 0.0 else 1)
        return b

    def per_kernel(self):
        import ctypes
        torch.cuda.synchronize()
        out = {}
        ms = ctypes.c_float()
        for a, b, f, name, nbytes, i0, i1 in self.recs:
            _call("srhip_prof_elapsed_ms", i0, i1, ctypes.cast(ctypes.byref(ms), ctypes.c_void_p))
            d = out.setdefault(name, [0.0, 0.0, 0, 0.0, 0.0])
            d[0] += f; d[1] += ms.value; d[2] += 1; d[3] += nbytes; d[4] += a.elapsed_time(b)
        return out           # name -> [flops, kernel-execution ms, launches, algorithmic bytes, event-pair ms]

    def totals(self):
        pk = self.per_kernel()
        return sum(v[0] for v in pk.values()), sum(v[1] for v in pk.values()), sum(v[2] for v in pk.values())


_PROFILE = None


def enable_gemm_profile():
    global _PROFILE
    _PROFILE = _GemmProfile()
    return _PROFILE


def disable_gemm_profile():
    global _PROFILE
    _PROFILE = None
    _lib.lib().srhip_prof_enable(0)


# ---- dense ------------------------------------------------------------------------------------
def gemm_nt(epi, A, B, C, M, N, K, *, lda=None, ldb=None, ldc=None, bias=None, row_scale=None, rows_per_sample=0,
            aux_in=None, aux_out=None, ldaux=0, alpha=1.0, beta=0.0, plan_M=None):
    """C[M,N] (+)= A[M,K] . B[N,K]^T  (bf16 operands; see srhip_gemm_nt).
    plan_M: take the tile kernel of a launch of plan_M >= M rows (srhip_gemm_nt_planned: the rows keep that launch's results bit for bit)."""
    if plan_M is not None:
        args = (epi, _p(A), lda or K, _p(B), ldb or K, _p(C), ldc or N, M, N, K, _p(bias), _p(row_scale), rows_per_sample, _p(aux_in),
                _p(aux_out), ldaux, alpha, beta, int(plan_M), _s())
        if _PROFILE is not None:           # (the kernel is the one of a plan_M-row launch)
            _PROFILE.timed("srhip_gemm_nt_planned", args, 2.0 * M * N * K, _GemmProfile.kernel_name(epi, int(plan_M), N, K),
                           _GemmProfile.gemm_bytes(epi, M, N, K, aux_in, aux_out, beta))
            return
        _call("srhip_gemm_nt_planned", *args)
        return
    if _PROFILE is not None:
        _PROFILE.timed("srhip_gemm_nt", (epi, _p(A), lda or K, _p(B), ldb or K, _p(C), ldc or N, M, N, K, _p(bias), _p(row_scale),
              rows_per_sample, _p(aux_in), _p(aux_out), ldaux, alpha, beta, _s(),), 2.0 * M * N * K, _GemmProfile.kernel_name(epi, M, N, K),
                              _GemmProfile.gemm_bytes(epi, M, N, K, aux_in, aux_out, beta))
        return
    _call("srhip_gemm_nt", epi, _p(A), lda or K, _p(B), ldb or K, _p(C), ldc or N, M, N, K, _p(bias), _p(row_scale),
          rows_per_sample, _p(aux_in), _p(aux_out), ldaux, alpha, beta, _s())


GEMM_PLAN_NAMES = {0: "tile128", 1: "small64", 2: "big256", 3: "big128", 4: "big2wg", 5: "pp256"}


def gemm_nt_plan(epi, M, N, K, beta=0.0):
    """Which tile kernel srhip_gemm_nt picks for this product (host logic, no launch; srhip_gemm_nt_plan)."""
    rc = int(_lib.lib().srhip_gemm_nt_plan(epi, M, N, K, beta))
    if rc < 0:
        _lib.check(rc, "srhip_gemm_nt_plan")
    return GEMM_PLAN_NAMES[rc]


GEMM_SMALL_ALONE, GEMM_SMALL_CONTENDED = 256, 40      # srhip_gemm_small_max_grid: chain alone on the chip / beside the deferred rows' launches
_small_max_grid = None


def gemm_small_max_grid(n):
    """Run-time threshold of the 64 x 64-tile kernel (srhip_gemm_small_max_grid); cached so that a step sets it with no call when unchanged."""
    global _small_max_grid
    if n != _small_max_grid:
        _lib.lib().srhip_gemm_small_max_grid(int(n))
        _small_max_grid = n


GROUP_DESC_DTYPE = [("A", "<u8"), ("B", "<u8"), ("C", "<u8"), ("M", "<i4"), ("N", "<i4"), ("K", "<i4"), ("lda", "<i4"),
                    ("ldb", "<i4"), ("ldc", "<i4"), ("tile_start", "<i4"), ("pad0", "<i4"), ("pad1", "<i4"), ("pad2", "<i4")]


def make_group_desc(problems, device):
    """problems: list of (A, B, C, M, N, K) with A bf16 [M,K], B bf16 [N,K], C fp32 [M,N] device tensors (dense rows).
    Returns (device uint8 tensor holding srhip_group_desc[], n_problems, total_tiles, total flops)."""
    import numpy as np
    arr = np.zeros(len(problems), dtype=GROUP_DESC_DTYPE)
    t = 0
    for i, (A, B, C, M, N, K) in enumerate(problems):
        arr[i] = (_p(A), _p(B), _p(C), M, N, K, K, K, N, t, 0, 0, 0)
        t += ((M + 127) // 128) * ((N + 127) // 128)
    assert arr.itemsize == 64
    flops = float(sum(2.0 * M * N * K for _, _, _, M, N, K in problems))
    nbytes = float(sum(2.0 * (M * K + N * K) + 8.0 * M * N for _, _, _, M, N, K in problems))
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device), len(problems), t, flops, nbytes


def gemm_nt_grouped_f32(desc, n_problems, total_tiles, alpha=1.0, beta=1.0, flops=0.0, nbytes=0.0, n64=False):
    """n64: the table counts 128 x 64 tiles (make_group_desc_ld(bn=64)) and goes to the narrow-column kernel."""
    fn, kern = ("srhip_gemm_nt_grouped_n64_f32", "gemm_grouped_n64_f32_kernel") if n64 else ("srhip_gemm_nt_grouped_f32", "gemm_grouped_f32_kernel")
    if _PROFILE is not None:
        _PROFILE.timed(fn, (_p(desc), n_problems, total_tiles, alpha, beta, _s(),), flops, kern, nbytes)
        return
    _call(fn, _p(desc), n_problems, total_tiles, alpha, beta, _s())


GROUP_TN_DESC_DTYPE = [("A", "<u8"), ("B", "<u8"), ("C", "<u8"), ("dbias", "<u8"), ("M", "<i4"), ("N", "<i4"), ("K", "<i4"),
                       ("lda", "<i4"), ("ldb", "<i4"), ("ldc", "<i4"), ("tile_start", "<i4"), ("flags", "<i4")]


TN_ATOMIC = 1


class TableStager:
    """Uploads small descriptor tables WITHOUT stalling the host: `tensor.to(device)` from pageable memory blocks until the copy has run, i.e. until
    everything queued in front of it on the stream has -- a whole training step for a table built inside one (the Wav2Vec2 encoder builds a
    weight-gradient table whenever LayerDrop leaves out a set of layers it has not seen before: 12 of the first 15 steps, 15 ms of host time
    each, the leg was host-bound).  A ring of pinned staging buffers and stream-ordered asynchronous copies instead; a slot is reused only after
    its copy has completed (an event per slot: by then it has, the wait is a formality)."""

    def __init__(self, nbytes, depth=8):
        self.bufs = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(depth)]
        self.events = [None] * depth
        self.i = 0

    def upload(self, arr_u8, device):
        n = int(arr_u8.size)
        slot = self.i % len(self.bufs)
        self.i += 1
        if n > self.bufs[slot].numel():
            return torch.from_numpy(arr_u8.copy()).to(device)                # (larger than the ring was sized for: the blocking path)
        if self.events[slot] is not None:
            self.events[slot].synchronize()
        self.bufs[slot][:n].copy_(torch.from_numpy(arr_u8))
        dev = torch.empty(n, dtype=torch.uint8, device=device)
        dev.copy_(self.bufs[slot][:n], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[slot] = ev
        return dev


SLAB_DESC_DTYPE = [("dst", "<u8"), ("src", "<u8"), ("stride", "<i8"), ("count", "<i4"), ("n_slabs", "<i4"), ("block_start", "<i4"), ("pad0", "<i4")]
TN_OVERWRITE = 2


def make_group_tn_desc(problems, device, split_k=0, tile=128, slabs=False, stager=None):
    """problems: list of (A, B, C, dbias, M, N, K) with A bf16 [K,M], B bf16 [K,N] (dense rows), C fp32 [M,N], dbias fp32 [M]
    or None.  Returns (device uint8 tensor holding srhip_group_tn_desc[], n_entries, total_tiles, flops, algorithmic bytes).
    split_k > 0: a problem with K >= 2 * split_k becomes ceil(K / split_k) entries over slices of its token axis, flagged
    SRHIP_TN_ATOMIC (they add into C; the launch must then be a C += product, beta = 1) -- or, with slabs=True, SRHIP_TN_OVERWRITE: every
    slice writes a scratch slab of its own and one srhip_slab_reduce_f32 launch (issued by gemm_tn_grouped_f32 behind the product) adds the
    slabs into C / dbias; the scratch and the reduce table ride on the returned tensor (.slab, .reduce).
    tile = 256: the table of srhip_gemm_tn_grouped_pp_f32 (256 x 256 tiles; gemm_tn_grouped_f32(..., pp=True)).  Its walk is static -- workgroup
    w of 256 takes tiles w, w + 256, ... -- so a short last round is balanced here: the last problems (enough of them to cover the tiles past
    the last full round) are handed over as token slices (SRHIP_TN_ATOMIC entries), which turns "a few workgroups run one tile more" into
    "most workgroups run a slice more" (beta must be 1 for such a table; `tn_pp_plan` says what was chosen).
    stager: a TableStager -- the table goes up through its asynchronous path (tables built inside a training step)."""
    import numpy as np
    assert all(pr[6] > 0 and pr[4] % 8 == 0 and pr[5] % 8 == 0 for pr in problems), "K >= 1 tokens; M, N multiples of 8 (srhip.h)"
    plan = [(tuple(pr), split_k if (split_k > 0 and pr[6] >= 2 * split_k) else 0) for pr in problems]
    if tile == 256 and split_k == 0:
        plan = tn_pp_plan(problems)
    slabs = slabs and any(sk > 0 for _, sk in plan)
    # scratch layout of the sliced problems: [slices][M][N] (+ [slices][M] for the bias sums), 16-byte aligned pieces
    lay, n_el = [], 0
    if slabs:
        for (A, B, C, db, M, N, K), sk in plan:
            if sk > 0:
                nsl = -(-K // sk)
                oc = n_el
                n_el += nsl * M * N
                ob = n_el
                n_el += nsl * M if db is not None else 0
                n_el = -(-n_el // 4) * 4
                lay.append((oc, ob, nsl))
            else:
                lay.append(None)
        slab = torch.empty(max(n_el, 4), dtype=torch.float32, device=device)
    ent, red = [], []
    t = rb = 0
    for i, ((A, B, C, db, M, N, K), sk) in enumerate(plan):
        tiles = ((M + tile - 1) // tile) * ((N + tile - 1) // tile)
        if sk > 0:
            for si, k0 in enumerate(range(0, K, sk)):
                if slabs:
                    oc, ob, nsl = lay[i]
                    cp = slab.data_ptr() + 4 * (oc + si * M * N)
                    bp = slab.data_ptr() + 4 * (ob + si * M) if db is not None else 0
                    ent.append((_p(A) + 2 * k0 * M, _p(B) + 2 * k0 * N, cp, bp, M, N, min(sk, K - k0), M, N, N, t, TN_OVERWRITE))
                else:
                    ent.append((_p(A) + 2 * k0 * M, _p(B) + 2 * k0 * N, _p(C), _p(db) or 0, M, N, min(sk, K - k0), M, N, N, t, TN_ATOMIC))
                t += tiles
            if slabs:
                oc, ob, nsl = lay[i]
                red.append((_p(C), slab.data_ptr() + 4 * oc, M * N, M * N, nsl, rb, 0))
                rb += -(-M * N // 1024)
                if db is not None:
                    red.append((_p(db), slab.data_ptr() + 4 * ob, M, M, nsl, rb, 0))
                    rb += -(-M // 1024)
        else:
            ent.append((_p(A), _p(B), _p(C), _p(db) or 0, M, N, K, M, N, N, t, 0))
            t += tiles
    arr = np.zeros(len(ent), dtype=GROUP_TN_DESC_DTYPE)
    for i, e in enumerate(ent):
        arr[i] = e
    assert arr.itemsize == 64
    flops = float(sum(2.0 * M * N * K for *_, M, N, K in problems))
    nbytes = float(sum(2.0 * (M * K + N * K) + 8.0 * M * N for *_, M, N, K in problems))
    up = (lambda a: stager.upload(a.view(np.uint8).reshape(-1), device)) if stager is not None else (lambda a: torch.from_numpy(a.view(np.uint8).copy()).to(device))
    desc = up(arr)
    # host copy of what the table writes, as (first byte, bytes): gemm_tn_grouped_tail_f32 checks its tail's outputs against it
    desc.out_ranges = [(e[2], 4 * e[4] * e[5]) for e in ent] + [(e[3], 4 * e[4]) for e in ent if e[3]]
    if slabs:
        ra = np.zeros(len(red), dtype=SLAB_DESC_DTYPE)
        for i, e in enumerate(red):
            ra[i] = e
        assert ra.itemsize == 40
        desc.slab = slab                                           # scratch + second-phase table live as long as the table
        desc.reduce = (up(ra), len(red), rb)
    return desc, len(ent), t, flops, nbytes


TN_PP_GRID = 256          # workgroups of srhip_gemm_tn_grouped_pp_f32 (one per CU)


def tn_pp_plan(problems, grid=TN_PP_GRID):
    """[(problem, token-slice length or 0)] for a 256-tile table: problems in order, the LAST ones sliced along the token axis when the tiles past
    the last full round of `grid` would otherwise leave most workgroups idle for one whole tile.  A slice is a multiple of 64 tokens (the
    kernel's K-tile) and at least 512; at most 8 slices per problem."""
    tiles = [((M + 255) // 256) * ((N + 255) // 256) for *_, M, N, K in problems]
    total = sum(tiles)
    rem = total % grid
    plan = [(tuple(pr), 0) for pr in problems]
    if total < grid or rem == 0 or rem > 0.7 * grid:
        return plan
    got = 0
    for i in range(len(problems) - 1, -1, -1):
        if got >= rem:
            break
        K = problems[i][6]
        want = max(2, min(8, grid // max(rem, 1)))
        n = min(want, K // 512)
        if n >= 2:
            sl = -(-K // n)
            sl = -(-sl // 64) * 64
            plan[i] = (tuple(problems[i]), sl)
        got += tiles[i]
    return plan


def tn_pp_efficiency(problems):
    """Share of the 256 x 256 tiles' area that is inside the problems (1.0 when every M and N is a multiple of 256)."""
    area = sum(M * N for *_, M, N, K in problems)
    cover = sum(((M + 255) // 256) * ((N + 255) // 256) * 65536 for *_, M, N, K in problems)
    return area / max(cover, 1)


def gemm_tn_grouped_f32(desc, n_problems, total_tiles, alpha=1.0, beta=1.0, flops=0.0, nbytes=0.0, pp=False):
    """C_p = alpha * A_p^T . B_p + beta * C_p (+ dbias_p += colsum A_p) for all problems in one launch.  pp: the table counts 256 x 256 tiles
    (make_group_tn_desc(tile=256)) and goes to the persistent two-group kernel."""
    fn, kern = ("srhip_gemm_tn_grouped_pp_f32", "gemm_tn_pp_kernel") if pp else ("srhip_gemm_tn_grouped_f32", "gemm_tn_grouped_f32_kernel")
    red = getattr(desc, "reduce", None)
    if red is not None:
        assert beta == 1.0, "a table with slab slices is a C += product"
    if _PROFILE is not None:
        _PROFILE.timed(fn, (_p(desc), n_problems, total_tiles, alpha, beta, _s(),), flops, kern, nbytes)
    else:
        _call(fn, _p(desc), n_problems, total_tiles, alpha, beta, _s())
    if red is not None:
        _call("srhip_slab_reduce_f32", _p(red[0]), red[1], red[2], _s())


def gemm_tn_grouped_tail_f32(desc, n_problems, total_tiles, D, ln=None, head=None, pe=None, alpha=1.0, beta=1.0):
    """gemm_tn_grouped_f32 with the ViT backward's small sums over all rows as extra workgroups of the same launch (srhip_dw_tail):
    ln = (desc, part, n_ln, n_rep): ln_grad_reduce;  head = (dlogits, feat, dWh, dbh, B, C): the weight half of cls_head_bwd;
    pe = (dx, img, img_index, dpos, dcls, ws, B, in_chans, HW, ps): the dpos / dcls launch and stage 1 of patch_embed_bwd_ws --
    patch_embed_bwd_ws(..., part_done=True) must follow.  Same bits as the separate launches."""
    from ._lib import DwTail
    assert getattr(desc, "reduce", None) is None, "a table with slab slices has a second phase of its own"
    t = DwTail()
    t.D = D
    if ln is not None:
        t.ln_desc, t.ln_part, t.n_ln, t.n_rep = _p(ln[0]), _p(ln[1]), ln[2], ln[3]
    if head is not None:
        t.dlogits, t.feat, t.dWh, t.dbh, t.B, t.C = _p(head[0]), _p(head[1]), _p(head[2]), _p(head[3]), head[4], head[5]
    if pe is not None:
        assert head is None or head[4] == pe[6]
        t.dx, t.img, t.img_index, t.dpos, t.dcls, t.pe_ws = (_p(x) for x in pe[:6])
        t.B, t.in_chans, t.HW, t.ps = pe[6:]
    if _CHECK_ARGS:     # the tail's workgroups run beside the tiles: nothing they write may be written by a tile (srhip.h)
        mine = list(getattr(ln[0], "out_ranges", ())) if ln is not None else []
        mine += [(_p(x), x.numel() * x.element_size()) for x in ((head[2], head[3]) if head is not None else ()) + (tuple(pe[3:6]) if pe is not None else ())]
        for a0, an in mine:
            for b0, bn in getattr(desc, "out_ranges", ()):
                assert a0 + an <= b0 or b0 + bn <= a0, "a tail output of gemm_tn_grouped_tail_f32 overlaps a C / dbias of the table"
    _call("srhip_gemm_tn_grouped_tail_f32", _p(desc), n_problems, total_tiles, alpha, beta, ctypes.addressof(t), _s())


def attn_block_supported(N, D, H):
    from ._lib import lib
    return bool(lib().srhip_attn_block_supported(N, D, H))


def attn_block_fused(xn, Wqkv, bqkv, out, B, N, D, H, scale, qkv_extra=None, out_scale=None):
    """out = attention(xn Wqkv^T + bqkv) for rows without a backward: qkv Linear + attention in one launch (xn = norm1 output, bf16).
    N = 257: the q | k | v row of the 257th token of every image comes from one small GEMM (qkv_extra [B, 3D] workspace, filled here).
    out_scale [B] fp32: per-image factor on the output rows, applied before their bf16 rounding (DropPath of the branch)."""
    if N == 257:
        # rows 256, 256 + N, ... of xn: a strided A operand (lda = N * D), no gather
        gemm_nt(EPI_BF16, xn[256:], Wqkv, qkv_extra, B, 3 * D, D, lda=N * D, bias=bqkv)
    if _PROFILE is not None:
        M = B * N
        # algorithmic work: the qkv product + QK^T + PV; bytes: xn bf16 in, bf16 out, the weights once
        _PROFILE.timed("srhip_attn_block_fused", (_p(xn), _p(Wqkv), _p(bqkv), _p(qkv_extra), _p(out), _p(out_scale), B, N, D, H, scale, _s(),), 2.0 * M * 3 * D * D + 4.0 * B * H * N * N * 64, "attn_block_kernel<%d>" % N,
                              2.0 * M * D + 2.0 * M * D + 2.0 * 3 * D * D)
        return
    _call("srhip_attn_block_fused", _p(xn), _p(Wqkv), _p(bqkv), _p(qkv_extra), _p(out), _p(out_scale), B, N, D, H, scale, _s())


AttnPlan = collections.namedtuple("AttnPlan", "nkt fwd_pair bwd_l2 bwd_split")


def attn_plan(B, N, H):
    """What an attention launch of this shape reaches (host logic, no launch; srhip_attn_plan): the key-tile instantiation, whether the
    forward is the paired kernel, whether the backward takes the L2 form, and the backward grid's blockIdx.y extent."""
    v = [ctypes.c_int(0) for _ in range(4)]
    rc = int(_lib.lib().srhip_attn_plan(B, N, H, *[ctypes.addressof(x) for x in v]))
    if rc != 0:
        _lib.check(rc, "srhip_attn_plan")
    return AttnPlan(v[0].value, bool(v[1].value), bool(v[2].value), v[3].value)


def attn_fwd(qkv, out, lse, B, N, H, scale):
    if _PROFILE is not None:        # flops: QK^T + PV; bytes: qkv in, out
        _PROFILE.timed("srhip_attn_fwd", (_p(qkv), _p(out), _p(lse), B, N, H, scale, _s()), 4.0 * B * H * N * N * 64, "attn_fwd_kernel",
                       2.0 * B * N * 4 * H * 64)
        return
    _call("srhip_attn_fwd", _p(qkv), _p(out), _p(lse), B, N, H, scale, _s())


def attn_bwd(qkv, out, d_out, lse, dqkv, delta_ws, B, N, H, scale):
    if _PROFILE is not None:        # flops: 5 N x N x 64 products per head (S, dP, dQ, dK, dV); bytes: qkv, out, d_out in, dqkv out
        _PROFILE.timed("srhip_attn_bwd", (_p(qkv), _p(out), _p(d_out), _p(lse), _p(dqkv), _p(delta_ws), B, N, H, scale, _s()),
                       10.0 * B * H * N * N * 64, "attn_bwd (dq + dkv kernels)", 2.0 * B * N * 8 * H * 64)
        return
    _call("srhip_attn_bwd", _p(qkv), _p(out), _p(d_out), _p(lse), _p(dqkv), _p(delta_ws), B, N, H, scale, _s())


def layernorm_fwd(x, gamma, beta, eps, out, mean, rstd, M, D):
    _call("srhip_layernorm_fwd", _p(x), _p(gamma), _p(beta), eps, _p(out), _p(mean), _p(rstd), M, D, _s())


def layernorm_bwd_cast(dy, x, mean, rstd, gamma, dx, dgamma, dbeta, out_bf16, row_scale, rows_per_sample, M, D):
    _call("srhip_layernorm_bwd_cast", _p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(dx), _p(dgamma), _p(dbeta), _p(out_bf16), _p(row_scale),
          rows_per_sample, M, D, _s())


def layernorm_bwd_part(dy, x, mean, rstd, gamma, dx, part, n_rep, out_bf16, row_scale, rows_per_sample, M, D):
    """layernorm_bwd(_cast) with dgamma / dbeta added into copy (workgroup % n_rep) of part fp32 [n_rep, 2, D]; see ln_grad_reduce."""
    if _PROFILE is not None:        # bytes: dy (bf16) + x (fp32) in, dx fp32 read + written, bf16 copy out
        _PROFILE.timed("srhip_layernorm_bwd_part", (_p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(dx), _p(part), n_rep, _p(out_bf16),
                                                    _p(row_scale), rows_per_sample, M, D, _s()), 0.0, "ln_bwd_kernel", 16.0 * M * D)
        return
    _call("srhip_layernorm_bwd_part", _p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(dx), _p(part), n_rep, _p(out_bf16), _p(row_scale),
          rows_per_sample, M, D, _s())


def make_ln_reduce_desc(pairs, device):
    """pairs: list of (dgamma, dbeta) fp32 views of the gradient block, in the order of the partial copies."""
    import numpy as np
    arr = np.array([[_p(g), _p(b)] for g, b in pairs], dtype=np.uint64)
    desc = torch.from_numpy(arr.view(np.uint8).copy()).to(device)
    desc.out_ranges = [(_p(t), t.numel() * t.element_size()) for pair in pairs for t in pair]
    return desc


def ln_grad_reduce(desc, part, n_ln, n_rep, D):
    _call("srhip_ln_grad_reduce", _p(desc), _p(part), n_ln, n_rep, D, _s())


def mlp_fused(x, gamma, beta, eps, W1, b1, W2, b2, row_scale, rows_per_sample, M, D, Hd, x_out=None, save=None):
    """x_out (default: x, in place; fp32 [M,D]) = x + row_scale * (fc2(gelu(fc1(LN(x)))) + b2), ONE launch.
    save = (rows, ln2, pre, h, mean, rstd): the first ``rows`` rows also get their backward operands written (see srhip.h)."""
    rows, ln2, pre, h, mean, rstd = save if save is not None else (0, None, None, None, None, None)
    args = (_p(x), _p(x_out if x_out is not None else x), _p(gamma), _p(beta), eps, _p(W1), _p(b1), _p(W2), _p(b2), _p(row_scale),
            rows_per_sample, rows, _p(ln2), _p(pre), _p(h), _p(mean), _p(rstd), M, D, Hd)
    if _PROFILE is not None:
        _PROFILE.timed("srhip_mlp_fused", (*args, _s(),), 4.0 * M * D * Hd, "mlp_fused_kernel<384, 0, 4>",
                              8.0 * M * D + 4.0 * D * Hd + rows * (2.0 * D + 4.0 * Hd))
        return
    _call("srhip_mlp_fused", *args, _s())


def mlp_fused_proj(x, ao, Wp, bp, row_scale1, gamma, beta, eps, W1, b1, W2, b2, row_scale2, rows_per_sample, M, D, Hd, x_out=None,
                   ln_next=None, next_gamma=None, next_beta=None, ao_scaled=False, row_pitch=None, plan_row=None):
    """x_out (default: x, in place) = x1 + row_scale2 * (fc2(gelu(fc1(LN(x1)))) + b2) with x1 = x + row_scale1 * (ao Wp^T + bp): the attention
    projection, both residuals and the MLP half of a block in ONE launch (rows without a backward).  ln_next (bf16 [M, D]): also
    LayerNorm(x_out) with the next block's norm1 affine.  ao_scaled: ao already carries row_scale1 (attn_block_fused out_scale).
    row_pitch (elements): the M rows lie that far apart in x, x_out and ao (srhip_mlp_fused_proj_strided); rows in between are untouched.
    plan_row (int32 [1 + M / rows_per_sample], one block's row of vit_droppath_plan): srhip_mlp_fused_proj_planned -- the samples whose MLP
    branch is dropped go to the tiles at the end of the launch, which stop after the projection."""
    assert row_pitch is None or plan_row is None
    args = (_p(x), _p(x_out if x_out is not None else x), _p(ao), _p(Wp), _p(bp), _p(row_scale1), int(bool(ao_scaled)), _p(gamma), _p(beta), eps,
            _p(W1), _p(b1),
            _p(W2), _p(b2), _p(row_scale2), rows_per_sample, _p(ln_next), _p(next_gamma), _p(next_beta), M, D, Hd)
    if _PROFILE is not None:
        # algorithmic: fc1 + fc2 + proj products; bytes: x in, x out (fp32; x1 never leaves the accumulators), ao in (bf16), [next norm1
        # output out (bf16)], the weights once
        nbytes = 8.0 * M * D + 2.0 * M * D + (2.0 * M * D if ln_next is not None else 0.0) + 4.0 * D * Hd + 2.0 * D * D
        if row_pitch is not None:       # a record of its own: the dense kernel's roofline line stays comparable with earlier ones
            _PROFILE.timed("srhip_mlp_fused_proj_strided", (*args, int(row_pitch), _s(),), 4.0 * M * D * Hd + 2.0 * M * D * D,
                           "mlp_fused_kernel<384, 0, 4, true, 1> class rows", nbytes)
            return
        if plan_row is not None:        # the same record as the dense launch it stands for, with that launch's nominal (reference) work
            _PROFILE.timed("srhip_mlp_fused_proj_planned", (*args, _p(plan_row), M // rows_per_sample, _s(),), 4.0 * M * D * Hd + 2.0 * M * D * D,
                           "mlp_fused_kernel<384, 0, 4, true, 1>", nbytes)
            return
        _PROFILE.timed("srhip_mlp_fused_proj", (*args, _s(),), 4.0 * M * D * Hd + 2.0 * M * D * D, "mlp_fused_kernel<384, 0, 4, true, 1>", nbytes)
        return
    if plan_row is not None:
        _call("srhip_mlp_fused_proj_planned", *args, _p(plan_row), M // rows_per_sample, _s())
        return
    if row_pitch is not None:
        _call("srhip_mlp_fused_proj_strided", *args, int(row_pitch), _s())
        return
    _call("srhip_mlp_fused_proj", *args, _s())


def gelu_eval(x, y_erf, y_poly):
    _call("srhip_gelu_eval", _p(x), _p(y_erf), _p(y_poly), x.numel(), _s())


def layernorm_bwd(dy, x, mean, rstd, gamma, dx, dgamma, dbeta, M, D):
    _call("srhip_layernorm_bwd", _p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(dx), _p(dgamma), _p(dbeta), M, D, _s())


def patch_embed_fwd(img, img_index, Wp, bp, cls, pos, x, B, C, HW, ps, D):
    _call("srhip_patch_embed_fwd", _p(img), _p(img_index), _p(Wp), _p(bp), _p(cls), _p(pos), _p(x), B, C, HW, ps, D, _s())


def patch_embed_bwd(dx, img, img_index, dWp, dbp, dcls, dpos, B, C, HW, ps, D):
    _call("srhip_patch_embed_bwd", _p(dx), _p(img), _p(img_index), _p(dWp), _p(dbp), _p(dcls), _p(dpos), B, C, HW, ps, D, _s())


def patch_embed_bwd_ws_floats(B, C, HW, ps, D):
    n = int(_lib.lib().srhip_patch_embed_bwd_ws_floats(B, C, HW, ps, D))
    if n < 0:
        raise ValueError("srhip_patch_embed_bwd_ws refuses B=%d C=%d HW=%d ps=%d D=%d" % (B, C, HW, ps, D))
    return n


def patch_embed_bwd_ws(dx, img, img_index, dWp, dbp, dcls, dpos, ws, B, C, HW, ps, D, part_done=False):
    """patch_embed_bwd through per-workgroup partial sums in ``ws`` (fp32, patch_embed_bwd_ws_floats elements): no atomics, fixed order.
    part_done: dpos / dcls and the partial sums already came from the tail of gemm_tn_grouped_tail_f32 on this stream -- only the fold runs."""
    if part_done:
        _call("srhip_patch_embed_bwd_fold", _p(ws), _p(dWp), _p(dbp), B, C, HW, ps, D, _s())
        return
    _call("srhip_patch_embed_bwd_ws", _p(dx), _p(img), _p(img_index), _p(dWp), _p(dbp), _p(dcls), _p(dpos), _p(ws), B, C, HW, ps, D, _s())


def patch_im2col(img, img_index, out, B, C, HW, ps):
    _call("srhip_patch_im2col", _p(img), _p(img_index), _p(out), B, C, HW, ps, _s())


def patch_assemble(tok, bp, cls, pos, x, B, Np, D):
    _call("srhip_patch_assemble", _p(tok), _p(bp), _p(cls), _p(pos), _p(x), B, Np, D, _s())


def patch_grad_operands(dx, dx_tok, dpos, dcls, B, Np, D):
    _call("srhip_patch_grad_operands", _p(dx), _p(dx_tok), _p(dpos), _p(dcls), B, Np, D, _s())


# ---- split-bf16 (bf16x3) forward of the rows that decide the masks (csrc/x3.hip) --------------------------------------------------------
def gemm_nt_x3(epi, A, W, C, M, N, K, *, lda=None, ldw=None, ldc=None, bias=None, row_scale=None, rows_per_sample=0):
    """C[M,N] = epilogue(A[M,K] . W[N,K]^T), fp32 operands as bf16 hi / lo planes, three MFMAs per fragment pair (see srhip_gemm_nt_x3)."""
    args = (epi, _p(A), lda or K, _p(W), ldw or K, _p(C), ldc or N, M, N, K, _p(bias), _p(row_scale), rows_per_sample, _s())
    if _PROFILE is not None:        # flops: the fp32-equivalent product (3x that on the MFMA); bytes: fp32 operands once + C (read too for RESID)
        _PROFILE.timed("srhip_gemm_nt_x3", args, 2.0 * M * N * K, "gemm_x3_kernel<nt, %s>" % ("f32", "gelu", "resid")[epi],
                       4.0 * (M * K + N * K) + 4.0 * M * N * (2 if epi == X3_EPI_RESID_F32 else 1))
        return
    _call("srhip_gemm_nt_x3", *args)


def attn_fwd_x3(qkv, out, B, N, H, scale):
    """out fp32 [B*N, H*64] = softmax(Q K^T * scale) V from qkv fp32 [B*N, 3*H*64], both products bf16x3 (srhip_attn_fwd_x3)."""
    if _PROFILE is not None:        # flops: QK^T (taken twice: max pass + exp pass) + PV as fp32-equivalent work; bytes: qkv in, out
        _PROFILE.timed("srhip_attn_fwd_x3", (_p(qkv), _p(out), B, N, H, scale, _s()), 4.0 * B * H * N * N * 64, "attn_fwd_x3_kernel<false>",
                       4.0 * B * N * 4 * H * 64)
        return
    _call("srhip_attn_fwd_x3", _p(qkv), _p(out), B, N, H, scale, _s())


def layernorm_fwd_f32(x, gamma, beta, eps, out, mean, rstd, M, D):
    _call("srhip_layernorm_fwd_f32", _p(x), _p(gamma), _p(beta), eps, _p(out), _p(mean), _p(rstd), M, D, _s())


def patch_im2col_f32(img, img_index, out, B, C, HW, ps):
    _call("srhip_patch_im2col_f32", _p(img), _p(img_index), _p(out), B, C, HW, ps, _s())


# ---- split-bf16 (bf16x3) gradient rows (csrc/x3.hip, the same tile engine) ------------------------------------------------------------
def attn_fwd_x3_lse(qkv, out, lse, B, N, H, scale):
    """attn_fwd_x3 that also writes lse fp32 [B, H, N] for attn_bwd_x3 (srhip_attn_fwd_x3_lse)."""
    args = (_p(qkv), _p(out), _p(lse), B, N, H, scale, _s())
    if _PROFILE is not None:
        _PROFILE.timed("srhip_attn_fwd_x3_lse", args, 4.0 * B * H * N * N * 64, "attn_fwd_x3_kernel<true>", 4.0 * B * N * 4 * H * 64)
        return
    _call("srhip_attn_fwd_x3_lse", *args)


def gemm_x3(layout, epi, A, B, C, M, N, K, *, lda=None, ldb=None, ldc=None, bias=None, aux=None, aux_out=None, ldaux=0):
    """X3B_NT: C[M,N] = gelu(A[M,K] . B[N,K]^T + bias), aux_out = the pre-activation (X3B_EPI_GELU_PRE).
    X3B_NN: C[M,N] = epi(A[M,K] . B[K,N]) with epi F32 (=), ACC (+=) or DGELU (* gelu'(aux)).  fp32 operands as bf16 hi / lo planes."""
    ldb = ldb or (K if layout == X3B_NT else N)
    args = (layout, epi, _p(A), lda or K, _p(B), ldb, _p(C), ldc or N, M, N, K, _p(bias), _p(aux), _p(aux_out), ldaux, _s())
    if _PROFILE is not None:        # flops: the fp32-equivalent product; bytes: fp32 operands once + C (+ aux / C read)
        extra = 1 if (epi == X3B_EPI_ACC or aux is not None or aux_out is not None) else 0
        _PROFILE.timed("srhip_gemm_x3", args, 2.0 * M * N * K, "gemm_x3_kernel<%s, %s>" % ("nt" if layout == X3B_NT else "nn", ("f32", "acc", "dgelu", "gelu_pre")[epi]),
                       4.0 * (M * K + N * K) + 4.0 * M * N * (1 + extra))
        return
    _call("srhip_gemm_x3", *args)


def gemm_tn_x3_grouped(desc, n_problems, total_tiles, flops=0.0, nbytes=0.0):
    """C_p += A_p^T . B_p, dbias_p += colsum A_p for every problem of a make_group_tn_desc table (fp32 A, B; 128-tiles, no split_k)."""
    args = (_p(desc), n_problems, total_tiles, _s())
    if _PROFILE is not None:
        _PROFILE.timed("srhip_gemm_tn_x3_grouped", args, flops, "gemm_tn_x3_grouped_kernel", nbytes)
        return
    _call("srhip_gemm_tn_x3_grouped", *args)


def make_group_tn_x3_desc(problems, device):
    """The srhip_group_tn_desc table of gemm_tn_x3_grouped: problems (A fp32 [K,M], B fp32 [K,N], C fp32 [M,N], dbias fp32 [M] or None, M, N,
    K); returns (desc, n, total_tiles, flops, fp32 algorithmic bytes)."""
    desc, n, tiles, flops, _ = make_group_tn_desc(problems, device)
    nbytes = float(sum(4.0 * (M * K + N * K) + 8.0 * M * N for *_, M, N, K in problems))
    return desc, n, tiles, flops, nbytes


def attn_bwd_x3(qkv, out, d_out, lse, dqkv, delta_ws, B, N, H, scale):
    """dqkv fp32 [B*N, 3*H*64] of softmax(Q K^T scale) V from the fp32 forward state and d_out fp32 (srhip_attn_bwd_x3)."""
    args = (_p(qkv), _p(out), _p(d_out), _p(lse), _p(dqkv), _p(delta_ws), B, N, H, scale, _s())
    if _PROFILE is not None:        # flops: S twice, dP twice, dQ, dK, dV; bytes: qkv, out, d_out in, dqkv out
        _PROFILE.timed("srhip_attn_bwd_x3", args, 14.0 * B * H * N * N * 64, "attn_bwd_x3_kernels", 4.0 * B * N * H * 64 * 8)
        return
    _call("srhip_attn_bwd_x3", *args)


def layernorm_bwd_part_f32(dy, x, mean, rstd, gamma, dx, part, n_rep, out, row_scale, rows_per_sample, M, D):
    """layernorm_bwd_part with fp32 dy; out (fp32 or None) = row_scale * the updated dx."""
    _call("srhip_layernorm_bwd_part_f32", _p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(dx), _p(part), n_rep, _p(out), _p(row_scale),
          rows_per_sample, M, D, _s())


def patch_grad_operands_f32(dx, dx_tok, dpos, dcls, B, Np, D):
    _call("srhip_patch_grad_operands_f32", _p(dx), _p(dx_tok), _p(dpos), _p(dcls), B, Np, D, _s())


def scale_rows_f32(x, scale, rows_per_sample, out, M, D):
    _call("srhip_scale_rows_f32", _p(x), _p(scale), rows_per_sample, _p(out), M, D, _s())


def cls_head_fwd_scatter(x, gamma, beta, eps, Wh, bh, feat, logits, xhat, rstd, feat_all, logits_all, out_rows, B, N, D, C):
    """cls_head_fwd that also (or only: feat / logits None) writes image b's outputs to row out_rows[b] of feat_all / logits_all."""
    _call("srhip_cls_head_fwd_scatter", _p(x), _p(gamma), _p(beta), eps, _p(Wh), _p(bh), _p(feat), _p(logits), _p(xhat), _p(rstd), _p(feat_all),
          _p(logits_all), _p(out_rows), B, N, D, C, _s())


def cls_head_fwd(x, gamma, beta, eps, Wh, bh, feat, logits, xhat, rstd, B, N, D, C):
    _call("srhip_cls_head_fwd", _p(x), _p(gamma), _p(beta), eps, _p(Wh), _p(bh), _p(feat), _p(logits), _p(xhat), _p(rstd),
          B, N, D, C, _s())


def cls_head_bwd(dlogits, Wh, gamma, feat, xhat, rstd, dx, dWh, dbh, dgamma, dbeta, B, N, D, C):
    _call("srhip_cls_head_bwd", _p(dlogits), _p(Wh), _p(gamma), _p(feat), _p(xhat), _p(rstd), _p(dx), _p(dWh), _p(dbh),
          _p(dgamma), _p(dbeta), B, N, D, C, _s())


def cast_scale_rows(x, scale, rows_per_sample, out, M, D):
    _call("srhip_cast_scale_rows", _p(x), _p(scale), rows_per_sample, _p(out), M, D, _s())


def transpose_to_bf16(inp, in_is_f32, ld_in, out, ld_out, M, Mp, C, apply_gelu=False, colsum=None):
    _call("srhip_transpose_to_bf16", _p(inp), int(in_is_f32), ld_in, _p(out), ld_out, M, Mp, C, int(apply_gelu), _p(colsum), _s())


TRANSPOSE_DESC_DTYPE = [("in", "<u8"), ("out", "<u8"), ("in_is_f32", "<i4"), ("ld_in", "<i4"), ("ld_out", "<i4"), ("M", "<i4"),
                        ("Mp", "<i4"), ("C", "<i4"), ("apply_gelu", "<i4"), ("tile_start", "<i4"), ("pad", "<i8")]


def make_transpose_desc(items, device):
    """items: list of (inp, in_is_f32, ld_in, out, ld_out, M, Mp, C, apply_gelu).  Returns (desc tensor, n, total_tiles)."""
    import numpy as np
    arr = np.zeros(len(items), dtype=TRANSPOSE_DESC_DTYPE)
    t = 0
    for i, (inp, f32, ld_in, out, ld_out, M, Mp, C, gelu) in enumerate(items):
        assert C % 64 == 0 and Mp % 2 == 0 and Mp >= M
        arr[i] = (_p(inp), _p(out), int(f32), ld_in, ld_out, M, Mp, C, int(gelu), t, 0)
        t += ((Mp + 63) // 64) * (C // 64)
    assert arr.itemsize == 56
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device), len(items), t


def transpose_batched(desc, n, total_tiles):
    _call("srhip_transpose_batched", _p(desc), n, total_tiles, _s())


def cast_f32_bf16(x, out, n):
    _call("srhip_cast_f32_bf16", _p(x), _p(out), n, _s())


def vit_droppath_plan(dp, depth, B, plan):
    """plan int32 [depth, 1 + B] of the DropPath table dp fp32 [depth, 2, B] (any strides over the first two dimensions, dense columns): per
    block the number of samples that keep the MLP branch, then those samples and the dropped ones, each in ascending order."""
    if _CHECK_ARGS:
        assert dp.is_cuda and dp.dim() == 3 and dp.stride(2) == 1 and dp.shape[0] >= depth and dp.shape[1] == 2 and dp.shape[2] >= B and plan.dtype == torch.int32 and plan.is_contiguous()
        assert plan.numel() == depth * (1 + B)
    _call("srhip_vit_droppath_plan", dp.data_ptr(), dp.stride(0), dp.stride(1), depth, B, _p(plan), _s())     # (a strided view: no _p)


def droppath_fill(out, probs, depth, B, seed, cols=None, seed_dev=None):
    """out [depth, 2, B] (cols None) or [depth, 2, len(cols)]: the columns cols of the same [depth, 2, B] draw, in that order.
    seed_dev (device address of a uint64): the seed is *seed_dev + seed (a step captured in a HIP graph, core/stepgraph.py)."""
    if seed_dev is not None:
        _call("srhip_droppath_fill_cols_dyn", _p(out), _p(probs), _p(cols), depth, B, cols.numel() if cols is not None else B, seed_dev, seed, _s())
    elif cols is None:
        _call("srhip_droppath_fill", _p(out), _p(probs), depth, B, seed, _s())
    else:
        _call("srhip_droppath_fill_cols", _p(out), _p(probs), _p(cols), depth, B, cols.numel(), seed, _s())


def vit_fork(x, ln, parent, n_new, dst0, rows_per_node, D):
    """Nodes dst0 .. dst0 + n_new - 1 of a pass-prefix tree level become copies of their parents (int32 device indices, each < dst0): the
    fp32 residual x [*, rows_per_node, D] and, if given, the bf16 norm1 output ln (srhip_vit_fork, in place)."""
    _call("srhip_vit_fork", _p(x), _p(ln), _p(parent), n_new, dst0, rows_per_node, D, _s())


def vit_fanout(node_logits, node_feat, n_nodes, col_node, col_rows, n_cols, logits_all, feat_all, C, D):
    """logits_all[col_rows[g]] = node_logits[col_node[g]], feat_all[col_rows[g]] = node_feat[col_node[g]] for g < n_cols (srhip_vit_fanout).
    A row is written in both tables, so it is bounded by the shorter of the two."""
    _call("srhip_vit_fanout", _p(node_logits), _p(node_feat), n_nodes, _p(col_node), _p(col_rows), n_cols, _p(logits_all), _p(feat_all),
          min(logits_all.shape[0], feat_all.shape[0]), C, D, _s())


# ---- score filter -----------------------------------------------------------------------------
def row_max(inp, in_is_probs, probs_out, max_probs, max_idx, B, C):
    _call("srhip_row_max", _p(inp), int(in_is_probs), _p(probs_out), _p(max_probs), _p(max_idx), B, C, _s())


def row_max_strided(base, first_row, in_is_probs, probs_out, max_probs, max_idx, B, C, rows_per_group, group_rows):
    """row_max over B rows read in place from the contiguous [*, C] buffer ``base``: row r is buffer row
    first_row + (r // rows_per_group) * group_rows + r % rows_per_group."""
    _call("srhip_row_max_strided", _pa(base, first_row * C), int(in_is_probs), _p(probs_out), _p(max_probs), _p(max_idx), B, C, rows_per_group,
          group_rows * C, _s())


def flexmatch_mask(max_probs, max_idx, idx_ulb, p_cutoff, selected_label, hist, classwise_acc, mask, B, C, ulb_dest_len,
                   thresh_warmup):
    _call("srhip_flexmatch_mask", _p(max_probs), _p(max_idx), _p(idx_ulb), p_cutoff, _p(selected_label), _p(hist),
          _p(classwise_acc), _p(mask), B, C, ulb_dest_len, int(thresh_warmup), _s())


def flexmatch_mask_passes(max_probs, max_idx, idx_ulb, p_cutoff, selected_label, hist, classwise_acc, mask, n_pass, B, C, ulb_dest_len,
                          thresh_warmup):
    """n_pass masking calls in pass order in one launch; max_probs / max_idx / mask are [n_pass * B]."""
    _call("srhip_flexmatch_mask_passes", _p(max_probs), _p(max_idx), _p(idx_ulb), p_cutoff, _p(selected_label), _p(hist),
          _p(classwise_acc), _p(mask), n_pass, B, C, ulb_dest_len, int(thresh_warmup), _s())


def flexmatch_rebuild_hist(selected_label, hist, ulb_dest_len, C):
    _call("srhip_flexmatch_rebuild_hist", _p(selected_label), _p(hist), ulb_dest_len, C, _s())


def fixed_mask(max_probs, p_cutoff, mask, B):
    _call("srhip_fixed_mask", _p(max_probs), p_cutoff, _p(mask), B, _s())


def freematch_stats(probs, max_idx, colsum, hist, B, C):
    _call("srhip_freematch_stats", _p(probs), _p(max_idx), _p(colsum), _p(hist), B, C, _s())


def freematch_update(maxp_all, n_all, colsum, hist, max_probs, max_idx, time_p, p_model, label_hist, mask, B, C, m, use_quantile, clip_thresh):
    import numpy as np
    _call("srhip_freematch_update", _p(maxp_all), n_all, _p(colsum), _p(hist), _p(max_probs), _p(max_idx), _p(time_p), _p(p_model),
          _p(label_hist), _p(mask), B, C, float(np.float32(m)), float(np.float32(1 - m)), int(use_quantile), int(clip_thresh), _s())


def distalign(probs, colsum_ulb, n_ulb, colsum_lb, n_lb, p_model, p_target, inited, momentum, aligned, max_probs, max_idx, B, C):
    _call("srhip_distalign", _p(probs), _p(colsum_ulb), n_ulb, _p(colsum_lb), n_lb, _p(p_model), _p(p_target), _p(inited), float(momentum),
          _p(aligned), _p(max_probs), _p(max_idx), B, C, _s())


def softmatch_mask(maxp_all, n_all, max_probs, mu_var, momentum, n_sigma, mask, B):
    _call("srhip_softmatch_mask", _p(maxp_all), n_all, _p(max_probs), _p(mu_var), float(momentum), int(n_sigma), _p(mask), B, _s())


def freematch_entropy(logits, mask, p_model, label_hist, grad_scale, loss_out, dlogits, ws, B, C, accumulate=False):
    _call("srhip_freematch_entropy", _p(logits), _p(mask), _p(p_model), _p(label_hist), grad_scale, _p(loss_out), _p(dlogits), _p(ws),
          B, C, int(accumulate), _s())


def reward_mask2(reward, mask2, mean_out, groups, B, mean_in=None, total=None):
    """total (rows in all, groups == ceil(total / B)): the last group holds the rows that are left and takes its own mean over them."""
    if total is not None and total != groups * B:
        assert mean_in is None and groups == -(-total // B)
        _call("srhip_reward_mask2_ragged", _p(reward), _p(mask2), _p(mean_out), total, B, _s())
        return
    _call("srhip_reward_mask2", _p(reward), _p(mask2), _p(mean_out), _p(mean_in), groups, B, _s())


def reward_topk_mask(reward, mask2, groups, B, k, total=None, k_last=None, peers=None, self_peer=0):
    """The opt-in top-k reward filter (srhip_reward_topk_mask): per group of B rows the k best rewards, NaN never, ties to the lower index.
    total (rows in all, groups == ceil(total / B)): the last group holds the rows that are left and keeps k_last (default k) of them.
    peers fp32 [n_peers, groups * B] (row ``self_peer`` equal to ``reward``): the candidates of a group are its rows on every peer."""
    total = groups * B if total is None else total
    n_peers = 0 if peers is None else int(peers.shape[0])
    if _CHECK_ARGS and peers is not None:
        assert peers.dim() == 2 and peers.shape[1] == groups * B and peers.dtype == torch.float32
    _call("srhip_reward_topk_mask", _p(reward), _p(mask2), groups, B, total, int(k), int(k if k_last is None else k_last), _p(peers), n_peers,
          int(self_peer) if peers is not None else 0, _s())


def masked_ce(logits, targets, mask, mask2, grad_scale, loss_out, dlogits, B, C):
    _call("srhip_masked_ce", _p(logits), _p(targets), _p(mask), _p(mask2), grad_scale, _p(loss_out), _p(dlogits), B, C, _s())


def _rows(t):
    """(pointer, row stride in elements) of a 2-D device tensor whose rows are dense (a row block or column block of a larger buffer)."""
    if t is None:
        return None, 0
    if _CHECK_ARGS:
        assert t.is_cuda and t.dim() == 2 and t.stride(1) == 1 and t.dtype == torch.float32, "libsrhip needs fp32 device rows, dense in the last dimension"
    return t.data_ptr(), t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def ce_hard(logits, targets, mask, mask2, grad_scale, reduction, loss_rows, loss_out, dlogits, B, C):
    """Hard-target cross entropy with ``reduction`` REDUCE_NONE | REDUCE_MEAN | REDUCE_SUM (criterions.hip); logits / dlogits may be row-strided."""
    (z, ld), (dl, ldd) = _rows(logits), _rows(dlogits)
    _call("srhip_ce_hard", z, ld, _p(targets), _p(mask), _p(mask2), grad_scale, reduction, _p(loss_rows), _p(loss_out), dl, ldd, B, C, _s())


def _soft_criterion(name, logits, targets, mask, mask2, grad_scale, reduction, loss_rows, loss_out, dlogits, B, C):
    (z, ld), (t, ldt), (dl, ldd) = _rows(logits), _rows(targets), _rows(dlogits)
    _call(name, z, ld, t, ldt, _p(mask), _p(mask2), grad_scale, reduction, _p(loss_rows), _p(loss_out), dl, ldd, B, C, _s())


def ce_soft(logits, targets, mask, mask2, grad_scale, reduction, loss_rows, loss_out, dlogits, B, C):
    """Soft-target cross entropy sum_c -t log_softmax(z) (targets fp32 [B, C], not normalised)."""
    _soft_criterion("srhip_ce_soft", logits, targets, mask, mask2, grad_scale, reduction, loss_rows, loss_out, dlogits, B, C)


def consistency_mse(logits, targets, mask, mask2, grad_scale, reduction, loss_rows, loss_out, dlogits, B, C):
    """mean_c (softmax(z) - t)^2 per row."""
    _soft_criterion("srhip_consistency_mse", logits, targets, mask, mask2, grad_scale, reduction, loss_rows, loss_out, dlogits, B, C)


def consistency_l1(logits, targets, mask, mask2, grad_scale, reduction, loss_rows, loss_out, dlogits, B, C):
    """mean_c |z - t| per row."""
    _soft_criterion("srhip_consistency_l1", logits, targets, mask, mask2, grad_scale, reduction, loss_rows, loss_out, dlogits, B, C)


# ---- evaluation accumulators ----------------------------------------------------------------------
EVAL_STATE_WORDS = 8          # srhip_eval_accumulate's state {double loss_sum, nll_sum; int64 rows, kept} in int32 words


def eval_accumulator(C, device):
    """A zeroed int32 block [8 + (C + 1) * C] holding the state and the confusion matrix of srhip_eval_accumulate side by side, so that ONE
    copy brings both to the host: returns (block, state view, confusion view [C + 1, C])."""
    block = torch.zeros(EVAL_STATE_WORDS + (C + 1) * C, dtype=torch.int32, device=device)
    return block, block[:EVAL_STATE_WORDS], block[EVAL_STATE_WORDS:].view(C + 1, C)


def eval_accumulator_read(block, C):
    """The block of eval_accumulator on the host (one transfer, synchronises): (confusion int32 [C + 1, C], loss_sum, nll_sum, rows, kept)."""
    import numpy as np
    h = block.cpu().numpy()
    st = h[:EVAL_STATE_WORDS]
    f, n = st.view(np.float64), st.view(np.int64)
    return h[EVAL_STATE_WORDS:].reshape(C + 1, C), float(f[0]), float(f[1]), int(n[2]), int(n[3])


def eval_accumulate(logits, y, confusion, state, pred_out=None, row_offset=0):
    """One evaluation batch into the device accumulators (srhip_eval_accumulate): logits fp32 [B, C] (rows may be strided), y int64 [B];
    confusion int32 [C + 1, C] and state (8 int32 words, 8-byte aligned) are the caller's and start at zero; pred_out int64 (optional)
    receives the predictions at row_offset .. row_offset + B - 1."""
    z, ld = _rows(logits)
    B, C = int(logits.shape[0]), int(logits.shape[1])
    if _CHECK_ARGS:
        assert y.dtype == torch.int64 and y.numel() == B
        assert confusion.dtype == torch.int32 and confusion.numel() == (C + 1) * C
        assert state.dtype == torch.int32 and state.numel() == EVAL_STATE_WORDS
        assert pred_out is None or (pred_out.dtype == torch.int64 and 0 <= row_offset and row_offset + B <= pred_out.numel())
    _call("srhip_eval_accumulate", z, ld, _p(y), _p(confusion), _p(state), _p(pred_out), row_offset, B, C, _s())


# ---- pseudo-label quality monitor -----------------------------------------------------------------
PL_HEADER_WORDS, PL_BINS, PL_SUMS = 16, 32, 4          # srhip_pl_monitor's state layout (include/srhip.h)


def pl_monitor_words(C):
    """int64 words of srhip_pl_monitor's integer state: the header, 2 * C per-class counters, 2 * 32 histogram bins."""
    return PL_HEADER_WORDS + 2 * C + 2 * PL_BINS


def pl_monitor(pseudo, mask0, mask_kept, mask2, reward, idx_ulb, ulb_targets, P, nu, C, istate, fstate):
    """One training step into the monitor's device counters (srhip_pl_monitor): pseudo int64 [P * nu], mask0 / mask_kept fp32 [nu] (the
    confidence masks of pass 0 and of the kept pass P - 1), mask2 / reward fp32 [(P - 1) * nu] or None when P == 1, idx_ulb int64 [nu],
    ulb_targets int64 [n_ulb]; istate int64 [pl_monitor_words(C)] and fstate float64 [4] are the caller's and start at zero."""
    if _CHECK_ARGS:
        assert pseudo.dtype == torch.int64 and pseudo.numel() >= P * nu and idx_ulb.dtype == torch.int64 and idx_ulb.numel() == nu
        assert mask0.dtype == torch.float32 and mask0.numel() >= nu and mask_kept.dtype == torch.float32 and mask_kept.numel() >= nu
        assert P == 1 or (mask2.dtype == torch.float32 and mask2.numel() >= (P - 1) * nu and reward.dtype == torch.float32 and
                          reward.numel() >= (P - 1) * nu)
        assert ulb_targets.dtype == torch.int64 and istate.dtype == torch.int64 and istate.numel() == pl_monitor_words(C)
        assert fstate.dtype == torch.float64 and fstate.numel() == PL_SUMS
    _call("srhip_pl_monitor", _p(pseudo), _p(mask0), _p(mask_kept), _p(mask2), _p(reward), _p(idx_ulb), _p(ulb_targets),
          int(ulb_targets.numel()), P, nu, C, _p(istate), _p(fstate), _s())


# ---- scoring a whole unlabelled set (score_rows.hip) ----------------------------------------------
SCORE_MODES = {"fixed": _lib.SCORE_FIXED, "flex": _lib.SCORE_FLEX, "free": _lib.SCORE_FREE, "soft": _lib.SCORE_SOFT}
SCORE_COLUMNS = (("label", torch.int64), ("conf", torch.float32), ("margin", torch.float32), ("entropy", torch.float32),
                 ("weight", torch.float32))                                   # what srhip_score_rows writes, dense [B]
TABLE_COLUMNS = SCORE_COLUMNS + (("reward", torch.float32), ("reward_keep", torch.uint8), ("selected", torch.uint8),
                                 ("count", torch.int32))                      # what srhip_score_commit scatters, [n]


def score_rows(logits, mode, out, p_cutoff=0.0, classwise_acc=None, time_p=None, p_model=None, mu_var=None, n_sigma=0, da_p_model=None,
               da_p_target=None, da_inited=None):
    """One batch of logits (fp32 [B, C], rows may be strided) -> the five dense columns of SCORE_COLUMNS in ``out`` (a dict of [>= B] device
    tensors): label / conf as ops.row_max gives them, margin, entropy, and the threshold rule's mask or weight from the state passed in, which
    is only read (srhip_score_rows).  mode: 'fixed' | 'flex' | 'free' | 'soft' or the integer."""
    z, ld = _rows(logits)
    B, C = int(logits.shape[0]), int(logits.shape[1])
    if _CHECK_ARGS:
        for k, dt in SCORE_COLUMNS:
            assert out[k].dtype == dt and out[k].numel() >= B and out[k].is_cuda and out[k].is_contiguous(), k
    _call("srhip_score_rows", z, ld, B, C, SCORE_MODES.get(mode, mode), float(p_cutoff), _p(classwise_acc), _p(time_p), _p(p_model),
          _p(mu_var), int(n_sigma), _p(da_p_model), _p(da_p_target), _p(da_inited), _p(out["label"]), _p(out["conf"]), _p(out["margin"]),
          _p(out["entropy"]), _p(out["weight"]), _s())


def score_commit(batch, reward, reward_keep, table, B, idx=None, row_offset=0):
    """Scatter one scored batch (``batch``: the dict score_rows filled; reward fp32 [B]; reward_keep the fp32 mask ops.reward_mask2 wrote)
    into ``table``, a dict of the [n] device columns of TABLE_COLUMNS, at idx[b] (int64, unique within the batch) or row_offset + b
    (srhip_score_commit).  An index outside [0, n) is skipped and raises IndexError at the next ops.check_label_errors()."""
    n = int(table["label"].numel())
    if _CHECK_ARGS:
        for k, dt in TABLE_COLUMNS:
            assert table[k].dtype == dt and table[k].numel() == n and table[k].is_cuda and table[k].is_contiguous(), k
        assert reward.dtype == torch.float32 and reward.numel() >= B and reward_keep.dtype == torch.float32 and reward_keep.numel() >= B
        assert idx is None or (idx.dtype == torch.int64 and idx.numel() >= B)
    _call("srhip_score_commit", _p(batch["label"]), _p(batch["conf"]), _p(batch["margin"]), _p(batch["entropy"]), _p(batch["weight"]),
          _p(reward), _p(reward_keep), _p(idx), int(row_offset), B, n, _p(table["label"]), _p(table["conf"]), _p(table["margin"]),
          _p(table["entropy"]), _p(table["weight"]), _p(table["reward"]), _p(table["reward_keep"]), _p(table["selected"]), _p(table["count"]),
          _s())


# ---- rewarder / generator ---------------------------------------------------------------------
def rewarder_param_count(F, L):
    return int(_lib.lib().srhip_rewarder_param_count(F, L))


def rewarder_ws_floats(G, B):
    return int(_lib.lib().srhip_rewarder_ws_floats(G, B))


def generator_param_count(F):
    return int(_lib.lib().srhip_generator_param_count(F))


def rewarder_t_floats(F):
    return int(_lib.lib().srhip_rewarder_t_floats(F))


def generator_t_floats(F):
    return int(_lib.lib().srhip_generator_t_floats(F))


def rewarder_prepare(params, params_t, F, L):
    _call("srhip_rewarder_prepare", _p(params), _p(params_t), F, L, _s())


def generator_prepare(params, params_t, F):
    _call("srhip_generator_prepare", _p(params), _p(params_t), F, _s())


def rewarder_fwd(params, params_t, feats, labels, reward, ws, G, B, F, L, save_for_bwd=False, feats_first_row=0, group_rows=None,
                 max_reward=None):
    """feats [G * B, F] dense, or (group_rows given) a contiguous [*, F] buffer in which group g's B rows start at row
    feats_first_row + g * group_rows.  max_reward (0-d device tensor; G == 1, B <= 8): updated to max(max_reward, mean(reward)) in place."""
    if group_rows is None and max_reward is None:
        _call("srhip_rewarder_fwd", _p(params), _p(params_t), _p(feats), _p(labels), _p(reward), _p(ws), G, B, F, L, int(save_for_bwd), _s())
    else:
        _call("srhip_rewarder_fwd_strided", _p(params), _p(params_t), _pa(feats, feats_first_row * F), (group_rows if group_rows else B) * F,
              _p(labels), _p(reward), _p(ws), _p(max_reward), G, B, F, L, int(save_for_bwd), _s())


def rewarder_bwd(params, feats, labels, target, ws, grads, losses, B, F, L):
    _call("srhip_rewarder_bwd", _p(params), _p(feats), _p(labels), _p(target), _p(ws), _p(grads), _p(losses), B, F, L, _s())


def generator_fwd(params, params_t, x, out, label, B, F):
    _call("srhip_generator_fwd", _p(params), _p(params_t), _p(x), _p(out), _p(label), B, F, _s())


def sr_target(gen, ref, target, B, num_classes=0):
    _call("srhip_sr_target", _p(gen), _p(ref), _p(target), B, num_classes, _s())


_LABEL_ERR = ("a label outside [0, label_dim) reached the rewarder's nn.Embedding (semireward.py:57)",
              "a label outside [0, label_dim) reached the embedding gradient (semireward.py:57)",
              "the generator output is NaN or not representable as int64 (srflexmatch.py:158-159)",
              "a label outside [0, num_classes) reached F.one_hot of the SR target (srflexmatch.py:180-181, :195-196)",
              "an evaluation label outside [-1, num_classes) reached F.cross_entropy (algorithmbase.py:407)",
              "an idx_ulb entry outside [0, len(ulb_targets)) or a true label >= num_classes reached the pseudo-label monitor "
              "(monitor_pseudo_labels)")
# bit 6 (srhip_score_commit), kept beside the tuple: its length is the number of bits the training step's launches can set
_SCORE_ERR_BIT = 6
_SCORE_ERR = "a row index outside [0, n) reached the pseudo-label table (score_unlabeled: idx_ulb, or more rows than the table holds)"


def check_label_errors(reset=True):
    """Raises IndexError if a rewarder / generator launch since the last check saw an out-of-range label -- the error the reference raises
    from nn.Embedding / F.one_hot at the call itself.  Synchronises the current stream: call it where the host waits anyway."""
    import ctypes
    bits, ibits = ctypes.c_int(0), ctypes.c_int(0)
    _call("srhip_label_error", ctypes.addressof(bits), int(reset), _s())
    _call("srhip_index_error", ctypes.addressof(ibits), int(reset), _s())
    msgs = [m for i, m in enumerate(_LABEL_ERR) if bits.value >> i & 1]
    if bits.value >> _SCORE_ERR_BIT & 1:
        msgs.append(_SCORE_ERR)
    if ibits.value:
        msgs.append("an idx_ulb entry outside [0, ulb_dest_len) reached FlexMatchThresholdingHook.update (srflexmatch/utils.py:59)")
    if msgs:
        raise IndexError("libsrhip: " + "; ".join(msgs))


def adam_flat(p, g, m, v, n, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, dyn=None):
    """dyn (device address of fp32 [2] = the step's bias corrections): srhip_adam_flat_dyn, ``step`` is then ignored."""
    if dyn is not None:
        _call("srhip_adam_flat_dyn", _p(p), _p(g), _p(m), _p(v), n, lr, beta1, beta2, eps, dyn, _s())
        return
    _call("srhip_adam_flat", _p(p), _p(g), _p(m), _p(v), n, lr, beta1, beta2, eps, step, _s())


def adam_bias_corrections(beta1, beta2, step):
    """(1 - beta1^step, sqrt(1 - beta2^step)) in the fp32 arithmetic of the optimizer launches (host function of the library)."""
    import ctypes
    out = (ctypes.c_float * 2)()
    _call("srhip_adam_bias_corrections", beta1, beta2, int(step), ctypes.cast(out, ctypes.c_void_p))
    return float(out[0]), float(out[1])


def adamw_flat(p, g, m, v, p_bf16, ema, chunk_table, n_chunks, lr_t, wd_t, lr_factor, step, beta1=0.9, beta2=0.999, eps=1e-8,
               ema_m=0.0, grad_scale=1.0, zero_grad=True, clip_coef=None, dyn=None):
    """dyn (device address of fp32 [3] = lr_factor and the step's two bias corrections): srhip_adamw_flat_dyn; lr_factor / step are then ignored."""
    if dyn is not None:
        _call("srhip_adamw_flat_dyn", _p(p), _p(g), _p(m), _p(v), _p(p_bf16), _p(ema), _p(chunk_table), n_chunks, _p(lr_t), _p(wd_t),
              dyn, beta1, beta2, eps, float(ema_m), grad_scale, _p(clip_coef), int(zero_grad), _s())
        return
    _call("srhip_adamw_flat", _p(p), _p(g), _p(m), _p(v), _p(p_bf16), _p(ema), _p(chunk_table), n_chunks, _p(lr_t), _p(wd_t),
          lr_factor, beta1, beta2, eps, step, float(ema_m), grad_scale, _p(clip_coef), int(zero_grad), _s())


def clip_grad_coef(g, n, pre_scale, max_norm, ws, coef_out):
    """coef_out[0] = min(1, max_norm / (||pre_scale * g|| + 1e-6)), coef_out[1] = the norm (clip_grad_norm_, param_update.py:34-35)."""
    _call("srhip_clip_grad_coef", _p(g), n, pre_scale, max_norm, _p(ws), _p(coef_out), _s())


def clip_grad_ws_floats():
    from ._lib import lib
    return int(lib().srhip_clip_grad_ws_floats())


# ---- WideResNet building blocks (classic_cv parity configuration) ---------------------------------------------------------------
def nchw_to_nhwc_bf16(img, out, B, C, H, W):
    _call("srhip_nchw_to_nhwc_bf16", _p(img), _p(out), B, C, H, W, _s())


def im2col(act, col, B, H, W, C, ksize, stride, Kpad):
    _call("srhip_im2col", _p(act), _p(col), B, H, W, C, ksize, stride, Kpad, _s())


def im2col_bn(x, stats, gamma, beta, slope, mode, col, B, H, W, C, ksize, stride, Kpad):
    m, i = stats if stats is not None else (None, None)
    _call("srhip_im2col_bn", _p(x), _p(m), _p(i), _p(gamma), _p(beta), slope, mode, _p(col), B, H, W, C, ksize, stride, Kpad, _s())


def col2im(dcol, dact, B, H, W, C, ksize, stride, Kpad, accumulate=False):
    _call("srhip_col2im", _p(dcol), _p(dact), B, H, W, C, ksize, stride, Kpad, int(accumulate), _s())


def conv_weight_prep(Wf, Wb, WbT, Cout, C, ksize, Kpad):
    _call("srhip_conv_weight_prep", _p(Wf), _p(Wb), _p(WbT), Cout, C, ksize, Kpad, _s())


CONV_DESC_DTYPE = [("a", "<u8"), ("b", "<u8"), ("c", "<u8"), ("Cout", "<i4"), ("C", "<i4"), ("kk", "<i4"), ("Kpad", "<i4"), ("start", "<i8")]


def make_conv_desc(entries, device, per_entry):
    """entries: (a, b, c or None, Cout, C, ksize, Kpad); per_entry(Cout, C, kk, Kpad) = elements of the flat index space an entry covers.
    Returns (device table, n, total)."""
    import numpy as np
    arr = np.zeros(len(entries), dtype=CONV_DESC_DTYPE)
    t = 0
    for i, (a, b, c, Cout, C, ks, Kpad) in enumerate(entries):
        arr[i] = (_p(a), _p(b), _p(c) or 0, Cout, C, ks * ks, Kpad, t)
        t += per_entry(Cout, C, ks * ks, Kpad)
    assert arr.itemsize == 48
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device), len(entries), t


def conv_weight_prep_grouped(desc, n, total):
    _call("srhip_conv_weight_prep_grouped", _p(desc), n, total, _s())


def conv_weight_flip_grouped(desc, n, total):
    _call("srhip_conv_weight_flip_grouped", _p(desc), n, total, _s())


def add_unpad_grouped(desc, n, total):
    _call("srhip_add_unpad_grouped", _p(desc), n, total, _s())


def add_unpad(src, dst, Cout, C, ksize, Kpad):
    _call("srhip_add_unpad", _p(src), _p(dst), Cout, C, ksize, Kpad, _s())


def bn_ws_doubles():
    from ._lib import lib
    return int(lib().srhip_bn_ws_doubles())


def wrn_conv_supported(Cin, Cout, ksize):
    from ._lib import lib
    return bool(lib().srhip_wrn_conv_supported(Cin, Cout, ksize))


def bn_acc_doubles(C):
    from ._lib import lib
    return int(lib().srhip_bn_acc_doubles(C))


def wrn_conv_last_kernel():
    """Name of the kernel template the last srhip_wrn_conv_bn[_passes] call launched (srhip_wrn_conv_last_plan)."""
    return wrn_conv_kernel_name(int(_lib.lib().srhip_wrn_conv_last_plan()))


WrnConvPlan = collections.namedtuple("WrnConvPlan", "kernel grid_x rounds")


def wrn_conv_kernel_name(c):
    return "wrn_conv_tile_kernel<%d, %d>" % ((c - 100) // 10, c % 10) if c >= 100 else "wrn_conv_kernel<%d, %d>" % (c // 10, c % 10)


def wrn_conv_plan(B, H, W, Cin, Cout, ksize, stride, passes=1):
    """What srhip_wrn_conv_bn[_passes] launches for this shape (host logic, no launch; srhip_wrn_conv_plan): the kernel template by the name
    wrn_conv_last_kernel() gives, gridDim.x, and the direct kernel's grid-stride loop count (1 for the tile kernel)."""
    v = [ctypes.c_int(0) for _ in range(3)]
    rc = int(_lib.lib().srhip_wrn_conv_plan(B, H, W, Cin, Cout, ksize, stride, int(passes), *[ctypes.addressof(x) for x in v]))
    if rc != 0:
        _lib.check(rc, "srhip_wrn_conv_plan")
    return WrnConvPlan(wrn_conv_kernel_name(v[0].value), v[1].value, v[2].value)


def wrn_conv_bn(xin, in_mode, in_stats, in_acc, in_gamma, in_beta, in_eps, slope, Wb, resid, y, B, H, W, Cin, Cout, ksize, stride, Kpad,
                publish=None, running=None, momentum=0.0, update_running=False, acc_out=None, stat_ranks=1, passes=1):
    """y = conv(f(xin)) (+ resid).  in_mode 0: in_stats = (mean, invstd); 1: (running_mean, running_var); 2: raw; 3: statistics folded from
    in_acc.  publish = (mean, invstd) buffers workgroup (0,0) fills from in_acc (+ running = (running_mean, running_var) moved when
    update_running).  acc_out: accumulator of the BatchNorm that reads y next (sums of y are added)."""
    im, ii = in_stats if in_stats is not None else (None, None)
    pm, pi = publish if publish is not None else (None, None)
    rm, rv = running if running is not None else (None, None)
    """passes > 1: that many independent forwards of B images each in the one launch (pass-major tensors, see srhip_wrn_conv_bn_passes)."""
    args = (_p(xin), in_mode, _p(im), _p(ii), _p(in_acc), _p(in_gamma), _p(in_beta), in_eps, slope, _p(pm), _p(pi), _p(rm),
            _p(rv), momentum, int(update_running), _p(Wb), _p(resid), _p(y), B, H, W, Cin, Cout, ksize, stride, Kpad, _p(acc_out), stat_ranks,
            int(passes), _s())
    if _PROFILE is not None:
        npix = y.shape[0]                   # (all passes)
        # algorithmic work: the convolution's MACs; bytes: the fp32 input once, the fp32 output (+ residual) once, the filter once
        _PROFILE.timed("srhip_wrn_conv_bn_passes", args, 2.0 * npix * Cin * ksize * ksize * Cout, wrn_conv_last_kernel,
                       4.0 * passes * B * H * W * Cin + 4.0 * npix * Cout * (2 if resid is not None else 1) + 2.0 * Cout * Kpad)
        return
    _call("srhip_wrn_conv_bn_passes", *args)


def wrn_head(x, in_mode, in_stats, in_acc, gamma, beta, eps, slope, Wc, bc, feat, logits, B, HW2, C, K, publish=None, running=None,
             momentum=0.0, update_running=False, stat_ranks=1, passes=1):
    im, ii = in_stats if in_stats is not None else (None, None)
    pm, pi = publish if publish is not None else (None, None)
    rm, rv = running if running is not None else (None, None)
    _call("srhip_wrn_head_passes", _p(x), in_mode, _p(im), _p(ii), _p(in_acc), _p(gamma), _p(beta), eps, slope, _p(pm), _p(pi), _p(rm), _p(rv), momentum,
          int(update_running), _p(Wc), _p(bc), _p(feat), _p(logits), B, HW2, C, K, stat_ranks, int(passes), _s())


BN_CHAIN_DESC_DTYPE = [("acc", "<u8"), ("running_mean", "<u8"), ("running_var", "<u8"), ("C", "<i4"), ("rows", "<i4")]


def make_bn_chain_desc(entries, device):
    """entries: (acc [groups, bn_acc_doubles(C)] fp64, running_mean, running_var, C, rows).  Returns (device table, n) for bn_running_chain."""
    import numpy as np
    arr = np.zeros(len(entries), dtype=BN_CHAIN_DESC_DTYPE)
    for i, (acc, rm, rv, C, rows) in enumerate(entries):
        assert 0 < C <= 256 and rows > 0
        arr[i] = (_p(acc), _p(rm), _p(rv), C, rows)
    assert arr.itemsize == 32
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device), len(entries)


def bn_running_chain(desc, n, groups, momentum):
    """Every statistics group of a shared-launch forward moves the running statistics, in group order (srhip_bn_running_chain)."""
    _call("srhip_bn_running_chain", _p(desc), n, int(groups), momentum, _s())


def bn_stats(x, eps, momentum, update_running, running_mean, running_var, out_mean, out_invstd, ws, rows, C):
    _call("srhip_bn_stats", _p(x), eps, momentum, int(update_running), _p(running_mean), _p(running_var), _p(out_mean), _p(out_invstd), _p(ws),
          rows, C, _s())


def bn_act(x, stats, gamma, beta, eps, slope, mode, act, rows, C, act_f32=None):
    m, i = stats if stats is not None else (None, None)
    _call("srhip_bn_act", _p(x), _p(m), _p(i), _p(gamma), _p(beta), eps, slope, mode, _p(act), _p(act_f32), rows, C, _s())


def bn_accumulate(x, acc, rows, C):
    _call("srhip_bn_accumulate", _p(x), _p(acc), rows, C, _s())


def bn_fold(acc, rows_total, eps, momentum, update_running, running_mean, running_var, out_mean, out_invstd, totals, C):
    _call("srhip_bn_fold", _p(acc), float(rows_total), eps, momentum, int(update_running), _p(running_mean), _p(running_var), _p(out_mean),
          _p(out_invstd), _p(totals), C, _s())


def bn_bwd_reduce(dact, x, save_mean, save_invstd, gamma, beta, slope, ws, rows, C):
    _call("srhip_bn_bwd_reduce", _p(dact), _p(x), _p(save_mean), _p(save_invstd), _p(gamma), _p(beta), slope, _p(ws), rows, C, _s())


def bn_bwd_apply(dact, x, save_mean, save_invstd, gamma, beta, slope, resid, dx, dgamma, dbeta, totals, local_totals, rows_total, rows, C,
                 dx_bf16=None):
    _call("srhip_bn_bwd_apply", _p(dact), _p(x), _p(save_mean), _p(save_invstd), _p(gamma), _p(beta), slope, _p(resid), _p(dx), _p(dgamma),
          _p(dbeta), _p(totals), _p(local_totals), float(rows_total), _p(dx_bf16), rows, C, _s())


def bn_fwd(x, gamma, beta, eps, slope, momentum, training, update_running, running_mean, running_var, save_mean, save_invstd, act_bf16,
           act_f32, ws, rows, C):
    _call("srhip_bn_fwd", _p(x), _p(gamma), _p(beta), eps, slope, momentum, int(training), int(update_running), _p(running_mean),
          _p(running_var), _p(save_mean), _p(save_invstd), _p(act_bf16), _p(act_f32), _p(ws), rows, C, _s())


def bn_bwd(dact, x, save_mean, save_invstd, gamma, beta, slope, resid, dx, dgamma, dbeta, ws, rows, C):
    _call("srhip_bn_bwd", _p(dact), _p(x), _p(save_mean), _p(save_invstd), _p(gamma), _p(beta), slope, _p(resid), _p(dx), _p(dgamma),
          _p(dbeta), _p(ws), rows, C, _s())


def avgpool_fwd(act, feat, B, HW2, C):
    _call("srhip_avgpool_fwd", _p(act), _p(feat), B, HW2, C, _s())


def avgpool_bwd(dfeat, dact, B, HW2, C):
    _call("srhip_avgpool_bwd", _p(dfeat), _p(dact), B, HW2, C, _s())


def fc_fwd(feat, Wc, bc, logits, B, F, K):
    _call("srhip_fc_fwd", _p(feat), _p(Wc), _p(bc), _p(logits), B, F, K, _s())


def fc_bwd(dlogits, feat, Wc, dfeat, dWc, dbc, B, F, K):
    _call("srhip_fc_bwd", _p(dlogits), _p(feat), _p(Wc), _p(dfeat), _p(dWc), _p(dbc), B, F, K, _s())


def sgd_flat(p, g, buf, ema, table, nchunks, n, lr, momentum, grad_scale=1.0, ema_m=0.0, first_step=False, zero_grad=True, clip_coef=None):
    _call("srhip_sgd_flat", _p(p), _p(g), _p(buf), _p(ema), _p(table), nchunks, n, lr, momentum, grad_scale, _p(clip_coef), float(ema_m),
          int(first_step), int(zero_grad), _s())


# ---- post-LN encoder (BERT / Wav2Vec2) --------------------------------------------------------------
class Drop:
    """One dropout site of one forward call: (key, thresh, scale) of the counter-based generator in csrc/common.h (drop_keep: one hash per two
    neighbouring elements; the attention probabilities pair within a query row, drop_pair_hash).  ``Drop.none`` disables it.  key = fmix32(lo ^ fmix32(hi + 0x9E3779B9 * site)) of the 64-bit call seed."""
    __slots__ = ("key", "thresh", "scale")
    none = None

    def __init__(self, seed, site, p):
        self.key, self.thresh, self.scale = site_key(seed, site), int(p * 4294967296.0), 1.0 / (1.0 - p)

    def args(self):
        return self.key, self.thresh, self.scale


def _fmix32(h):
    h &= 0xFFFFFFFF
    h ^= h >> 16; h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13; h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def site_key(seed, site):
    lo, hi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    return _fmix32(lo ^ _fmix32((hi + 0x9E3779B9 * (site & 0xFFFFFFFF)) & 0xFFFFFFFF))


def _d(drop):
    return drop.args() if drop is not None else (0, 0, 1.0)


def gemm_nt_resid_dropout(A, B, C, M, N, K, bias, resid, drop, lda=None, ldb=None):
    """C(f32)[M,N] = resid (or C) + dropout(A . B^T + bias)."""
    if _PROFILE is not None:
        _PROFILE.timed("srhip_gemm_nt_resid_dropout", (_p(A), lda or K, _p(B), ldb or K, _p(C), N, M, N, K, _p(bias), _p(resid), N, *_d(drop), _s(),), 2.0 * M * N * K, _GemmProfile.kernel_name(EPI_RESID_F32, M, N, K),
                              _GemmProfile.gemm_bytes(EPI_RESID_F32, M, N, K, resid, None, 0.0))
        return
    _call("srhip_gemm_nt_resid_dropout", _p(A), lda or K, _p(B), ldb or K, _p(C), N, M, N, K, _p(bias), _p(resid), N, *_d(drop), _s())


def gemm_nt_resid_ln_dropout(A, B, C, M, N, K, bias, ln_mean, ln_rstd, ln_gamma, ln_beta, drop, lda=None, ldb=None):
    """C(f32)[M,N] = LayerNorm(C; mean, rstd, gamma, beta) + dropout(A . B^T + bias), in place: C holds the pre-LayerNorm sums of the sub-layer
    before (post-LN encoders, rows without a backward: postln_fwd(x=None) wrote only the bf16 operand and the statistics)."""
    args = (_p(A), lda or K, _p(B), ldb or K, _p(C), N, M, N, K, _p(bias), _p(ln_mean), _p(ln_rstd), _p(ln_gamma), _p(ln_beta), *_d(drop), _s())
    if _PROFILE is not None:
        _PROFILE.timed("srhip_gemm_nt_resid_ln_dropout", args, 2.0 * M * N * K, _GemmProfile.kernel_name(EPI_RESID_F32, M, N, K),
                       _GemmProfile.gemm_bytes(EPI_RESID_F32, M, N, K, None, None, 0.0))
        return
    _call("srhip_gemm_nt_resid_ln_dropout", *args)


def attn_masked_fwd(qkv, out, lse, key_len, B, N, H, scale, drop=None):
    _call("srhip_attn_masked_fwd", _p(qkv), _p(out), _p(lse), _p(key_len), B, N, H, scale, *_d(drop), _s())


def attn_masked_bwd(qkv, out, d_out, lse, dqkv, delta_ws, key_len, B, N, H, scale, drop=None):
    _call("srhip_attn_masked_bwd", _p(qkv), _p(out), _p(d_out), _p(lse), _p(dqkv), _p(delta_ws), _p(key_len), B, N, H, scale, *_d(drop), _s())


def embed_ln_fwd(ids, seq_index, word, pos, type0, gamma, beta, eps, x, xb, mean, rstd, B, L, D, drop=None):
    _call("srhip_embed_ln_fwd", _p(ids), ids.stride(0), _p(seq_index), _p(word), _p(pos), _p(type0), _p(gamma), _p(beta), eps, _p(x), _p(xb),
          _p(mean), _p(rstd), B, L, D, *_d(drop), _s())


def embed_ln_bwd(dy, ids, seq_index, word, pos, type0, mean, rstd, gamma, dword, dpos, dtype0, dgamma, dbeta, B, L, D, pad_id, drop=None):
    _call("srhip_embed_ln_bwd", _p(dy), _p(ids), ids.stride(0), _p(seq_index), _p(word), _p(pos), _p(type0), _p(mean), _p(rstd), _p(gamma),
          _p(dword), _p(dpos), _p(dtype0), _p(dgamma), _p(dbeta), B, L, D, pad_id, *_d(drop), _s())


def embed_ln_bwd_ws_floats(B, L, D):
    return int(_lib.lib().srhip_embed_ln_bwd_ws_floats(B, L, D))


def embed_ln_bwd_ordered(dy, ids, seq_index, word, pos, type0, mean, rstd, gamma, dword, dpos, dtype0, dgamma, dbeta, ws, B, L, D, pad_id, drop=None):
    """embed_ln_bwd with one summation order, no atomics (srhip.h): ``ws`` fp32 scratch of at least embed_ln_bwd_ws_floats(B, L, D) elements."""
    if _CHECK_ARGS:
        assert ws.dtype == torch.float32 and ws.numel() >= embed_ln_bwd_ws_floats(B, L, D)
    _call("srhip_embed_ln_bwd_ordered", _p(dy), _p(ids), ids.stride(0), _p(seq_index), _p(word), _p(pos), _p(type0), _p(mean), _p(rstd), _p(gamma),
          _p(dword), _p(dpos), _p(dtype0), _p(dgamma), _p(dbeta), _p(ws), B, L, D, pad_id, *_d(drop), _s())


def postln_fwd(y, gamma, beta, eps, x, xb, mean, rstd, M, D):
    _call("srhip_postln_fwd", _p(y), _p(gamma), _p(beta), eps, _p(x), _p(xb), _p(mean), _p(rstd), M, D, _s())


def postln_bwd_part(dy, y, mean, rstd, gamma, dx, dxb, part, n_rep, M, D, drop=None):
    _call("srhip_postln_bwd_part", _p(dy), _p(y), _p(mean), _p(rstd), _p(gamma), _p(dx), _p(dxb), _p(part), n_rep, M, D, *_d(drop), _s())


def postln_bwd(dy, y, mean, rstd, gamma, dx, dxb, dgamma, dbeta, M, D, drop=None):
    _call("srhip_postln_bwd", _p(dy), _p(y), _p(mean), _p(rstd), _p(gamma), _p(dx), _p(dxb), _p(dgamma), _p(dbeta), M, D, *_d(drop), _s())


def meanpool_fwd(x, feat, B, L, D, drop=None, seq_len=None):
    _call("srhip_meanpool_fwd", _p(x), _p(feat), _p(seq_len), B, L, D, *_d(drop), _s())


def meanpool_bwd(dfeat, dx, B, L, D, drop=None, seq_len=None):
    _call("srhip_meanpool_bwd", _p(dfeat), _p(dx), _p(seq_len), B, L, D, *_d(drop), _s())


def gelu_f32(pre, out, n):
    _call("srhip_gelu_f32", _p(pre), _p(out), n, _s())


def gelu_bwd_f32(dout, pre, dpre, n):
    _call("srhip_gelu_bwd_f32", _p(dout), _p(pre), _p(dpre), n, _s())


def dropout_cast(x, out, n, drop=None):
    _call("srhip_dropout_cast", _p(x), _p(out), n, *_d(drop), _s())


def mask_lengths(mask, key_len, B, L):
    _call("srhip_mask_lengths", _p(mask), mask.stride(0), _p(key_len), B, L, _s())


def gemm_nt_dropout(epi, A, B, C, M, N, K, drop, *, lda=None, ldb=None, bias=None, aux_in=None, aux_out=None, ldaux=0):
    """gemm_nt with dropout in the GELU / DGELU / RESID epilogue (ldc == N)."""
    if _PROFILE is not None:
        _PROFILE.timed("srhip_gemm_nt_dropout", (epi, _p(A), lda or K, _p(B), ldb or K, _p(C), N, M, N, K, _p(bias), _p(aux_in), _p(aux_out), ldaux, *_d(drop), _s(),), 2.0 * M * N * K, _GemmProfile.kernel_name(epi, M, N, K), _GemmProfile.gemm_bytes(epi, M, N, K, aux_in, aux_out, 0.0))
        return
    _call("srhip_gemm_nt_dropout", epi, _p(A), lda or K, _p(B), ldb or K, _p(C), N, M, N, K, _p(bias), _p(aux_in), _p(aux_out), ldaux, *_d(drop), _s())


# ---- Wav2Vec2 front end ---------------------------------------------------------------------------------
def _pa(t, off_elems=0):
    """device pointer of a (possibly offset) view into a contiguous buffer"""
    return t.data_ptr() + off_elems * t.element_size()


def w2v_conv0(mode, wave, W0, gamma, beta, ws, ws2, out, dY, dW0, dgamma, dbeta, B, S, T0, P0, C, k, stride, eps=1e-5):
    _call("srhip_w2v_conv0", mode, _p(wave), _p(W0), _p(gamma), _p(beta), _p(ws), _p(ws2), _p(out), _p(dY), _p(dW0), _p(dgamma), _p(dbeta),
          B, S, T0, P0, C, k, stride, eps, _s())


def w2v_conv_weight_prep(W, Wr, WrT, Cout, Cin, k):
    _call("srhip_w2v_conv_weight_prep", _p(W), _p(Wr), _p(WrT), Cout, Cin, k, _s())


def w2v_conv_wgrad_add(dWr, dW, Cout, Cin, k, n_part=1):
    _call("srhip_w2v_conv_wgrad_add", _p(dWr), _p(dW), Cout, Cin, k, n_part, _s())


def w2v_col2im_dgelu(dcol, pre_prev, out, B, Pl, Pprev, C, k, stride):
    _call("srhip_w2v_col2im_dgelu", _p(dcol), _p(pre_prev), _p(out), B, Pl, Pprev, C, k, stride, _s())


def w2v_featln_fwd(x, gamma, beta, eps, out, mean, rstd, B, T, P, C):
    _call("srhip_w2v_featln_fwd", _p(x), _p(gamma), _p(beta), eps, _p(out), _p(mean), _p(rstd), B, T, P, C, _s())


def w2v_featln_bwd(dy, x, pre, mean, rstd, gamma, dpre, dgamma, dbeta, B, T, P, C):
    _call("srhip_w2v_featln_bwd", _p(dy), _p(x), _p(pre), _p(mean), _p(rstd), _p(gamma), _p(dpre), _p(dgamma), _p(dbeta), B, T, P, C, _s())


def w2v_spec_mask_fwd(x, mask, embed, M, D):
    _call("srhip_w2v_spec_mask_fwd", _p(x), _p(mask), _p(embed), M, D, _s())


def w2v_spec_mask_bwd(dx, add, mask, dembed, B, T, P, Padd, D):
    _call("srhip_w2v_spec_mask_bwd", _p(dx), _p(add), _p(mask), _p(dembed), B, T, P, Padd, D, _s())


def w2v_pos_stage(src, out, B, T, P, Pp, D, groups, pad_left, rows_total):
    _call("srhip_w2v_pos_stage", _p(src), _p(out), B, T, P, Pp, D, groups, pad_left, rows_total, _s())


def w2v_weightnorm_prep(v, g, norms, Wf, Wb, D, groups, k):
    _call("srhip_w2v_weightnorm_prep", _p(v), _p(g), _p(norms), _p(Wf), _p(Wb), D, groups, k, _s())


def w2v_weightnorm_bwd(dWf, v, g, norms, dv, dg, ws, D, groups, k):
    """dv +=, dg += ; ws: fp32 workspace of at least (D + 1) * k elements (w2v_weightnorm_ws_floats)."""
    assert ws.numel() >= w2v_weightnorm_ws_floats(D, k)
    _call("srhip_w2v_weightnorm_bwd", _p(dWf), _p(v), _p(g), _p(norms), _p(dv), _p(dg), _p(ws), D, groups, k, _s())


def w2v_weightnorm_ws_floats(D, k):
    return (D + 1) * k


def w2v_pos_finish_fwd(x, conv, cbias, gamma, beta, eps, x0, x0b, ysave, mean, rstd, B, T, P, Pp, D, drop=None):
    _call("srhip_w2v_pos_finish_fwd", _p(x), _p(conv), _p(cbias), _p(gamma), _p(beta), eps, _p(x0), _p(x0b), _p(ysave), _p(mean), _p(rstd),
          B, T, P, Pp, D, *_d(drop), _s())


def w2v_pos_finish_bwd(dx0, ysave, conv, cbias, mean, rstd, gamma, dconv, dgamma, dbeta, B, T, P, Pp, D, drop=None):
    _call("srhip_w2v_pos_finish_bwd", _p(dx0), _p(ysave), _p(conv), _p(cbias), _p(mean), _p(rstd), _p(gamma), _p(dconv), _p(dgamma), _p(dbeta),
          B, T, P, Pp, D, *_d(drop), _s())


def make_group_desc_ld(problems, device, bn=128):
    """srhip_group_desc table with explicit leading dimensions / raw pointers: problems = list of (A_ptr, lda, B_ptr, ldb, C_ptr, ldc, M, N, K).
    bn = 64: the table of srhip_gemm_nt_grouped_n64_f32 (128 x 64 tiles; gemm_nt_grouped_f32(..., n64=True)).
    The kernels walk K in steps of 32 and read no partial step (srhip.h: K % 32 == 0): a table that breaks that is refused here, on the host."""
    import numpy as np
    assert all(pr[8] > 0 and pr[8] % 32 == 0 for pr in problems), "grouped products need K % 32 == 0 (srhip.h)"
    arr = np.zeros(len(problems), dtype=GROUP_DESC_DTYPE)
    t = 0
    for i, (A, lda, B, ldb, C, ldc, M, N, K) in enumerate(problems):
        arr[i] = (A, B, C, M, N, K, lda, ldb, ldc, t, 0, 0, 0)
        t += ((M + 127) // 128) * ((N + bn - 1) // bn)
    flops = float(sum(2.0 * M * N * K for *_, M, N, K in problems))
    nbytes = float(sum(2.0 * (M * K + N * K) + 8.0 * M * N for *_, M, N, K in problems))
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device), len(problems), t, flops, nbytes


def make_group_tn_desc_ld(problems, device, tile=128):
    """srhip_group_tn_desc table with explicit pointers / leading dimensions: (A_ptr, lda, B_ptr, ldb, C_ptr, ldc, dbias_ptr, M, N, K).
    tile = 256: the table of the persistent kernel (gemm_tn_grouped_f32(..., pp=True)); the caller sizes the problems so that its static walk is
    balanced (the audio front end cuts its frame axis into chunks that give one round of tiles)."""
    import numpy as np
    arr = np.zeros(len(problems), dtype=GROUP_TN_DESC_DTYPE)
    t = 0
    for i, (A, lda, B, ldb, C, ldc, db, M, N, K) in enumerate(problems):
        arr[i] = (A, B, C, db or 0, M, N, K, lda, ldb, ldc, t, 0)
        t += ((M + tile - 1) // tile) * ((N + tile - 1) // tile)
    flops = float(sum(2.0 * M * N * K for *_, M, N, K in problems))
    nbytes = float(sum(2.0 * (M * K + N * K) + 8.0 * M * N for *_, M, N, K in problems))
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device), len(problems), t, flops, nbytes


_RESIZE_TABLES = {}


def resize_bilinear_u8(src, S, chunk=4096):
    """uint8 [N, H0, H0, 3] device tensor -> new uint8 [N, S, S, 3]: Image.resize((S, S), BILINEAR) of Pillow, byte for byte (srhip.h).  The
    host tables of (H0, S) are built once and kept on the device; ``chunk`` images per launch bound the horizontal pass's scratch."""
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[-1] != 3:
        raise ValueError("resize_bilinear_u8 takes uint8 [N, H, W, 3] images, got %s %s" % (src.dtype, tuple(src.shape)))
    N, H0, W0, _ = src.shape
    if H0 != W0:
        raise ValueError("resize_bilinear_u8: square images only (the four SemiReward cv datasets are), got %d x %d" % (H0, W0))
    assert src.is_cuda and src.is_contiguous() and N > 0 and S > 0
    dst = torch.empty(N, S, S, 3, dtype=torch.uint8, device=src.device)
    if H0 == S:
        _call("srhip_resize_bilinear_u8", _p(src), N, H0, W0, _p(dst), S, None, None, 0, None, _s())
        return dst
    key = (H0, S, src.device)
    if key not in _RESIZE_TABLES:
        from .data.resize import resize_tables
        b, c, k = resize_tables(H0, S)
        _RESIZE_TABLES[key] = (torch.from_numpy(b).to(src.device), torch.from_numpy(c).to(src.device), k)
    bounds, coefs, ksize = _RESIZE_TABLES[key]
    tmp = torch.empty(min(N, chunk) * H0 * S * 3, dtype=torch.uint8, device=src.device)
    for s in range(0, N, chunk):
        n = min(chunk, N - s)
        _call("srhip_resize_bilinear_u8", _p(src[s:s + n]), n, H0, W0, _p(dst[s:s + n]), S, _p(bounds), _p(coefs), ksize, _p(tmp), _s())
    return dst


def check_wave_rows(src_row, crop_off, row_len):
    """The host-side argument check of ``wave_view``: numpy ``src_row`` / ``crop_off`` (where a loader produces them) against the numpy
    ``row_len`` of the store.  The kernel clamps such a row to an empty window; here it is an error."""
    import numpy as np
    src_row, crop_off = np.asarray(src_row), np.asarray(crop_off)
    if src_row.shape != crop_off.shape or src_row.ndim != 1:
        raise ValueError("wave_view: src_row and crop_off must be 1-D arrays of one length, got %s and %s" % (src_row.shape, crop_off.shape))
    if src_row.size and (src_row.min() < 0 or src_row.max() >= len(row_len)):
        raise IndexError("wave_view: src_row outside the store's %d rows" % len(row_len))
    if src_row.size and (crop_off.min() < 0 or (crop_off >= np.asarray(row_len)[src_row]).any()):
        raise IndexError("wave_view: crop_off outside its clip (0 <= crop_off < row_len[src_row])")


def wave_view(store, row_off, row_len, src_row, crop_off, S, normalize, host=None):
    """One view of a batch from the flat fp32 clip store (srhip.h: srhip_wave_view): row b is S samples of clip ``src_row[b]`` from sample
    ``crop_off[b]``, zero-padded, normalised like Wav2Vec2FeatureExtractor when ``normalize``.  store fp32, row_off int64, row_len int32,
    src_row int64 [B], crop_off int32 [B], all on the device -> new fp32 [B, S] (a view of a [B, ldo] allocation, ldo = S rounded up to 4:
    contiguous when S % 4 == 0).  ``host``: (src_row, crop_off, row_len) as numpy arrays, checked before the launch (check_wave_rows)."""
    if store.dtype != torch.float32 or row_off.dtype != torch.int64 or row_len.dtype != torch.int32:
        raise ValueError("wave_view: the store is fp32 with int64 row_off and int32 row_len, got %s / %s / %s" % (store.dtype, row_off.dtype, row_len.dtype))
    if src_row.dtype != torch.int64 or crop_off.dtype != torch.int32 or src_row.dim() != 1 or src_row.shape != crop_off.shape:
        raise ValueError("wave_view: src_row is int64 [B] and crop_off int32 [B], got %s %s / %s %s"
                         % (src_row.dtype, tuple(src_row.shape), crop_off.dtype, tuple(crop_off.shape)))
    if row_off.shape != row_len.shape or row_off.dim() != 1:
        raise ValueError("wave_view: row_off and row_len hold one entry per clip")
    if host is not None:
        check_wave_rows(*host)
    B, S = int(src_row.shape[0]), int(S)
    ldo = (S + 3) & ~3
    out = torch.empty(B, ldo, dtype=torch.float32, device=store.device)
    _call("srhip_wave_view", _p(store), _p(row_off), _p(row_len), int(row_len.shape[0]), _p(src_row), _p(crop_off), B, S, 1 if normalize else 0,
          _p(out), ldo, _s())
    return out if ldo == S else out[:, :S]


WAVE_COPY, WAVE_GAIN, WAVE_RESAMPLE, WAVE_REVERB = range(4)                 # srhip_wave_effect ops (srhip.h: SR_WAVE_*)
WAVE_STEP_ONE = 1 << 32                                                     # a resample step is 32.32 fixed point
FREEVERB_DELAYS = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617, 556, 441, 341, 225)      # eight combs, four allpasses, in samples at 44.1 kHz


def reverb_delays(sample_rate):
    """The 12 delays of srhip_wave_effect's reverb at ``sample_rate``: max(1, round(d * sample_rate / 44100)), halves rounded up."""
    import numpy as np
    return np.maximum(1, np.floor(np.array(FREEVERB_DELAYS, dtype=np.float64) * float(sample_rate) / 44100.0 + 0.5)).astype(np.int32)


def wave_effect_len(n, op, param):
    """The length rule of srhip_wave_effect: m = max(1, (n << 32) // step) for a resample, m = n otherwise (numpy arrays, int64 arithmetic)."""
    import numpy as np
    n, op, param = np.asarray(n, dtype=np.int64), np.asarray(op), np.asarray(param, dtype=np.int64)
    step = np.where(op == WAVE_RESAMPLE, param, WAVE_STEP_ONE)
    return np.where(op == WAVE_RESAMPLE, np.maximum(1, (n << 32) // np.maximum(step, 1)), n)


def check_wave_effect(src_row, op, param, dst_len, row_len, pitch):
    """The host-side argument check of ``wave_effect``: what the kernel cannot decide -- the rows against the store (as check_wave_rows), the
    ops and resample steps, and ``dst_len`` against the op's length rule and the pitch."""
    import numpy as np
    src_row, op, param, dst_len, row_len = (np.asarray(a) for a in (src_row, op, param, dst_len, row_len))
    if src_row.ndim != 1 or not (src_row.shape == op.shape == param.shape == dst_len.shape):
        raise ValueError("wave_effect: src_row, op, param and dst_len must be 1-D arrays of one length, got %s %s %s %s"
                         % (src_row.shape, op.shape, param.shape, dst_len.shape))
    if src_row.size == 0:
        return
    if src_row.min() < 0 or src_row.max() >= len(row_len):
        raise IndexError("wave_effect: src_row outside the store's %d rows" % len(row_len))
    if op.min() < WAVE_COPY or op.max() > WAVE_REVERB:
        raise ValueError("wave_effect: op outside 0..3 (copy, gain, resample, reverb)")
    rs = op == WAVE_RESAMPLE
    if rs.any() and (param[rs].min() < WAVE_STEP_ONE >> 1 or param[rs].max() > WAVE_STEP_ONE << 1):
        raise ValueError("wave_effect: a resample step outside [2^31, 2^33] (a speed outside [0.5, 2])")
    n = row_len[src_row].astype(np.int64)
    if n.min() <= 0 or n.max() > 1 << 30:
        raise ValueError("wave_effect: a source row of %d samples (1 .. 2^30 are supported)" % (n.min() if n.min() <= 0 else n.max()))
    want = wave_effect_len(n, op, param)
    if (dst_len != want).any():
        b = int(np.flatnonzero(dst_len != want)[0])
        raise ValueError("wave_effect: dst_len[%d] = %d, but op %d maps %d samples to %d" % (b, dst_len[b], op[b], n[b], want[b]))
    if dst_len.max() > pitch:
        raise ValueError("wave_effect: dst_len %d does not fit the destination's pitch %d" % (dst_len.max(), pitch))


def wave_effect(store, row_off, row_len, src_row, op, param, dst_len, dst, delays, host):
    """One effect slot of the device-made strong waveform view (srhip.h: srhip_wave_effect): row b of ``dst`` (fp32 [>= B, pitch], contiguous,
    pitch % 4 == 0) becomes ``dst_len[b]`` samples of clip ``src_row[b]`` of the flat fp32 ``store`` after copy / gain / resample / reverb
    (``op[b]``, ``param[b]``); the rest of the row is not written.  src_row int64, op int32, param int64, dst_len int32, all [B] on the device;
    ``delays``: the 12 reverb delays (``reverb_delays``, host int32).  ``host``: (src_row, op, param, dst_len, row_len) as numpy arrays, the
    values the device arrays were copied from: checked here (check_wave_effect) and handed to the entry, which checks them again."""
    import numpy as np
    if store.dtype != torch.float32 or row_off.dtype != torch.int64 or row_len.dtype != torch.int32:
        raise ValueError("wave_effect: the store is fp32 with int64 row_off and int32 row_len, got %s / %s / %s" % (store.dtype, row_off.dtype, row_len.dtype))
    if row_off.shape != row_len.shape or row_off.dim() != 1:
        raise ValueError("wave_effect: row_off and row_len hold one entry per clip")
    B = int(src_row.shape[0]) if src_row.dim() == 1 else -1
    if (src_row.dtype, op.dtype, param.dtype, dst_len.dtype) != (torch.int64, torch.int32, torch.int64, torch.int32) \
            or not (tuple(op.shape) == tuple(param.shape) == tuple(dst_len.shape) == (B,)):
        raise ValueError("wave_effect: src_row int64, op int32, param int64 and dst_len int32 are [B] arrays, got %s %s / %s %s / %s %s / %s %s"
                         % (src_row.dtype, tuple(src_row.shape), op.dtype, tuple(op.shape), param.dtype, tuple(param.shape), dst_len.dtype, tuple(dst_len.shape)))
    if dst.dtype != torch.float32 or dst.dim() != 2 or not dst.is_contiguous() or dst.shape[0] < B or dst.shape[1] % 4:
        raise ValueError("wave_effect: dst is a contiguous fp32 [>= B, pitch] buffer with pitch %% 4 == 0, got %s %s" % (dst.dtype, tuple(dst.shape)))
    if store.untyped_storage().data_ptr() == dst.untyped_storage().data_ptr():
        raise ValueError("wave_effect: source and destination are the same buffer (a row is read while others are written)")
    h_src, h_op, h_param, h_len, h_row_len = host
    h_op, h_param, h_len = (np.ascontiguousarray(a, dtype=t) for a, t in ((h_op, np.int32), (h_param, np.int64), (h_len, np.int32)))
    if h_op.shape != (B,):
        raise ValueError("wave_effect: the host arrays hold %s entries for %d device rows" % (h_op.shape, B))
    check_wave_effect(h_src, h_op, h_param, h_len, h_row_len, int(dst.shape[1]))
    delays = np.ascontiguousarray(delays, dtype=np.int32)
    if delays.shape != (12,):
        raise ValueError("wave_effect: delays holds the 12 reverb delays (reverb_delays(sample_rate)), got shape %s" % (delays.shape,))
    _call("srhip_wave_effect", _p(store), _p(row_off), _p(row_len), int(row_len.shape[0]), _p(src_row), _p(op), _p(param), _p(dst_len), B, _p(dst),
          int(dst.shape[1]), h_op.ctypes.data, h_param.ctypes.data, h_len.ctypes.data, delays.ctypes.data, _s())
    return dst


def check_token_rows(src_row, row_len):
    """The host-side argument check of ``token_view``: numpy ``src_row`` (where a loader produces it) against the numpy ``row_len`` of the
    store.  The kernel turns such a row into an all-pad row; here it is an error."""
    import numpy as np
    src_row = np.asarray(src_row)
    if src_row.ndim != 1 or src_row.dtype.kind not in "iu":
        raise ValueError("token_view: src_row must be a 1-D integer array, got %s %s" % (src_row.dtype, src_row.shape))
    if src_row.size and (src_row.min() < 0 or src_row.max() >= len(row_len)):
        raise IndexError("token_view: src_row outside the store's %d rows" % len(row_len))


def token_view(store, row_off, row_len, src_row, L, pad_id=0, host=None):
    """One view of a batch from the flat int32 token store (srhip.h: srhip_token_view): row b holds the first L tokens of store row
    ``src_row[b]``, right-padded with ``pad_id``.  store int32, row_off int64, row_len int32, src_row int64 [B], all on the device ->
    (ids int64 [B, L] contiguous, key_len int32 [B]).  ``host``: (src_row, row_len) as numpy arrays, checked before the launch
    (check_token_rows)."""
    if store.dtype != torch.int32 or row_off.dtype != torch.int64 or row_len.dtype != torch.int32:
        raise ValueError("token_view: the store is int32 with int64 row_off and int32 row_len, got %s / %s / %s" % (store.dtype, row_off.dtype, row_len.dtype))
    if src_row.dtype != torch.int64 or src_row.dim() != 1:
        raise ValueError("token_view: src_row is int64 [B], got %s %s" % (src_row.dtype, tuple(src_row.shape)))
    if row_off.shape != row_len.shape or row_off.dim() != 1:
        raise ValueError("token_view: row_off and row_len hold one entry per row")
    if host is not None:
        check_token_rows(*host)
    B, L = int(src_row.shape[0]), int(L)
    ids = torch.empty(B, L, dtype=torch.int64, device=store.device)
    key_len = torch.empty(B, dtype=torch.int32, device=store.device)
    _call("srhip_token_view", _p(store), _p(row_off), _p(row_len), int(row_len.shape[0]), _p(src_row), B, L, int(pad_id), _p(ids), L, _p(key_len),
          _s())
    return ids, key_len


TOKEN_CAT_MAX_SRC = 4                                                       # srhip_token_cat: the sources ride in the kernel's arguments


def token_len_bucket(L, bucket, cap):
    """The padded length ``token_len_bucket: bucket`` gives a batch of padded length L: the next multiple of ``bucket``, at most ``cap``
    (the model's positions); ``bucket`` None or 0: L."""
    L = int(L)
    return L if not bucket else max(L, min((L + bucket - 1) // bucket * bucket, int(cap)))


def token_cat(sources, L_out, pad_id=0, out=None):
    """One token batch out of up to four (srhip.h: srhip_token_cat), one launch: ``sources`` = [(ids int64 [S, L] contiguous, key_len int32
    [S], seq_len int32 [S] or None), ...] on one device -> (ids int64 [sum S, L_out], key_len int32 [sum S], seq_len int32 [sum S]); a row is
    its source row filled up with ``pad_id``, seq_len the source's own or its L.  ``out``: the three outputs (contiguous, of exactly these
    shapes) -- nothing is allocated then.  Refused here, before anything is launched: no or more than four sources, an L_out below a
    source's L, ids that are not contiguous, wrong dtypes or shapes."""
    sources, L_out = list(sources), int(L_out)
    if not 1 <= len(sources) <= TOKEN_CAT_MAX_SRC:
        raise ValueError("token_cat: takes 1 .. %d sources, got %d" % (TOKEN_CAT_MAX_SRC, len(sources)))
    if int(pad_id) < 0:
        raise ValueError("token_cat: pad_id is a token id, got %d" % pad_id)
    dev, total = sources[0][0].device, 0
    for j, (ids, kl, sl) in enumerate(sources):
        if ids.dtype != torch.int64 or ids.dim() != 2 or ids.shape[0] < 1 or ids.shape[1] < 1:
            raise ValueError("token_cat: ids of source %d is int64 [S, L], got %s %s" % (j, ids.dtype, tuple(ids.shape)))
        if not ids.is_contiguous():
            raise ValueError("token_cat: ids of source %d is not contiguous (strides %s)" % (j, tuple(ids.stride())))
        S, L = ids.shape
        if L > L_out:
            raise ValueError("token_cat: L_out = %d is below the L = %d of source %d" % (L_out, L, j))
        for n, t in (("key_len", kl), ("seq_len", sl)):
            if t is None and n == "seq_len":
                continue
            if t is None or t.dtype != torch.int32 or tuple(t.shape) != (S,) or not t.is_contiguous():
                raise ValueError("token_cat: %s of source %d is int32 [%d] contiguous, got %s" % (
                    n, j, S, None if t is None else "%s %s" % (t.dtype, tuple(t.shape))))
        if any(t is not None and t.device != dev for t in (ids, kl, sl)):
            raise ValueError("token_cat: every source lives on one device, source %d does not (%s)" % (j, dev))
        total += S
    if total > 65535:
        raise ValueError("token_cat: %d rows, more than the 65535 of one launch" % total)
    if out is None:
        out = (torch.empty(total, L_out, dtype=torch.int64, device=dev), torch.empty(total, dtype=torch.int32, device=dev),
               torch.empty(total, dtype=torch.int32, device=dev))
    o_ids, o_kl, o_sl = out
    if (o_ids.dtype != torch.int64 or tuple(o_ids.shape) != (total, L_out) or not o_ids.is_contiguous()
            or any(t.dtype != torch.int32 or tuple(t.shape) != (total,) or not t.is_contiguous() for t in (o_kl, o_sl))
            or any(t.device != dev for t in out)):
        raise ValueError("token_cat: out is (int64 [%d, %d], int32 [%d], int32 [%d]), contiguous, on %s" % (total, L_out, total, total, dev))
    arr = (_lib.TokenSrc * len(sources))(*[_lib.TokenSrc(_p(ids), _p(kl), _p(sl), ids.shape[0], ids.shape[1]) for ids, kl, sl in sources])
    _call("srhip_token_cat", ctypes.addressof(arr), len(sources), int(pad_id), _p(o_ids), L_out, _p(o_kl), _p(o_sl), _s())
    return o_ids, o_kl, o_sl


TOKEN_COPY, TOKEN_DELETE, TOKEN_MASK, TOKEN_CUTOFF, TOKEN_SWAP = range(5)   # srhip_token_strong ops (srhip.h: SR_TOKEN_*)
TOKEN_STRONG_MAX_LSRC = 4096                                                # the longest source row srhip_token_strong takes (row and keys share LDS)


def token_strong_len(n, op, c):
    """The length rule of one srhip_token_strong slot: n - c after a DELETE or a CUTOFF, n otherwise (numpy arrays, int64 arithmetic;
    ``c`` as the slot applies it, i.e. already inside 0 .. max(0, n - 2))."""
    import numpy as np
    n, op, c = np.asarray(n, dtype=np.int64), np.asarray(op), np.asarray(c, dtype=np.int64)
    return np.where((op == TOKEN_DELETE) | (op == TOKEN_CUTOFF), n - c, n)


def pack_token_slot(op, c, seed):
    """(op, c, seed) -> the int64 slot word of srhip_token_strong: bits 0..7 op, bits 8..31 c, bits 32..63 seed."""
    import numpy as np
    op, c, seed = (np.asarray(a, dtype=np.int64) for a in (op, c, seed))
    if op.size and (op.min() < 0 or op.max() > 0xff or c.min() < 0 or c.max() > 0xffffff or seed.min() < 0 or seed.max() > 0xffffffff):
        raise ValueError("pack_token_slot: op is 8 bits, c 24 bits and seed 32 bits, all unsigned")
    return (op.astype(np.uint64) | (c.astype(np.uint64) << np.uint64(8)) | (seed.astype(np.uint64) << np.uint64(32))).view(np.int64)


def unpack_token_slot(slot):
    """The inverse of ``pack_token_slot``: (op, c, seed) as int64 arrays."""
    import numpy as np
    w = np.ascontiguousarray(slot, dtype=np.int64).view(np.uint64)
    return tuple(a.astype(np.int64) for a in (w & np.uint64(0xff), (w >> np.uint64(8)) & np.uint64(0xffffff), w >> np.uint64(32)))


def check_token_strong(src_row, slots, L, row_len, Lsrc):
    """The host-side argument check of ``token_strong``: what the kernel would quietly mend is an error here -- a row outside the store (as
    check_token_rows), an unknown op, a count above the interior its slot meets, an ``L`` (one number, or one per row) below a row's
    predicted length.  ``slots``: the packed slot words, int64 [2, B].  Returns the predicted lengths int64 [B]."""
    import numpy as np
    src_row, slots, row_len = np.asarray(src_row), np.asarray(slots), np.asarray(row_len)
    if src_row.ndim != 1 or src_row.dtype.kind not in "iu":
        raise ValueError("token_strong: src_row must be a 1-D integer array, got %s %s" % (src_row.dtype, src_row.shape))
    if slots.shape != (2, src_row.size) or slots.dtype != np.int64:
        raise ValueError("token_strong: slots holds the two packed int64 slot words of every row, [2, %d], got %s %s" % (src_row.size, slots.dtype, slots.shape))
    if not 1 <= int(Lsrc) <= TOKEN_STRONG_MAX_LSRC:
        raise ValueError("token_strong: Lsrc = %d outside 1 .. %d" % (Lsrc, TOKEN_STRONG_MAX_LSRC))
    if src_row.size == 0:
        return np.zeros(0, dtype=np.int64)
    if src_row.min() < 0 or src_row.max() >= len(row_len):
        raise IndexError("token_strong: src_row outside the store's %d rows" % len(row_len))
    n = np.minimum(row_len[src_row].astype(np.int64), int(Lsrc))
    for s in (0, 1):
        op, c, _ = unpack_token_slot(slots[s])
        if op.max() > TOKEN_SWAP:
            raise ValueError("token_strong: slot %d holds op %d, outside 0..4 (copy, delete, mask, cutoff, swap)" % (s, op.max()))
        ni = np.maximum(n - 2, 0)
        if (c > ni).any():
            b = int(np.flatnonzero(c > ni)[0])
            raise ValueError("token_strong: slot %d of row %d asks for %d of the %d interior tokens it meets" % (s, b, c[b], ni[b]))
        n = token_strong_len(n, op, c)
    if (n > np.asarray(L, dtype=np.int64)).any():
        b = int(np.flatnonzero(n > np.asarray(L, dtype=np.int64))[0])
        raise ValueError("token_strong: L = %d is below the %d tokens row %d comes out with" % (np.broadcast_to(L, n.shape)[b], n[b], b))
    return n


def token_strong(store, row_off, row_len, src_row, slot0, slot1, L, Lsrc, pad_id=0, mask_id=103, host=None):
    """The strong view of a batch made from the clean rows of the flat int32 token store (srhip.h: srhip_token_strong): row b is store row
    ``src_row[b]`` (its first ``Lsrc`` tokens) after the two slots ``slot0[b]``, ``slot1[b]`` (``pack_token_slot``), right-padded with
    ``pad_id`` to ``L``.  store int32, row_off int64, row_len int32, src_row / slot0 / slot1 int64 [B], all on the device ->
    (ids int64 [B, L] contiguous, key_len int32 [B]), as ``token_view``.  ``host``: (src_row, slots [2, B], row_len) as numpy arrays, the
    values the device arrays were copied from, checked before the launch (check_token_strong)."""
    if store.dtype != torch.int32 or row_off.dtype != torch.int64 or row_len.dtype != torch.int32:
        raise ValueError("token_strong: the store is int32 with int64 row_off and int32 row_len, got %s / %s / %s" % (store.dtype, row_off.dtype, row_len.dtype))
    B = int(src_row.shape[0]) if src_row.dim() == 1 else -1
    if any(t.dtype != torch.int64 or tuple(t.shape) != (B,) for t in (src_row, slot0, slot1)):
        raise ValueError("token_strong: src_row, slot0 and slot1 are int64 [B], got %s"
                         % " / ".join("%s %s" % (t.dtype, tuple(t.shape)) for t in (src_row, slot0, slot1)))
    if row_off.shape != row_len.shape or row_off.dim() != 1:
        raise ValueError("token_strong: row_off and row_len hold one entry per row")
    if int(pad_id) < 0 or int(mask_id) < 0:
        raise ValueError("token_strong: pad_id and mask_id are token ids, got %d and %d" % (pad_id, mask_id))
    L, Lsrc = int(L), int(Lsrc)
    if host is not None:
        check_token_strong(host[0], host[1], L, host[2], Lsrc)
    ids = torch.empty(B, L, dtype=torch.int64, device=store.device)
    key_len = torch.empty(B, dtype=torch.int32, device=store.device)
    _call("srhip_token_strong", _p(store), _p(row_off), _p(row_len), int(row_len.shape[0]), _p(src_row), _p(slot0), _p(slot1), B, Lsrc, L,
          int(pad_id), int(mask_id), _p(ids), L, _p(key_len), _s())
    return ids, key_len
