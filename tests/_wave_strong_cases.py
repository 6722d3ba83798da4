"""The specification of the device-made strong waveform view (``device_audio_strong: True``; csrc/wave_strong.hip, srhip_wave_effect) and the cases
of tests/test_{cpu,gpu}_wave_strong.py and tools/wave_strong_time.py.  The chain is the engine's own: there is no reference output for it, the
float64 numpy restatements below ARE what the kernel has to compute.  Every function returns float64 and takes the exact arguments the kernel
takes (the attenuation, the 32.32 fixed-point step, the 12 delays).

Bounds, all derived from the arithmetic (u = 2^-24, the unit roundoff of fp32), never from what the kernel returned:

gain.      The host passes g = fp32(10^(att / 20)): within 2^-24 relative, which is at most 1 ulp of the product.  The kernel forms x * (g / peak)
           in fp64 and rounds once: 0.5 ulp.  |got - want| <= 1.5 ulp_fp32(want) before the clamp; the clamp is exact and 1-Lipschitz.

resample.  out[j] = sum_k x_k h_k over at most 66 taps, h = c sinc(c u) w(u) = sin(pi c u) w(u) / (pi u).  (a) the weights.  The kernel writes
           u = d + f, d the integer distance to the NEAREST input sample and |f| <= 1/2 (one rounding of a 32-bit fraction; f - 1 is exact), and
           expands sin(pi c (d + f)) and cos(pi (d + f) / T) by the angle-addition formulas: the factors in d come from a table computed in fp64
           and rounded (u each), the factors in f from sinpif / cospif (within 2 ulp: HIP's documented maximum error stays inside that, 4 u) of
           an argument c f that carries 3 u relative error (c, f, the product) of at most 1/2: 1.5 pi u = 4.7 u on the angle, 8.7 u in all.
           Numerator: (|sin| + |cos|) 8.7 u + the table's 2 u + two roundings <= 16.3 u.  For d != 0, |u| >= 1/2: divided by pi u that is
           10.4 u, not scaled by c.  For d = 0 the table entry is exactly {0, 1}: the numerator is sinpif(c f) itself, 7 u RELATIVE, so the
           division by a small pi c u keeps it.  pi c, the product and the divide: 3 u.  The window: the same expansion with an angle below
           pi / 32, 0.5 u + 4 u per factor in f, u per table entry, the products: 10 u, halved, plus the addition: 6 u.  The products of
           c sinc w: 3 u.  |dh| <= 10.4 u + 3 u + 6 u + 3 u = 22.4 u, taken as W_ERR = 32 u.  A tap at the very edge |u| = T may be in one
           tap set and not in the other: its window is below (pi 2^-22)^2, far inside the margin.
           (b) the sum: one rounding per fused multiply-add, <= (taps + 2) u sum |x_k h_k|.
           bound_j = 32 u sum_k |x_k| + (taps + 2) u sum_k |x_k h_k|.

reverb.    The network is linear, so a rounding made at a node reaches the output through the l1 gain of the path behind it, and a node's
           magnitude is max |x| times the l1 gain of the path before it.  All gains are computed here from impulse responses of the restatement
           (``reverb_gains``), none is a constant.  Roundings per sample, in units of u times the node's magnitude: the input 0.015f x: 2; a comb's
           new delay-line sample: 6 (24 Horner steps of the damping state 1.9, the constants 0.2f 0.8f 0.84f and the two products 2.9, the final
           fused multiply-add 1; the dropped terms of the damping recursion are below 0.2^24 = 1.7e-17 of the signal, four orders below u^2);
           the sum of eight comb outputs: 7; an allpass: its stored value 1 (reaching the output through its own loop, l1 gain 2) and its
           output 1; the output scale 3: 1.  ``reverb_bound`` adds them up.

composed.  A chain of two slots and the view: an input error e reaches a slot's output through the slot's Lipschitz constant (copy 1; gain
           2 g / peak: the scale moves with the peak; resample max_j sum_k |h_k|; reverb the network's l1 gain), and the normalised view
           (v - m) / sd moves by at most 2 e (1 + max |out|) / sd; the view's own rounding is the floor 4 ulp of tests/_wave_view_cases.py."""
import functools

import numpy as np

import _wave_view_cases as WC

U = 2.0 ** -24
ONE = 1 << 32
COPY, GAIN, RESAMPLE, REVERB = range(4)
COMB_D = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)
ALLPASS_D = (556, 441, 341, 225)
DELAYS_16K = (405, 431, 463, 492, 516, 541, 565, 587, 202, 160, 124, 82)
DELAYS_8K = (202, 216, 232, 246, 258, 270, 282, 293, 101, 80, 62, 41)
FIR = 24
W_ERR = 32.0


def delays(sample_rate):
    return [max(1, int(np.floor(d * sample_rate / 44100.0 + 0.5))) for d in COMB_D + ALLPASS_D]


# ---- the draws (datasetbase.py:12-39 restated: three uniforms, then two of {gain, pitch, speed, reverb} with replacement) -----------------------
def effect_of(speed, cents, att, which):
    """(op, param) of effect ``which`` (0 gain, 1 pitch, 2 speed, 3 reverb) with the sample's three draws."""
    if which == 0:
        return GAIN, int(np.float32(10.0 ** (att / 20.0)).view(np.uint32))
    if which == 3:
        return REVERB, 0
    s = 2.0 ** (cents / 1200.0) if which == 1 else speed
    return RESAMPLE, step_of(s)


def step_of(s):
    return int(np.floor(s * 4294967296.0 + 0.5))


def out_len(n, op, param):
    return max(1, (n << 32) // param) if op == RESAMPLE else n


# ---- the effects ------------------------------------------------------------------------------------------------------------------------------
def gain(x, g):
    """sox ``gain -n``: (clamped output, the values before the clamp).  ``g``: 10^(att / 20)."""
    x = np.asarray(x, dtype=np.float64)
    peak = np.abs(x).max()
    if peak == 0:
        return x.copy(), x.copy()
    pre = x * (g / peak)
    return np.clip(pre, -1.0, 1.0), pre


def resample(x, step, block=32768):
    """(out, sum_k |x_k h_k|, sum_k |x_k|, sum_k |h_k|, taps) per output sample: the windowed-sinc gather at the 32.32 fixed-point ``step``."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    if step == ONE:
        a = np.abs(x)
        return x.copy(), a, a, np.ones(n), np.ones(n, dtype=np.int64)
    m = max(1, (n << 32) // step)
    assert m * step < 1 << 62
    c = min(1.0, ONE / step)
    T = 16.0 / c
    K = int(T) + 1
    d = np.arange(-K, K + 1, dtype=np.int64)
    out, l1, l1x, l1h, taps = tuple(np.empty(m) for _ in range(4)) + (np.empty(m, dtype=np.int64),)
    for j0 in range(0, m, block):
        p = np.arange(j0, min(m, j0 + block), dtype=np.int64) * step
        i0, f = p >> 32, (p & 0xFFFFFFFF) * 2.0 ** -32
        k = i0[:, None] - d[None, :]                                   # u = i0 + f - k = d + f
        u = d[None, :] + f[:, None]
        ok = (k >= 0) & (k <= n - 1) & (np.abs(u) <= T)
        h = np.where(ok, c * np.sinc(c * u) * (0.5 + 0.5 * np.cos(np.pi * u / T)), 0.0)
        xk = np.where(ok, x[np.clip(k, 0, n - 1)], 0.0)
        s = slice(j0, j0 + p.size)
        out[s], l1[s], l1x[s], l1h[s], taps[s] = (xk * h).sum(1), np.abs(xk * h).sum(1), np.abs(xk).sum(1), np.abs(h).sum(1), ok.sum(1)
    return out, l1, l1x, l1h, taps


def resample_bound(l1, l1x, taps):
    return W_ERR * U * l1x + (taps + 2) * U * l1


def _comb(inp, D, fir=False):
    """One lowpass-feedback comb, sample by sample: (its output y, what it stored w).  ``fir``: the damping state as its first 24 terms."""
    n = len(inp)
    w, y = [0.0] * n, [0.0] * n
    st = 0.0
    for i in range(n):
        y[i] = w[i - D] if i >= D else 0.0
        if fir:
            st = 0.0
            for k in range(FIR - 1, -1, -1):                            # Horner from the oldest term
                st = 0.2 * st + (w[i - k - D] if i - k >= D else 0.0)
            st *= 0.8
        else:
            st = 0.8 * y[i] + 0.2 * st
        w[i] = inp[i] + 0.84 * st
    return y, w


def _allpass(inp, D):
    n = len(inp)
    v, out = [0.0] * n, [0.0] * n
    for i in range(n):
        b = v[i - D] if i >= D else 0.0
        out[i] = b - inp[i]
        v[i] = inp[i] + 0.5 * b
    return out


def reverb(x, dl, fir=False):
    """Freeverb, mono, wet only, from an empty state, the tail dropped: the sequential recursion."""
    inp = [0.015 * float(v) for v in np.asarray(x, dtype=np.float64)]
    s = np.zeros(len(inp))
    for D in dl[:8]:                                                    # summed in comb order
        s = s + np.array(_comb(inp, D, fir)[0])
    s = list(s)
    for D in dl[8:]:
        s = _allpass(s, D)
    return 3.0 * np.array(s)


@functools.lru_cache(maxsize=None)
def reverb_gains(dl, length):
    """l1 gains from impulse responses of ``length`` samples: G of the whole network (with 0.015 and 3), H[c] of comb c (input to its stored
    sample, which is also the gain of a rounding of that sample to the comb's output), A[a] of the allpasses a .. 3 in series (A[4] = 1),
    S[a] of allpass a alone, Lp[a] of the allpasses 0 .. a - 1 in series."""
    imp = [1.0] + [0.0] * (length - 1)
    G = float(np.abs(reverb(np.array(imp), dl)).sum())
    H = [float(np.abs(_comb(imp, D)[1]).sum()) for D in dl[:8]]

    def chain(ds):
        s = imp
        for D in ds:
            s = _allpass(s, D)
        return float(np.abs(s).sum())
    ap = dl[8:]
    return dict(G=G, H=H, A=[chain(ap[a:]) for a in range(5)], S=[chain(ap[a:a + 1]) for a in range(4)], Lp=[chain(ap[:a]) for a in range(4)])


def reverb_bound(dl, xmax, length):
    g = reverb_gains(tuple(dl), length)
    out = 3.0 * g["A"][0]
    e = 2.0 * g["G"] + g["G"]                                           # the input product; the output scale
    e += sum(6.0 * 0.015 * h * h * out for h in g["H"])                # the combs' stored samples
    smax = 0.015 * sum(g["H"])
    e += 7.0 * smax * out                                               # the sum of the eight comb outputs
    for a in range(4):
        e += smax * g["Lp"][a] * (2.0 * 2.0 + g["S"][a]) * 3.0 * g["A"][a + 1]
    return e * U * xmax


def ir_length(sample_rate):
    return 3 * int(sample_rate)                                         # 3 s: the response is 150 dB down


# ---- one slot and a chain, with the bound and the Lipschitz constant the composed bound needs ------------------------------------------------------
def apply(op, param, x, dl, sample_rate=16000):
    """(float64 output, bound of the fp32 kernel's error per element, Lipschitz constant of the slot)."""
    x = np.asarray(x, dtype=np.float64)
    if op == COPY or (op == RESAMPLE and param == ONE):
        return x.copy(), np.zeros(x.size), 1.0
    if op == GAIN:
        g32 = float(np.array([param], dtype=np.uint32).view(np.float32)[0])
        out, pre = gain(x, g32)
        peak = np.abs(x).max()
        return out, 1.5 * np.spacing(np.abs(pre).astype(np.float32)).astype(np.float64), (2.0 * g32 / peak if peak > 0 else 1.0)
    if op == RESAMPLE:
        out, l1, l1x, l1h, taps = resample(x, param)
        return out, resample_bound(l1, l1x, taps), float(l1h.max())
    n_ir = ir_length(sample_rate)
    return reverb(x, dl), np.full(x.size, reverb_bound(dl, np.abs(x).max(), n_ir)), reverb_gains(tuple(dl), n_ir)["G"]


def gain_want(x, att):
    """The gain case against the float64 attenuation itself (the 1.5 ulp of the issue): (clamped, before the clamp)."""
    return gain(x, 10.0 ** (att / 20.0))


def chain(x, slots, dl, sample_rate=16000):
    """Two (op, param) slots on a clip: (float64 output, bound of the device chain's error per element)."""
    err = np.zeros(len(x))
    for op, param in slots:
        x, b, lip = apply(op, param, x, dl, sample_rate)
        err = b + lip * (float(err.max()) if err.size else 0.0)
    return x, err


def view_bound(want_view, var, e):
    """The normalised view of a chain output that is within ``e``: 2 e (1 + max |out|) / sd, and the view's own 4 ulp."""
    amax = float(np.abs(want_view).max())
    return 2.0 * e * (1.0 + amax) / np.sqrt(var + 1e-7) + 4.0 * WC.ulp32(amax)


# ---- clips and kernel cases -------------------------------------------------------------------------------------------------------------------------
def clip(seed, n, amp=0.3):
    """A float32 clip: two tones and noise, a spike of +-0.9 at each end (the clipped taps at the edges are hit)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n)
    x = amp * (0.5 * np.sin(0.07 * t + seed) + 0.3 * np.sin(0.9 * t) + 0.2 * rng.standard_normal(n))
    x[0], x[-1] = 0.9, -0.9
    return x.astype(np.float32)


RESAMPLE_N = (1, 2, 3, 31, 64, 65, 255, 1000, 4099)
RESAMPLE_S = (0.5, 0.75, 1.0, 1.3, 2.0, 2.0 ** (2.0 / 1200.0), 2.0 ** (-2.0 / 1200.0))
LONG_N = (1 << 18) + 5                                                  # positions need more than fp32's fraction bits
GAIN_ATT = tuple(range(-4, 5))
REVERB_N_16K = (1, 81, 82, 83, 404, 405, 406, 588, 5000)
REVERB_N_8K = (40, 41, 42, 300)
MIXED = ((COPY, 0, 37), (GAIN, -3, 1000), (RESAMPLE, 0.5, 33), (REVERB, 0, 700), (RESAMPLE, 1.3, 4099), (GAIN, 4, 5), (RESAMPLE, 1.0, 130),
         (REVERB, 0, 83), (RESAMPLE, 2.0, 1))                           # (op, att | speed, samples): nine rows of one launch


def gain_clip(seed, n, where):
    """A clip whose peak sits at the first, the last or a middle sample."""
    x = clip(seed, n, amp=0.2)
    x[0], x[-1] = 0.05, -0.05
    x[{"first": 0, "last": n - 1, "middle": n // 2}[where]] = -0.83
    return x


# ---- a device output against the restatement: asserts every element inside its bound, returns the largest share of the bound used ------------
def gain_bits(att):
    return effect_of(1.0, 0.0, att, 0)[1]


def check_resample(x, step, got, what):
    want, l1, l1x, _, taps = resample(x.astype(np.float64), step)
    tol = resample_bound(l1, l1x, taps)
    err = np.abs(got - want)
    assert got.shape == want.shape and np.isfinite(got).all() and (err <= tol).all(), (what, float(err.max()), float(tol[err.argmax()]))
    return float((err / np.maximum(tol, 1e-300)).max())


def check_gain(x, att, got, what):
    want, pre = gain_want(x.astype(np.float64), att)
    tol = 1.5 * np.spacing(np.abs(pre).astype(np.float32)).astype(np.float64)
    err = np.abs(got - want)                                           # (the clamp is 1-Lipschitz: the bound before it holds behind it)
    assert (err <= tol).all() and np.abs(got).max() <= 1.0, (what, float((err / tol).max()))
    sure = np.abs(pre) >= 1.0 + 1e-6
    assert np.array_equal(got[sure], np.sign(pre[sure]).astype(np.float32)), what       # the clamp is exact
    return float((err / tol).max())


def check_reverb(x, dl, rate, got, what):
    want = reverb(x.astype(np.float64), dl)
    tol = reverb_bound(dl, float(np.abs(x).max()), ir_length(rate))
    err = float(np.abs(got - want).max())
    assert np.isfinite(got).all() and err <= tol, (what, err, tol)
    return err / tol


# ---- running slots on the device ---------------------------------------------------------------------------------------------------------------------
NAN_BITS = WC.NAN_BITS


def launch(clips, slots, dl, device, pitch=None):
    """One srhip_wave_effect launch over ``clips`` (row b through slots[b] = (op, param)): (the outputs, one array of dst_len[b] floats per row,
    whether everything else of the NaN-initialised destination came back untouched, the raw bits)."""
    import torch
    from semireward_amd import ops
    from semireward_amd.data.device_audio import DeviceWaveDataset
    ds = DeviceWaveDataset(clips, None, device)
    B = len(clips)
    op = np.array([s[0] for s in slots], dtype=np.int32)
    param = np.array([s[1] for s in slots], dtype=np.int64)
    n = np.array([len(c) for c in clips], dtype=np.int64)
    m = np.array([out_len(int(a), int(o), int(p)) for a, o, p in zip(n, op, param)], dtype=np.int32)
    pitch = pitch or ((int(m.max()) + 3) & ~3) + 8
    dst = torch.full((B, pitch), NAN_BITS, dtype=torch.int32, device=device).view(torch.float32)
    rows = np.arange(B, dtype=np.int64)
    dev = [torch.from_numpy(a).to(device) for a in (rows, op, param, m)]
    ops.wave_effect(ds.store, ds.row_off, ds.row_len, *dev, dst, np.asarray(dl, dtype=np.int32), host=(rows, op, param, m, ds.row_len_host))
    bits = dst.view(torch.int32).cpu().numpy()
    outs = [bits[b, :m[b]].view(np.float32).copy() for b in range(B)]
    clean = all((bits[b, m[b]:] == NAN_BITS).all() for b in range(B))
    return outs, clean, bits
