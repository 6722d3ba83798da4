"""Host half of the Pillow-exact bilinear resize (csrc/resize.hip): the per-output-pixel windows and fixed-point weights of Pillow's
``ImagingResample`` for 8-bit images (Resample.c: precompute_coeffs + normalize_coeffs_8bpc, 12.2.0).  They depend only on (input size,
output size); CPython floats are the C doubles Pillow uses and the order of operations is Pillow's, so the integer tables are the ones
Pillow builds.  ``apply_tables`` is the two integer passes in numpy: what the kernel does, for CPU tests and tools."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2


def _triangle(x):
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


def resize_tables(in_size, out_size):
    """(bounds int32 [out, 2] = first source index and tap count, coefs int32 [out, ksize], ksize) of Image.resize(BILINEAR) along one axis."""
    in_size, out_size = int(in_size), int(out_size)
    assert in_size > 0 and out_size > 0
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 1.0 * filterscale                      # the triangle filter's support, widened when shrinking (antialias)
    ksize = int(math.ceil(support)) * 2 + 1
    bounds, coefs = np.zeros((out_size, 2), dtype=np.int32), np.zeros((out_size, ksize), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        ww, w = 0.0, []
        for x in range(xmax):
            w.append(_triangle((x + xmin - center + 0.5) * ss))
            ww += w[-1]
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            coefs[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, coefs, ksize


def _pass(a, bounds, coefs, axis):
    a = np.moveaxis(a.astype(np.int64), axis, 0)
    out = np.empty((len(bounds),) + a.shape[1:], dtype=np.uint8)
    for s, (lo, n) in enumerate(bounds):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(coefs[s, :n].astype(np.int64), a[lo:lo + n], axes=1)
        out[s] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def apply_tables(img_u8, out_size):
    """uint8 [..., H0, H0, 3] -> [..., S, S, 3]: horizontal pass into a uint8 intermediate, then the vertical pass (numpy, integer)."""
    img_u8 = np.asarray(img_u8)
    H0 = img_u8.shape[-3]
    assert img_u8.dtype == np.uint8 and img_u8.shape[-2] == H0
    if H0 == out_size:
        return img_u8.copy()
    bounds, coefs, _ = resize_tables(H0, out_size)
    return _pass(_pass(img_u8, bounds, coefs, img_u8.ndim - 2), bounds, coefs, img_u8.ndim - 3)
