"""TEST INFRASTRUCTURE ONLY: an independent statement of miseg_gaussian_filter3d (include/miseg_hip.h) in numpy that the
CPU and the GPU tests share: MONAI's erf taps, the three zero-padded 1-D passes W, H, D, smoothing and sharpening.  A pass is vectorised over
the elements and sequential over the taps, and every product and every sum is cast to float32, so it carries the kernel's bits."""
import math

import numpy as np

MAX_RADIUS = 8
F = np.float32


def radius(sigma, truncated=4.0):
    return int(max(float(sigma) * truncated, 0.5) + 0.5)


def taps(sigma, truncated=4.0):
    """float32 [2 r + 1]: w[k] = max(0.5 (erf(t (k + 0.5)) - erf(t (k - 0.5))), 0), t = 0.70710678 / |sigma|, in float64, rounded once"""
    r = radius(sigma, truncated)
    t = 0.70710678 / abs(float(sigma))
    w = [max(0.5 * (math.erf(t * (k + 0.5)) - math.erf(t * (k - 0.5))), 0.0) for k in range(-r, r + 1)]
    return np.asarray(w, dtype=np.float64).astype(F)


def pass_1d(v, w, axis):
    """acc = 0; acc = fl(acc + fl(w[k] * v[x + k])) for k = -r..r along `axis`, zeros outside"""
    v = np.asarray(v, dtype=F)
    r = (len(w) - 1) // 2
    n = v.shape[axis]
    pad = [(0, 0)] * v.ndim
    pad[axis] = (r, r)
    p = np.pad(v, pad)
    acc = np.zeros(v.shape, dtype=F)
    for k in range(-r, r + 1):
        sl = [slice(None)] * v.ndim
        sl[axis] = slice(r + k, r + k + n)
        prod = (F(w[k + r]) * p[tuple(sl)]).astype(F)
        acc = (acc + prod).astype(F)
    return acc


def smooth(x, sigmas):
    """G(sigma)(x) over the last three axes of x (sigmas = (D, H, W)); an axis with sigma == 0 is skipped"""
    out = np.array(x, dtype=F, copy=True)
    for axis, sg in ((-1, sigmas[2]), (-2, sigmas[1]), (-3, sigmas[0])):
        if float(sg) != 0.0:
            out = pass_1d(out, taps(sg), axis)
    return out


def sharpen(x, sigma1, sigma2, alpha):
    """b1 = G(sigma1)(x), b2 = G(sigma2)(b1), out = fl(b1 + fl(alpha * fl(b1 - b2)))"""
    b1 = smooth(x, sigma1)
    b2 = smooth(b1, sigma2)
    diff = (b1 - b2).astype(F)
    scaled = (F(alpha) * diff).astype(F)
    return (b1 + scaled).astype(F)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)
