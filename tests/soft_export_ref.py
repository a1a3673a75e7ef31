"""numpy fp32 restatement of the soft prediction export (include/miseg_hip.h: miseg_soft_export), independent of the
package's own CPU path: the host tables of PredictionGeometry.lerp_tables, the softmax in channel order, the separable blend along logits W,
then H, then D with the t == 0 rule - every operation an explicit np.float32 operation in the stated order - the first-maximum argmax and the
uint8 quantisation.  blend() evaluates the whole output grid or a given list of output coordinates."""
import numpy as np

F = np.float32


def nearest_rule(n_in, n_out):
    """miseg_resample3d's nearest rule (floor(fma(dst + 0.5, in / out, -0.5) + 0.5) in fp32, clamped), one output at a time"""
    r = F(n_in) / F(n_out)
    out = []
    for d in range(n_out):
        t = F(float(F(d) + F(0.5)) * float(r) - 0.5)
        out.append(min(max(int(np.floor(t + F(0.5))), 0), n_in - 1))
    return np.array(out, dtype=np.int64)


def lerp_tables(geom, mode="trilinear"):
    """-> ([(lo, hi, t) per file axis X, Y, Z], axes), one file voxel at a time"""
    tables, axes = [None] * 3, [None] * 3
    for k, a in enumerate(geom.order):
        m, n, off = geom.resampled_shape[k], geom.ras_shape[k], geom.pad_before[k]
        near = nearest_rule(m, n) if mode == "nearest" else None
        lo, hi, t = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, F)
        for i in range(n):
            r = n - 1 - i if geom.flips[k] else i
            if mode == "nearest":
                lo[i] = hi[i] = near[r] + off
                continue
            scale = F(F(m) / F(n))
            f = F(F(F(F(r) + F(0.5)) * scale) - F(0.5))
            f = min(max(f, F(0)), F(m - 1))
            l = int(np.floor(f))
            lo[i], hi[i], t[i] = l + off, min(l + 1, m - 1) + off, F(f - F(l))
        tables[a], axes[a] = (lo, hi, t), k
    return tables, axes


def softmax(x):
    """e_c = exp(x_c - max_c x), p_c = e_c / sum_c e_c in fp32, the sum taken in channel order"""
    x = np.asarray(x, dtype=F)
    mx = x[0].copy()
    for c in range(1, x.shape[0]):
        up = x[c] > mx
        mx[up] = x[c][up]
    e = np.exp((x - mx[None]).astype(F)).astype(F)
    total = np.zeros_like(mx)
    for c in range(x.shape[0]):
        total = (total + e[c]).astype(F)
    return (e / total[None]).astype(F)


def _lerp(a, b, t):
    with np.errstate(invalid="ignore", over="ignore"):
        u = (F(1) - t).astype(F)
        v = ((a * u).astype(F) + (b * t).astype(F)).astype(F)
    return np.where(t == 0, a, v).astype(F)


def blend(scores, tables, axes, coords=None):
    """scores fp32 [C, D, H, W] -> the blended scores, [C, nz, ny, nx], or [C, N] at the output voxels coords = (x, y, z) index arrays"""
    scores = np.asarray(scores, dtype=F)
    if coords is None:
        n = [len(t[0]) for t in tables]
        coords = (np.arange(n[0]).reshape(1, 1, -1), np.arange(n[1]).reshape(1, -1, 1), np.arange(n[2]).reshape(-1, 1, 1))
    idx, tt = [None] * 3, [None] * 3           # per logits axis: (lo, hi) index arrays and the weight, broadcast over the outputs
    for a in range(3):
        lo, hi, t = (np.asarray(v) for v in tables[a])
        idx[axes[a]] = (lo[coords[a]].astype(np.int64), hi[coords[a]].astype(np.int64))
        tt[axes[a]] = t[coords[a]].astype(F)

    def at(bd, bh, bw):
        return scores[(slice(None),) + np.broadcast_arrays(idx[0][bd], idx[1][bh], idx[2][bw])]

    tD, tH, tW = (np.broadcast_to(t, np.broadcast_shapes(tt[0].shape, tt[1].shape, tt[2].shape))[None] for t in tt)
    c = [[_lerp(at(bd, bh, 0), at(bd, bh, 1), tW) for bh in (0, 1)] for bd in (0, 1)]
    return _lerp(_lerp(c[0][0], c[0][1], tH), _lerp(c[1][0], c[1][1], tH), tD)


def first_max(v):
    """strict `>` scan over axis 0: the first maximum wins, a NaN after channel 0 never does, a NaN in channel 0 gives 0"""
    arg = np.zeros(v.shape[1:], dtype=np.int64)
    mx = v[0].copy()
    with np.errstate(invalid="ignore"):
        for c in range(1, v.shape[0]):
            up = v[c] > mx
            mx[up] = v[c][up]
            arg[up] = c
    return arg


def labels(v, lut, nbytes=2):
    """lut[first_max(v)] truncated to nbytes, as an unsigned array of that width"""
    dt = {1: np.uint8, 2: np.uint16, 4: np.uint32}[nbytes]
    return (np.asarray(lut, dtype=np.int64)[first_max(v)] & ((1 << (8 * nbytes)) - 1)).astype(dt)


def quantize(p):
    """uint8 q = min(255, floor(p * 255 + 0.5)) in fp32; a NaN gives 0"""
    with np.errstate(invalid="ignore"):
        q = np.floor(((p * F(255)).astype(F) + F(0.5)).astype(F))
    return np.where(p == p, np.clip(q, 0, 255), 0).astype(np.uint8)


def top_two_margin(v):
    """largest minus second largest value over axis 0 (inf for one channel)"""
    if v.shape[0] < 2:
        return np.full(v.shape[1:], np.inf, dtype=F)
    s = np.sort(v, axis=0)
    return s[-1] - s[-2]


def softmax_tolerance(C):
    """per-element absolute bound of a device softmax + blend against this restatement, on values <= 1 where a rounding is at most 2^-24:
    the softmax takes C + 4 roundings (a subtraction, the exp, C - 1 additions, a division and the exp's own error of up to 3), counted 4
    times over because the two exp implementations differ by more than a rounding; the blend adds 9 roundings that both sides share in
    order, counted once.  4.8e-6 at C = 14 (the narrower of the two readings of "4 x ((C + 4) + 9) roundings")."""
    return (4.0 * (C + 4) + 9.0) * 2.0 ** -24
