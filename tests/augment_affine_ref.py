"""TEST INFRASTRUCTURE ONLY: an independent statement of miseg_augment_affine (include/miseg_hip.h) in numpy that the
CPU and the GPU tests share.  Coordinates are taken in float64 from the SAME float32 m and t the kernel gets, the noise hash is restated in
exact uint64 arithmetic, Box-Muller and gamma are float64.  Also here: the error bounds of DESIGN.md section 7.11, each from the roundings
of the fp32 chain it bounds."""
import numpy as np

U24 = 2.0 ** -24          # half an ulp of a float32 in [1, 2): the relative error of one rounding
ULP = 2.0 ** -23
TWO_PI_F = float(np.float32(6.28318530717958647692))
# documented accuracy of the device math library's accurate single-precision functions (the OpenCL full-profile bounds it is built to), in ulp
ULP_POW, ULP_LOG, ULP_COS, ULP_SQRT = 16.0, 3.0, 4.0, 3.0
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def identity_sample(origin, flip=(0, 0, 0), rot_k=0, m=None, t=(0, 0, 0), scale=0.0, shift=0.0, gamma=0.0, noise=(0.0, 0.0)):
    return dict(origin=list(origin), flip=list(flip), rot_k=int(rot_k), m=np.eye(3, dtype=np.float32) if m is None else np.asarray(m, dtype=np.float32).reshape(3, 3),
                t=np.asarray(t, dtype=np.float32), scale=float(np.float32(scale)), shift=float(np.float32(shift)), gamma=float(np.float32(gamma)),
                noise_mean=float(np.float32(noise[0])), noise_std=float(np.float32(noise[1])))


def pre_flip_coords(roi, flip, rot_k):
    """int64 [3, rd, rh, rw]: for every output voxel the coordinate inside the un-augmented crop (the chain crop -> flip 0, 1, 2 -> rot90^k in
    the (0, 1) plane, inverted back to front), found by pushing an index volume through the forward chain"""
    rd, rh, rw = roi
    idx = np.stack(np.meshgrid(np.arange(rd), np.arange(rh), np.arange(rw), indexing="ij"))
    for a in range(3):
        if flip[a]:
            idx = np.flip(idx, 1 + a)
    return np.ascontiguousarray(np.rot90(idx, rot_k & 3, (1, 2))).astype(np.int64)


def source_positions(roi, sample):
    """float64 [3, rd, rh, rw]: s = origin + c + M (q - c) + t in the resident volume, from the float32 m and t"""
    q = pre_flip_coords(roi, sample["flip"], sample["rot_k"]).astype(np.float64)
    c = (np.asarray(roi, dtype=np.float64) - 1.0) / 2.0
    d = q - c[:, None, None, None]
    m = np.asarray(sample["m"], dtype=np.float32).astype(np.float64).reshape(3, 3)
    t = np.asarray(sample["t"], dtype=np.float32).astype(np.float64)
    return np.einsum("ab,bdhw->adhw", m, d) + (t + np.asarray(sample["origin"], dtype=np.float64) + c)[:, None, None, None]


def coord_error_bound(roi, sample):
    """E_c: the fp32 coordinate chain d = q - c (exact), three products, two sums, + t, + (origin + c) (exact) makes 7 roundings, each at
    most 2^-24 of an intermediate, and no intermediate exceeds origin + c + sum_b |m_ab| c_b + |t_a| in magnitude"""
    c = (np.asarray(roi, dtype=np.float64) - 1.0) / 2.0
    m = np.abs(np.asarray(sample["m"], dtype=np.float64).reshape(3, 3))
    big = np.asarray(sample["origin"], dtype=np.float64) + c + m @ c + np.abs(np.asarray(sample["t"], dtype=np.float64))
    return 7.0 * U24 * float(big.max())


def _neighbours(image, s, padding):
    """the 8 neighbours of every position: float64 [C, 2, 2, 2, ...] (zeros mode: 0 outside the volume, border: clamped indices), and f [3, ...]"""
    C, D, H, W = image.shape
    fl = np.floor(s)
    f = s - fl
    i0 = fl.astype(np.int64)
    x = np.zeros((C, 2, 2, 2) + s.shape[1:], dtype=np.float64)
    img = image.astype(np.float64)
    for p in range(2):
        for q in range(2):
            for r in range(2):
                i, j, k = i0[0] + p, i0[1] + q, i0[2] + r
                inside = (i >= 0) & (i < D) & (j >= 0) & (j < H) & (k >= 0) & (k < W)
                v = img[:, np.clip(i, 0, D - 1), np.clip(j, 0, H - 1), np.clip(k, 0, W - 1)]
                x[:, p, q, r] = v if padding == "border" else np.where(inside[None], v, 0.0)
    return x, f


def resample_image64(image, s, padding="border"):
    """trilinear: seven lerps a + f (b - a), along W, then H, then D.  -> (float64 [C, ...], spread [C, ...], vmax [C, ...]): spread is the sum
    over the axes of the largest neighbour difference around the position, vmax the largest neighbour magnitude"""
    x, f = _neighbours(image, s, padding)
    y = x[:, :, :, 0] + f[2] * (x[:, :, :, 1] - x[:, :, :, 0])
    z = y[:, :, 0] + f[1] * (y[:, :, 1] - y[:, :, 0])
    v = z[:, 0] + f[0] * (z[:, 1] - z[:, 0])
    spread = (np.abs(x[:, 1] - x[:, 0]).max(axis=(1, 2)) + np.abs(x[:, :, 1] - x[:, :, 0]).max(axis=(1, 2)) +
              np.abs(x[:, :, :, 1] - x[:, :, :, 0]).max(axis=(1, 2)))
    return v, spread, np.abs(x).max(axis=(1, 2, 3))


def resample_label(label, s, padding="border"):
    """nearest: floor(s + 0.5) per axis (halves round up), the element copied; zeros mode: 0 outside the volume"""
    D, H, W = label.shape
    n = np.floor(s + 0.5).astype(np.int64)
    inside = (n[0] >= 0) & (n[0] < D) & (n[1] >= 0) & (n[1] < H) & (n[2] >= 0) & (n[2] < W)
    v = label[np.clip(n[0], 0, D - 1), np.clip(n[1], 0, H - 1), np.clip(n[2], 0, W - 1)]
    return v if padding == "border" else np.where(inside, v, np.zeros((), dtype=label.dtype)).astype(label.dtype)


def half_distance(s):
    """[...]: how far the position is from a nearest-neighbour tie, the smallest over the axes of |frac(s) - 1/2|"""
    return np.abs((s - np.floor(s)) - 0.5).min(axis=0)


def mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z ^ (z >> np.uint64(30))
        z = z * np.uint64(0xBF58476D1CE4E5B9)
        z = z ^ (z >> np.uint64(27))
        z = z * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def noise_uniforms(seed, draw, sample, count):
    """(u1 in (0, 1], u2 in [0, 1)) float64 [count], exact multiples of 2^-24: elements 0 .. count - 1 of sample `sample`"""
    with np.errstate(over="ignore"):
        key = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(draw & 0xFFFFFFFFFFFFFFFF) * np.uint64(0xC2B2AE3D27D4EB4F) + \
            np.uint64(0x165667B19E3779F9)
        ks = mix64(key ^ (np.uint64(sample) * np.uint64(0x9E3779B97F4A7C15)))
        h = mix64(ks + np.arange(count, dtype=np.uint64) * np.uint64(0xD1342543DE82EF95))
    u1 = ((h >> np.uint64(40)).astype(np.float64) + 1.0) * U24
    u2 = ((h >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64) * U24
    return u1, u2


def noise_z64(u1, u2):
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI_F * u2)


def noise_z_bound(u1):
    """|z_fp32 - z_64|: r = sqrtf(-2 logf(u1)) carries logf's ulps halved by the root plus sqrtf's own; the angle fl(2 pi u2) one rounding of a
    value below 2 pi, cosf its own ulps of a value of at most 1; the product one rounding more"""
    r = np.sqrt(-2.0 * np.log(u1))
    rel_r = (ULP_LOG / 2.0 + ULP_SQRT) * ULP
    return r * (rel_r + TWO_PI_F * U24 + ULP_COS * ULP + U24)


def gamma64(v, gamma):
    lo = v.min()
    rng = v.max() - lo
    return ((v - lo) / (rng + float(np.float32(1e-7)))) ** gamma * rng + lo, lo, rng


def gamma_bound(v, gamma, lo, rng):
    """|fp32 - float64| of v' = powf((v - lo) / (range + eps), gamma) * range + lo per element, for exact v: x = (v - lo) / den carries four
    roundings (v - lo, max - lo, + eps, the division: relative 4 * 2^-24), which the power multiplies by gamma; powf adds its documented
    ulps; `range` carries its one rounding, the product and the sum round once each"""
    x = (v - lo) / (rng + 1e-7)
    p = x ** gamma
    return p * rng * (4.0 * U24 * gamma + ULP_POW * ULP + 2.0 * U24) + U24 * np.abs(p * rng + lo)


def augment_affine_ref(image, label, roi, samples, padding="border", seed=0, draw=0):
    """image [C, D, H, W] float32, label [D, H, W]; samples: identity_sample dicts.  -> list of dicts per sample: image (float64 [C, roi]), label,
    s, resampled (before gamma), spread, vmax, after_gamma, lo, range, u1, u2 (None without noise)"""
    out = []
    C = image.shape[0]
    for i, sm in enumerate(samples):
        s = source_positions(roi, sm)
        v, spread, vmax = resample_image64(image, s, padding)
        r = dict(s=s, resampled=v, spread=spread, vmax=vmax, label=None if label is None else resample_label(label, s, padding), lo=None, range=None, u1=None, u2=None)
        if sm["gamma"] > 0:
            v, r["lo"], r["range"] = gamma64(v, sm["gamma"])
        r["after_gamma"] = v
        v = v * float(np.float32(1.0) + np.float32(sm["scale"])) + sm["shift"]          # the kernel's factor is the float32 fl(1 + scale)
        r["before_noise"] = v
        if sm["noise_std"] > 0:
            r["u1"], r["u2"] = (u.reshape(v.shape) for u in noise_uniforms(seed, draw, i, v.size))
            v = v + (sm["noise_mean"] + sm["noise_std"] * noise_z64(r["u1"], r["u2"]))
        r["image"] = v
        out.append(r)
    return out
