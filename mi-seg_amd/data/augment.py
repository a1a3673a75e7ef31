"""GPU-resident training augmentation: the random tail of the reference's MONAI chain (data/multi_modal.py:50-65) on volumes that stay
in HBM (the deterministic head -- load, orient, resample, ScaleIntensity, SpatialPad -- is what the reference's CacheDataset caches).

    RandCropByPosNegLabeld(pos=1, neg=1, num_samples=patches_training_sample, image_threshold=0)
    RandFlipd x 3 (axes 0, 1, 2, prob randFlipd_prob each), RandRotate90d(prob, max_k=3, axes (0, 1))
    RandScaleIntensityd(factors=0.1, prob), RandShiftIntensityd(offsets=0.1, prob)

The host draws the per-patch parameters (a torch.Generator: reproducible, rank-seedable) and ONE gather kernel per batch
(csrc/training.hip::augment_kernel) writes image and label patches - no intermediate crops, no per-transform passes.  MONAI's own random
stream cannot be reproduced (its RNG consumption order is an implementation detail of a dependency that is not vendored): the
DISTRIBUTIONS are restated, parity unpinned.

Beyond the reference's chain, all off by default (csrc/augment.hip::miseg_augment_affine, DESIGN.md section 7.11 - still one gather per batch):

    RandAffined(prob, rotate_range, scale_range, translate_range, padding_mode)      small free rotations / zooms about the crop centre
    RandAdjustContrastd(prob, gamma)                                                   v' = ((v - min) / (max - min + 1e-7))^gamma (max - min) + min
    RandGaussianNoised(prob, mean, std)                                                std drawn U(0, noise_std) per sample

Behind the gather, on the image only and off by default as well (csrc/gaussian.hip::miseg_gaussian_filter3d): a separable
Gaussian filter with MONAI's erf taps and zero padding at the patch faces, one launch per filter application over the whole batch

    RandGaussianSmoothd(prob, sigma_x, sigma_y, sigma_z)                               out = G(sigma)(x), one sigma per axis drawn U(smooth_sigma_range)
    RandGaussianSharpend(prob, sigma1, sigma2, alpha)                                  b1 = G(sigma1)(x); out = b1 + alpha (b1 - G(sigma2)(b1))"""
import ctypes as C
import math

import numpy as np
import torch

from ..hip import lib as L
from ..hip import ops


class ResidentVolume:
    """one cached sample: image fp32 [C, D, H, W] and label [D, H, W] on the device + its foreground / background voxel lists
    (MONAI map_binary_to_indices: fg = label > 0, bg = label == 0 & image > image_threshold)"""

    def __init__(self, image, label, modality=0, image_threshold=0.0):
        if image.dim() != 4 or label.shape != image.shape[1:]:
            raise ValueError("image [C, D, H, W] and label [D, H, W] expected")
        self.image = image.float().contiguous()
        self.label = label.contiguous()
        self.modality = int(modality)
        flat = self.label.reshape(-1)
        self.fg = torch.nonzero(flat > 0).reshape(-1)
        self.bg = torch.nonzero((flat == 0) & (self.image.amax(0).reshape(-1) > image_threshold)).reshape(-1)


def affine_matrix(rotate=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0)):
    """float32 [3, 3] sampling matrix M = Rz . Ry . Rx . diag(scale): it maps an OUTPUT offset from the crop centre to the INPUT offset that
    is read there (a sampling grid, as MONAI's RandAffine builds one - so scale > 1 reads a wider region: the content shrinks).  Axes are the
    patch axes (0, 1, 2) = (D, H, W); rotate[a] is the angle about axis a, in radians, with

        Rx(r) = [[1, 0, 0], [0, c, -s], [0, s, c]]     Ry(r) = [[c, 0, s], [0, 1, 0], [-s, 0, c]]     Rz(r) = [[c, -s, 0], [s, c, 0], [0, 0, 1]]

    (c, s = cos r, sin r: MONAI's create_rotate forms).  Sign convention: rotate = (0, 0, -pi / 2) samples like torch.rot90(x, 1, (0, 1)) -
    RandRotate90d's rot_k = 1 - and (0, 0, +pi / 2) like rot_k = 3.  Composed in float64; entries of the rotation product within 1e-7 of 0 or
    +-1 are snapped to them before the scaling, so that quarter turns are exact gathers (the kernel's integer path needs the exact identity,
    tests/test_hip_augment_affine.py the exact quarter turn); a drawn angle is moved by less than 1e-7 of a voxel per voxel of offset."""
    rx, ry, rz = (float(r) for r in rotate)
    c, s = math.cos(rx), math.sin(rx)
    Rx = np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=np.float64)
    c, s = math.cos(ry), math.sin(ry)
    Ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=np.float64)
    c, s = math.cos(rz), math.sin(rz)
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float64)
    R = Rz @ Ry @ Rx
    for v in (0.0, 1.0, -1.0):
        R[np.abs(R - v) < 1e-7] = v
    return (R @ np.diag(np.asarray(scale, dtype=np.float64))).astype(np.float32)


def _triple(v, name):
    t = (float(v),) * 3 if isinstance(v, (int, float)) else tuple(float(x) for x in v)
    if len(t) == 1:
        t = t * 3
    if len(t) != 3:
        raise ValueError(f"{name}: one value or one per axis expected, got {v!r}")
    return t


def gaussian_radius(sigma, truncated=4.0):
    """the taps of sigma reach from -r to r: r = int(max(sigma * truncated, 0.5) + 0.5) (MONAI gaussian_1d); sigma == 0: 0, the axis is skipped"""
    sigma = float(sigma)
    if not math.isfinite(sigma):
        raise ValueError(f"sigma {sigma!r} is not finite")
    return 0 if sigma == 0.0 else int(max(sigma * truncated, 0.5) + 0.5)


def gaussian_taps(sigma, truncated=4.0):
    """float32 [2 r + 1]: MONAI gaussian_1d(sigma, truncated, approx="erf") - w[k] = max(0.5 (erf(t (k + 0.5)) - erf(t (k - 0.5))), 0) with
    t = 0.70710678 / |sigma|, k = -r..r, not normalised - in float64, rounded once.  ValueError: sigma == 0 (no taps: the axis is skipped) or a
    radius above MISEG_GAUSS_MAX_RADIUS."""
    r = gaussian_radius(sigma, truncated)
    if r == 0:
        raise ValueError("sigma == 0 has no taps (a filter skips that axis)")
    if r > L.GAUSS_MAX_RADIUS:
        raise ValueError(f"sigma {sigma!r} needs a radius of {r}: the kernel's maximum is {L.GAUSS_MAX_RADIUS}")
    t = 0.70710678 / abs(float(sigma))
    return np.array([max(0.5 * (math.erf(t * (k + 0.5)) - math.erf(t * (k - 0.5))), 0.0) for k in range(-r, r + 1)], dtype=np.float64).astype(np.float32)


def gaussian_sample(sigmas=(0.0, 0.0, 0.0), alpha=0.0, sharpen=False):
    """the miseg_gaussian_filter_sample of one filter application: sigmas per axis (D, H, W), 0 = the axis is skipped; the default copies"""
    q = L.GaussSample()
    for a, sg in enumerate(_triple(sigmas, "sigmas")):
        q.radius[a] = gaussian_radius(sg)
        if q.radius[a]:
            for k, w in enumerate(gaussian_taps(sg).tolist()):
                q.taps[a][k] = w
    q.alpha, q.sharpen = float(alpha), int(bool(sharpen))
    return q


def _gaussian_call(src, dst, descs):
    """miseg_gaussian_filter3d over [n, C, D, H, W] with one descriptor per sample, MISEG_AUG_MAX_SAMPLES samples a launch"""
    n, Cc, D, H, W = src.shape
    for i0 in range(0, n, L.AUG_MAX_SAMPLES):
        m = min(L.AUG_MAX_SAMPLES, n - i0)
        arr = (L.GaussSample * m)(*descs[i0:i0 + m])
        q = L.GaussianFilter(C.sizeof(L.GaussianFilter), src[i0:].data_ptr(), dst[i0:].data_ptr(), m, Cc, D, H, W, C.cast(arr, C.c_void_p))
        ops._call("miseg_gaussian_filter3d", q)


def _gaussian_args(x, out, what):
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 5 and x.is_contiguous()):
        raise ValueError(f"{what}: a contiguous float32 device tensor [n, C, D, H, W] expected")
    if out is None:
        return torch.empty_like(x)
    if not (out.is_cuda and out.dtype == torch.float32 and out.shape == x.shape and out.is_contiguous() and out.device == x.device):
        raise ValueError(f"{what}: out has to be a contiguous float32 tensor of x's shape on x's device")
    return out


def _per_sample(sigmas, n, name):
    """one triple for every sample, or one triple per sample -> n triples"""
    rows = np.asarray(sigmas, dtype=np.float64)
    if rows.ndim == 2:
        if rows.shape != (n, 3):
            raise ValueError(f"{name}: one triple per sample expected, got shape {rows.shape} for {n} samples")
        return [tuple(r) for r in rows.tolist()]
    return [_triple(sigmas, name)] * n


def gaussian_filter(x, sigmas, out=None):
    """G(sigma)(x): x fp32 [n, C, D, H, W] on the device, sigmas = one (D, H, W) triple (or one value) or one triple per sample; 0 skips an axis.
    One miseg_gaussian_filter3d call, taps as gaussian_taps gives them, zeros outside the volume.  out: another tensor of x's shape."""
    out = _gaussian_args(x, out, "gaussian_filter")
    _gaussian_call(x, out, [gaussian_sample(sg) for sg in _per_sample(sigmas, x.shape[0], "sigmas")])
    return out


def gaussian_sharpen(x, sigma1, sigma2, alpha, out=None):
    """b1 = G(sigma1)(x); out = b1 + alpha (b1 - G(sigma2)(b1)) (MONAI GaussianSharpen): two calls, the second with the sharpen epilogue.
    sigma1, sigma2 as gaussian_filter's sigmas; alpha: one value or one per sample."""
    out = _gaussian_args(x, out, "gaussian_sharpen")
    n = x.shape[0]
    alphas = [float(alpha)] * n if isinstance(alpha, (int, float)) else [float(v) for v in alpha]
    if len(alphas) != n:
        raise ValueError(f"alpha: one value or one per sample expected, got {len(alphas)} for {n} samples")
    b1 = torch.empty_like(x)
    _gaussian_call(x, b1, [gaussian_sample(sg) for sg in _per_sample(sigma1, n, "sigma1")])
    _gaussian_call(b1, out, [gaussian_sample(sg, al, True) for sg, al in zip(_per_sample(sigma2, n, "sigma2"), alphas)])
    return out


def _sigma_range(v, name):
    """(low, high) of a sigma drawn U(low, high): 0 <= low <= high, and the taps of `high` fit the kernel's radius"""
    t = tuple(float(x) for x in v) if not isinstance(v, (int, float)) else ()
    if len(t) != 2 or not (math.isfinite(t[0]) and math.isfinite(t[1]) and 0.0 <= t[0] <= t[1]):
        raise ValueError(f"{name}: 0 <= low <= high expected, got {v!r}")
    if gaussian_radius(t[1]) > L.GAUSS_MAX_RADIUS:
        raise ValueError(f"{name}: sigma {t[1]} needs a radius of {gaussian_radius(t[1])}, the kernel's maximum is {L.GAUSS_MAX_RADIUS}")
    return t


class GpuAugmenter:
    def __init__(self, roi, patches_training_sample=1, randFlipd_prob=0.2, randRotate90d_prob=0.2, randScaleIntensityd_prob=0.1,
                 randShiftIntensityd_prob=0.1, pos=1.0, neg=1.0, seed=0, randAffined_prob=0.0, rotate_range=(0, 0, 0), scale_range=(0, 0, 0),
                 translate_range=(0, 0, 0), affine_padding_mode="border", randAdjustContrastd_prob=0.0, gamma_range=(0.5, 4.5),
                 randGaussianNoised_prob=0.0, noise_mean=0.0, noise_std=0.1, randGaussianSmoothd_prob=0.0, smooth_sigma_range=(0.25, 1.5),
                 randGaussianSharpend_prob=0.0, sharpen_sigma1_range=(0.5, 1.0), sharpen_sigma2=0.5, sharpen_alpha_range=(10.0, 30.0)):
        """rotate_range: radians per axis, drawn U(-r, r); scale_range: factor 1 + U(-s, s) per axis; translate_range: voxels, U(-t, t);
        affine_padding_mode: "border" | "zeros" for positions outside the VOLUME (the resample reads the resident volume, not the crop);
        gamma_range: (low, high) of U(low, high); noise_std: the std of a sample is drawn U(0, noise_std) (MONAI's rule);
        smooth_sigma_range, sharpen_sigma1_range: (low, high) of the per-axis sigma; sharpen_sigma2: one value s2, the second sigma of an axis
        is drawn U(min(s2, sigma1), max(s2, sigma1)) (MONAI's rule for a single value); sharpen_alpha_range: (low, high) of alpha"""
        self.roi = (roi,) * 3 if isinstance(roi, int) else tuple(roi)
        self.n = int(patches_training_sample)
        if not 1 <= self.n <= L.AUG_MAX_SAMPLES:
            raise ValueError(f"patches_training_sample must be in 1..{L.AUG_MAX_SAMPLES}")
        self.p_flip, self.p_rot, self.p_scale, self.p_shift = randFlipd_prob, randRotate90d_prob, randScaleIntensityd_prob, randShiftIntensityd_prob
        self.pos_ratio = pos / (pos + neg)
        self.seed = int(seed)
        self.gen = torch.Generator().manual_seed(seed)
        self.p_affine, self.p_gamma, self.p_noise = float(randAffined_prob), float(randAdjustContrastd_prob), float(randGaussianNoised_prob)
        self.rotate_range, self.scale_range = _triple(rotate_range, "rotate_range"), _triple(scale_range, "scale_range")
        self.translate_range = _triple(translate_range, "translate_range")
        if affine_padding_mode not in L.AUG_PAD_MODES:
            raise ValueError(f"affine_padding_mode {affine_padding_mode!r} is not one of {tuple(L.AUG_PAD_MODES)}")
        self.padding_mode = affine_padding_mode
        self.gamma_range = tuple(float(g) for g in gamma_range)
        if len(self.gamma_range) != 2 or not 0.0 < self.gamma_range[0] <= self.gamma_range[1]:
            raise ValueError(f"gamma_range: 0 < low <= high expected, got {gamma_range!r}")
        self.noise_mean, self.noise_std = float(noise_mean), float(noise_std)
        self.draws = 0                 # calls that went through miseg_augment_affine so far: the `draw` half of the noise key
        self._minmax = None            # the gamma scratch (zero before its first use; every call hands it back zeroed)
        self.p_smooth, self.p_sharpen = float(randGaussianSmoothd_prob), float(randGaussianSharpend_prob)
        self.smooth_sigma_range = _sigma_range(smooth_sigma_range, "smooth_sigma_range")
        self.sharpen_sigma1_range = _sigma_range(sharpen_sigma1_range, "sharpen_sigma1_range")
        if not isinstance(sharpen_sigma2, (int, float)):
            raise ValueError(f"sharpen_sigma2: one value expected, got {sharpen_sigma2!r}")
        self.sharpen_sigma2 = _sigma_range((sharpen_sigma2, sharpen_sigma2), "sharpen_sigma2")[0]
        self.sharpen_alpha_range = tuple(float(v) for v in sharpen_alpha_range)
        if len(self.sharpen_alpha_range) != 2 or not (all(math.isfinite(v) for v in self.sharpen_alpha_range) and self.sharpen_alpha_range[0] <= self.sharpen_alpha_range[1]):
            raise ValueError(f"sharpen_alpha_range: finite low <= high expected, got {sharpen_alpha_range!r}")
        self._blur = None              # the filters' second batch buffer, kept across calls

    @classmethod
    def from_argparse_args(cls, args, seed=0):
        """the augmenter of a parsed command line (utils/parser.py::DATA_ARGS + the roi of MODEL_ARGS)"""
        return cls((args.roi_x, args.roi_y, args.roi_z), patches_training_sample=args.patches_training_sample, randFlipd_prob=args.randFlipd_prob,
                   randRotate90d_prob=args.randRotate90d_prob, randScaleIntensityd_prob=args.randScaleIntensityd_prob,
                   randShiftIntensityd_prob=args.randShiftIntensityd_prob, seed=seed, randAffined_prob=args.randAffined_prob,
                   rotate_range=args.rotate_range, scale_range=args.scale_range, translate_range=args.translate_range,
                   affine_padding_mode=args.affine_padding_mode, randAdjustContrastd_prob=args.randAdjustContrastd_prob, gamma_range=args.gamma_range,
                   randGaussianNoised_prob=args.randGaussianNoised_prob, noise_std=args.noise_std,
                   randGaussianSmoothd_prob=args.randGaussianSmoothd_prob, smooth_sigma_range=args.smooth_sigma_range,
                   randGaussianSharpend_prob=args.randGaussianSharpend_prob, sharpen_sigma1_range=args.sharpen_sigma1_range,
                   sharpen_sigma2=args.sharpen_sigma2, sharpen_alpha_range=args.sharpen_alpha_range)

    def _u(self):
        return float(torch.rand((), generator=self.gen))

    def _sym(self, r):
        return (self._u() * 2.0 - 1.0) * r

    def _between(self, lo, hi):
        return lo + self._u() * (hi - lo)

    def draw(self, vol: ResidentVolume):
        """per-patch parameters (host side): list of dicts origin / flip / rot_k / scale / shift (+ centre: the voxel the crop was drawn around,
        before the crop was moved inside the volume - what the pos / neg balance is about) + affine (float32 [3, 4] = [M | t], affine_matrix's
        convention, or None) / gamma (float or None) / noise ((mean, std) or None) / smooth (the sigma triple (D, H, W) or None) / sharpen
        ((sigma1 triple, sigma2 triple, alpha) or None).  A transform whose probability is 0 consumes no random number, and the later ones draw
        after the sample's existing draws: with them off the parameter stream is the one it always was."""
        D, H, W = vol.label.shape
        out = []
        for _ in range(self.n):
            use_fg = (self._u() < self.pos_ratio and vol.fg.numel() > 0) or vol.bg.numel() == 0
            idx = vol.fg if (use_fg and vol.fg.numel() > 0) else vol.bg
            if idx.numel() == 0:
                centre = (D // 2, H // 2, W // 2)
            else:
                flat = int(idx[int(torch.randint(0, idx.numel(), (), generator=self.gen))])
                centre = (flat // (H * W), (flat // W) % H, flat % W)
            # MONAI correct_crop_centers: the crop stays inside the volume
            origin = [min(max(c - r // 2, 0), s - r) for c, r, s in zip(centre, self.roi, (D, H, W))]
            flip = [int(self._u() < self.p_flip) for _ in range(3)]
            rot_k = int(torch.randint(1, 4, (), generator=self.gen)) if self._u() < self.p_rot else 0
            scale = (self._u() * 0.2 - 0.1) if self._u() < self.p_scale else 0.0
            shift = (self._u() * 0.2 - 0.1) if self._u() < self.p_shift else 0.0
            affine = gamma = noise = None
            if self.p_affine > 0 and self._u() < self.p_affine:
                rot = [self._sym(r) for r in self.rotate_range]
                zoom = [1.0 + self._sym(s) for s in self.scale_range]
                t = [self._sym(t) for t in self.translate_range]
                affine = np.concatenate([affine_matrix(rot, zoom), np.asarray(t, dtype=np.float32)[:, None]], axis=1)
            if self.p_gamma > 0 and self._u() < self.p_gamma:
                gamma = self.gamma_range[0] + self._u() * (self.gamma_range[1] - self.gamma_range[0])
            if self.p_noise > 0 and self._u() < self.p_noise:
                noise = (self.noise_mean, self._u() * self.noise_std)
            smooth = sharpen = None
            if self.p_smooth > 0 and self._u() < self.p_smooth:
                smooth = tuple(self._between(*self.smooth_sigma_range) for _ in range(3))
            if self.p_sharpen > 0 and self._u() < self.p_sharpen:
                s1 = tuple(self._between(*self.sharpen_sigma1_range) for _ in range(3))
                s2 = tuple(self._between(min(self.sharpen_sigma2, v), max(self.sharpen_sigma2, v)) for v in s1)
                sharpen = (s1, s2, self._between(*self.sharpen_alpha_range))
            out.append(dict(origin=origin, flip=flip, rot_k=rot_k, scale=scale, shift=shift, centre=centre, affine=affine, gamma=gamma, noise=noise,
                            smooth=smooth, sharpen=sharpen))
        return out

    def __call__(self, vol: ResidentVolume, params=None):
        """-> batch dict like the reference's collated loader output: image [n, C, r, r, r] fp32, label [n, 1, r, r, r], modality [n].
        params: dicts as draw() returns them; the keys affine / gamma / noise / smooth / sharpen may be absent.  A batch in which no sample has
        one of the first three is miseg_augment_crop's, as it always was; any other goes through miseg_augment_affine (one launch, two when a
        sample has gamma).  A batch in which a sample has smooth or sharpen is filtered behind the gather (_filters); any other is not touched."""
        params = params if params is not None else self.draw(vol)
        if any(s < r for s, r in zip(vol.label.shape, self.roi)):
            raise ValueError("volume smaller than the roi: pad it first (SpatialPadd is part of the cached, deterministic head)")
        n, Cc = len(params), vol.image.shape[0]
        passes = self._filter_passes(params)
        ret = img = torch.empty((n, Cc) + self.roi, dtype=torch.float32, device=vol.image.device)
        if passes:
            if self._blur is None or self._blur.shape != img.shape or self._blur.device != img.device:
                self._blur = torch.empty_like(img)
            if len(passes) & 1:            # every pass changes sides: an odd number of them starts in the kept buffer and ends in the returned one
                img = self._blur
        lab = torch.empty((n, 1) + self.roi, dtype=vol.label.dtype, device=vol.image.device)
        D, H, W = vol.label.shape
        batch = {"image": ret, "label": lab, "modality": torch.full((n,), vol.modality, dtype=torch.int64)}
        if not any(p.get("affine") is not None or p.get("gamma") is not None or p.get("noise") is not None for p in params):
            samples = (L.AugSample * n)()
            for i, p in enumerate(params):
                samples[i] = L.AugSample((C.c_int * 3)(*p["origin"]), (C.c_int * 3)(*p["flip"]), p["rot_k"], p["scale"], p["shift"])
            q = L.Augment(C.sizeof(L.Augment), vol.image.data_ptr(), vol.label.data_ptr(), vol.label.element_size(), Cc, D, H, W, self.roi[0], self.roi[1],
                          self.roi[2], n, img.data_ptr(), lab.data_ptr(), C.cast(samples, C.c_void_p))
            ops._call("miseg_augment_crop", q)
            self._filters(passes, img, ret)
            return batch
        if self._minmax is None or self._minmax.device != vol.image.device:
            self._minmax = torch.zeros(L.AUG_AFFINE_SCRATCH_BYTES // 4, dtype=torch.int32, device=vol.image.device)
        augment_affine(vol.image, vol.label, self.roi, params, padding_mode=self.padding_mode, seed=self.seed, draw=self.draws, minmax=self._minmax,
                       out_image=img, out_label=lab)
        self.draws += 1
        self._filters(passes, img, ret)
        return batch

    @staticmethod
    def _filter_passes(params):
        """the filter applications behind the gather, each a list of one descriptor per sample: smooth when a sample has it, then sharpen's two
        when a sample has that; a sample that takes no part in a pass is copied by it.  A batch with neither: no pass"""
        smooth, sharpen = [p.get("smooth") for p in params], [p.get("sharpen") for p in params]
        passes = []
        if any(s is not None for s in smooth):
            passes.append([gaussian_sample() if s is None else gaussian_sample(s) for s in smooth])
        if any(s is not None for s in sharpen):
            passes.append([gaussian_sample() if s is None else gaussian_sample(s[0]) for s in sharpen])
            passes.append([gaussian_sample() if s is None else gaussian_sample(s[1], s[2], True) for s in sharpen])
        return passes

    def _filters(self, passes, src, ret):
        """run the passes from `src` (where the gather wrote), alternating between the kept buffer and the returned tensor: the last one writes `ret`"""
        for descs in passes:
            dst = ret if src is self._blur else self._blur
            _gaussian_call(src, dst, descs)
            src = dst
        assert src is ret


def augment_affine(image, label, roi, samples, padding_mode="border", seed=0, draw=0, minmax=None, out_image=None, out_label=None):
    """One miseg_augment_affine call (csrc/augment.hip): image fp32 [C, D, H, W] and label [D, H, W] (1, 4 or 8 byte elements) on the device,
    samples: dicts (affine_sample) -> (image fp32 [n, C, roi], label [n, 1, roi]).  minmax: the int32 [64] gamma scratch, zero before its
    first use (the call hands it back zeroed); needed when a sample has gamma.  The noise of sample i is a function of (seed, draw, i)."""
    n, Cc = len(samples), image.shape[0]
    roi = tuple(roi)
    if not (image.is_cuda and image.dtype == torch.float32 and image.is_contiguous() and label.is_contiguous() and label.device == image.device):
        raise ValueError("augment_affine: contiguous device tensors expected, the image in float32")
    if out_image is None:
        out_image = torch.empty((n, Cc) + roi, dtype=torch.float32, device=image.device)
    if out_label is None:
        out_label = torch.empty((n, 1) + roi, dtype=label.dtype, device=image.device)
    arr = (L.AugAffineSample * max(n, 1))()
    for i, p in enumerate(samples):
        arr[i] = affine_sample(p)
    D, H, W = label.shape
    q = L.AugmentAffine(C.sizeof(L.AugmentAffine), image.data_ptr(), label.data_ptr(), label.element_size(), Cc, D, H, W, roi[0], roi[1], roi[2], n,
                        out_image.data_ptr(), out_label.data_ptr(), C.cast(arr, C.c_void_p), L.AUG_PAD_MODES[padding_mode], int(seed) & (2 ** 64 - 1),
                        int(draw) & (2 ** 64 - 1), None if minmax is None else minmax.data_ptr())
    ops._call("miseg_augment_affine", q)
    return out_image, out_label


def affine_sample(p):
    """a sample dict -> the miseg_aug_affine_sample of the C ABI.  The matrix is `affine` (float32 [3, 4] = [M | t], draw()'s key) or `m` [3, 3]
    and `t` [3]; absent / None: the exact identity.  `gamma`: a float, absent / None / <= 0 = off.  The noise is `noise` = (mean, std) or
    `noise_mean` / `noise_std`; absent / None / std <= 0 = off."""
    a = p.get("affine")
    if a is None and p.get("m") is not None:
        a = np.concatenate([np.asarray(p["m"], dtype=np.float32).reshape(3, 3), np.asarray(p.get("t", (0, 0, 0)), dtype=np.float32).reshape(3, 1)], axis=1)
    a = np.concatenate([np.eye(3, dtype=np.float32), np.zeros((3, 1), dtype=np.float32)], axis=1) if a is None else np.asarray(a, dtype=np.float32)
    if a.shape != (3, 4):
        raise ValueError("affine: a [3, 4] matrix [M | t] expected")
    gamma, noise = p.get("gamma"), p.get("noise")
    mean, std = noise if noise is not None else (p.get("noise_mean", 0.0), p.get("noise_std", 0.0))
    return L.AugAffineSample((C.c_int * 3)(*p["origin"]), (C.c_int * 3)(*p["flip"]), p["rot_k"], (C.c_float * 9)(*a[:, :3].reshape(-1).tolist()),
                             (C.c_float * 3)(*a[:, 3].tolist()), p["scale"], p["shift"], 0.0 if gamma is None else gamma, mean, std)
