"""CPU tests of Gaussian smoothing / sharpening on the device augmenter (data/augment.py): the taps are MONAI's erf taps,
the numpy restatement the GPU tests hold the kernel to (tests/gaussian_filter_ref.py) agrees with a float64 zero-padded convolution, the seeded
parameter stream with the new options off is the one it always was, and the command-line flags are what the documents say.  No GPU work."""
import argparse

import numpy as np
import pytest
import torch

import gaussian_filter_ref as R

OLD_KEYS = ("origin", "flip", "rot_k", "scale", "shift", "centre", "affine", "gamma", "noise")
SIGMAS = (0.25, 0.5, 1.0, 1.5, 2.0)


def test_taps_are_the_erf_taps():
    from mi_seg_amd.data.augment import gaussian_taps
    for sigma, length in zip(SIGMAS, (3, 5, 9, 13, 17)):
        w = R.taps(sigma)
        assert w.dtype == np.float32 and len(w) == length and np.array_equal(w, w[::-1]) and np.all(w >= 0)
        total = float(w.astype(np.float64).sum())
        print(f"sigma {sigma}: {length} taps, float64 sum {total:.7f}")
        assert 0.9999 < total <= 1.0
        mine = gaussian_taps(sigma)
        assert mine.dtype == np.float32 and np.array_equal(mine.view(np.int32), w.view(np.int32))


def _conv3d_f64(x, sigmas):
    """float64 torch conv3d of [D, H, W] with the outer product of the float32 taps, zero padding"""
    w = [torch.from_numpy(R.taps(s).astype(np.float64)) if s else torch.ones(1, dtype=torch.float64) for s in sigmas]
    k = w[0][:, None, None] * w[1][None, :, None] * w[2][None, None, :]
    pad = tuple((len(v) - 1) // 2 for v in w)
    return torch.nn.functional.conv3d(torch.from_numpy(x.astype(np.float64))[None, None], k[None, None], padding=pad)[0, 0].numpy()


@pytest.mark.parametrize("shape,sigmas", [((13, 17, 37), (1.5, 0.25, 0.9)), ((3, 2, 5), (1.5, 1.5, 1.5)), ((20, 20, 20), (2.0, 2.0, 2.0))])
def test_restatement_agrees_with_a_float64_convolution(shape, sigmas):
    """three passes of non-negative taps whose sum is at most 1: each pass rounds taps + 1 products and sums of magnitude at most max|x|"""
    x = np.random.default_rng(sum(shape)).uniform(-1, 1, shape).astype(np.float32)
    got = R.smooth(x, sigmas)
    want = _conv3d_f64(x, sigmas)
    taps_max = max(len(R.taps(s)) for s in sigmas)
    bound = 3 * (taps_max + 1) * 2.0 ** -24 * float(np.abs(x).max())
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{shape} sigma {sigmas}: max err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.4f}")
    assert got.dtype == np.float32 and err <= bound


def test_impulse_constant_and_identity():
    sig = (1.5, 0.25, 0.9)
    wd, wh, ww = (R.taps(s) for s in sig)
    x = np.zeros((13, 17, 37), dtype=np.float32)
    x[6, 8, 18] = 1.0
    got = R.smooth(x, sig)
    # an impulse: one non-zero product a pass, so the response is fl(w_D * fl(w_H * w_W)) exactly
    want = (wd[:, None, None] * (wh[None, :, None] * ww[None, None, :]).astype(np.float32)).astype(np.float32)
    rd, rh, rw = (len(w) // 2 for w in (wd, wh, ww))
    assert np.array_equal(R.bits(got[6 - rd:7 + rd, 8 - rh:9 + rh, 18 - rw:19 + rw]), R.bits(want))
    assert np.count_nonzero(got) == np.count_nonzero(want) == want.size                  # and nothing outside that box
    # sigma == 0 on every axis returns the input, bit for bit; on one axis that axis is left alone
    y = np.random.default_rng(1).standard_normal((5, 6, 7)).astype(np.float32)
    y[1, 2, 3] = -0.0
    assert np.array_equal(R.bits(R.smooth(y, (0.0, 0.0, 0.0))), R.bits(y))
    assert np.array_equal(R.bits(R.smooth(y, (0.0, 1.0, 0.0))), R.bits(R.pass_1d(y, R.taps(1.0), -2)))
    # alpha == 0: sharpening returns the first blur
    assert np.array_equal(R.bits(R.sharpen(y, (1.0, 0.5, 0.7), (0.5, 0.5, 0.5), 0.0)), R.bits(R.smooth(y, (1.0, 0.5, 0.7))))


def test_binding_constants_are_the_headers():
    import os
    import re
    from conftest import ROOT
    from mi_seg_amd.hip import lib as L
    defs = dict(re.findall(r"#define (MISEG_GAUSS_\w+) (\d+)", open(os.path.join(ROOT, "include", "miseg_hip.h")).read()))
    assert L.GAUSS_MAX_RADIUS == int(defs["MISEG_GAUSS_MAX_RADIUS"]) == R.MAX_RADIUS
    assert L.GAUSS_TILE == tuple(int(defs["MISEG_GAUSS_TILE_" + a]) for a in "DHW")


def _resident(shape=(20, 18, 16), C=2, seed=0):
    from mi_seg_amd.data.augment import ResidentVolume
    g = torch.Generator().manual_seed(seed)
    return ResidentVolume(torch.rand((C,) + shape, generator=g), torch.randint(0, 5, shape, generator=g))


def test_seeded_stream_is_preserved_with_the_new_options_off():
    from mi_seg_amd.data.augment import GpuAugmenter
    vol = _resident()
    old = dict(patches_training_sample=6, randFlipd_prob=0.5, randRotate90d_prob=0.7, randScaleIntensityd_prob=0.5, randShiftIntensityd_prob=0.5, seed=11,
               randAffined_prob=0.5, rotate_range=(0.2, 0.2, 0.2), randAdjustContrastd_prob=0.5, randGaussianNoised_prob=0.5)
    base = GpuAugmenter((8, 8, 6), **old).draw(vol)              # built without the new arguments
    off = GpuAugmenter((8, 8, 6), **old, randGaussianSmoothd_prob=0.0, smooth_sigma_range=(0.5, 1.0), randGaussianSharpend_prob=0.0).draw(vol)
    for a, b in zip(base, off):
        assert set(a) == set(b) == set(OLD_KEYS) | {"smooth", "sharpen"}
        for k in OLD_KEYS:
            assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], k
        assert b["smooth"] is None and b["sharpen"] is None
    # with them on, no draw made before them within the same sample moves: the first sample's old keys are unchanged
    on = GpuAugmenter((8, 8, 6), **old, randGaussianSmoothd_prob=1.0, randGaussianSharpend_prob=1.0).draw(vol)
    for k in OLD_KEYS:
        assert np.array_equal(base[0][k], on[0][k]) if isinstance(base[0][k], np.ndarray) else base[0][k] == on[0][k], k
    for p in on:
        assert len(p["smooth"]) == 3 and all(0.25 <= s <= 1.5 for s in p["smooth"])
        s1, s2, alpha = p["sharpen"]
        assert len(s1) == 3 and all(0.5 <= s <= 1.0 for s in s1) and 10.0 <= alpha <= 30.0
        assert all(min(0.5, a) <= b <= max(0.5, a) for a, b in zip(s1, s2))              # MONAI's one-value rule for sigma2
    only = GpuAugmenter((8, 8, 6), **old, randGaussianSharpend_prob=1.0, sharpen_sigma1_range=(0.2, 0.3), sharpen_sigma2=0.8, sharpen_alpha_range=(2.0, 3.0)).draw(vol)
    for p in only:
        s1, s2, alpha = p["sharpen"]
        assert p["smooth"] is None and all(0.2 <= a <= 0.3 and a <= b <= 0.8 for a, b in zip(s1, s2)) and 2.0 <= alpha <= 3.0


def test_parser_and_validation():
    from mi_seg_amd.data.augment import GpuAugmenter, gaussian_taps
    from mi_seg_amd.utils.parser import add_data_argparse_args, add_model_argparse_args
    ap = add_data_argparse_args(add_model_argparse_args(argparse.ArgumentParser()))
    args = ap.parse_args([])
    assert (args.randGaussianSmoothd_prob, args.smooth_sigma_range, args.randGaussianSharpend_prob) == (0.0, [0.25, 1.5], 0.0)
    assert (args.sharpen_sigma1_range, args.sharpen_sigma2, args.sharpen_alpha_range) == ([0.5, 1.0], 0.5, [10.0, 30.0])
    d = GpuAugmenter.from_argparse_args(args, seed=3)
    assert (d.p_smooth, d.smooth_sigma_range, d.p_sharpen, d.sharpen_sigma1_range, d.sharpen_sigma2, d.sharpen_alpha_range) == \
        (0.0, (0.25, 1.5), 0.0, (0.5, 1.0), 0.5, (10.0, 30.0))
    a = ap.parse_args(["--randGaussianSmoothd_prob=0.2", "--smooth_sigma_range", "0.5", "1.0", "--randGaussianSharpend_prob=0.3", "--sharpen_sigma1_range", "0.4",
                       "0.9", "--sharpen_sigma2=0.7", "--sharpen_alpha_range", "5", "15"])
    g = GpuAugmenter.from_argparse_args(a)
    assert (g.p_smooth, g.smooth_sigma_range, g.p_sharpen, g.sharpen_sigma1_range, g.sharpen_sigma2, g.sharpen_alpha_range) == \
        (0.2, (0.5, 1.0), 0.3, (0.4, 0.9), 0.7, (5.0, 15.0))
    for bad in (dict(smooth_sigma_range=(1.0, 0.5)), dict(smooth_sigma_range=(-0.1, 0.5)), dict(smooth_sigma_range=(0.25, 2.2)),      # 2.2 * 4 -> radius 9
                dict(sharpen_sigma1_range=(0.5, 3.0)), dict(sharpen_sigma1_range=(0.5,)), dict(sharpen_sigma2=-1.0), dict(sharpen_sigma2=2.5),
                dict(sharpen_alpha_range=(3.0, 1.0))):
        with pytest.raises(ValueError):
            GpuAugmenter((8, 8, 8), **bad)
    GpuAugmenter((8, 8, 8), smooth_sigma_range=(0.0, 2.0))                                # radius 8 fits
    with pytest.raises(ValueError):
        gaussian_taps(2.2)
    with pytest.raises(ValueError):
        gaussian_taps(0.0)
