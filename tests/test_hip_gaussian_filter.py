"""GPU tests of the separable Gaussian filter (csrc/gaussian.hip::miseg_gaussian_filter3d, data/augment.py) against the
numpy restatement of tests/gaussian_filter_ref.py.  The arithmetic is defined to the bit (fp32, taps in order, no FMA), so EVERY comparison
with the restatement is bit for bit (int32 views), on the smallest shapes that reach each path: tile faces, volumes smaller than a tile and
than the halo, both staging forms, the verbatim copy, the sharpen epilogue, and the augmenter's one, two and three filter passes.

Measured (MI355X, scripts/micro/gaussian_filter_bench.py: roi 96^3, C = 1, device events around 50 warm augmenter calls, median of 7 runs), a call
with patches_training_sample 1 / 2: options off 16.2 / 17.5 us; smooth on every sample at sigma 1.5: 44.5 / 60.8 us (added 28.3 / 43.3 us);
sharpen on every sample: 61.4 / 83.3 us (added 45.3 / 65.8 us); both: 87.9 / 124.3 us (added 71.7 / 106.8 us); one filter call alone at sigma
1.5: 28.1 / 42.1 us, at sigma 2.0: 32.7 / 47.7 us - beside a 96^3 train step of roughly 6 ms."""
import ctypes as C

import numpy as np
import pytest
import torch

import gaussian_filter_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
L_BADARG = -1                                             # MISEG_E_BADARG
# sigma -> radius: 0.25 -> 1, 0.75 -> 3, 1.0 -> 4, 1.5 -> 6, 2.0 -> 8; 0 skips the axis
SIG_614, SIG_888, SIG_030 = (1.5, 0.25, 1.0), (2.0, 2.0, 2.0), (0.0, 0.75, 0.0)


def _A():
    from mi_seg_amd.data import augment
    return augment


def _L():
    from mi_seg_amd.hip import lib
    return lib


def _rand(shape, seed):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)


def _filter(x, sigmas):
    out = _A().gaussian_filter(torch.from_numpy(x).to(DEV), sigmas)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same(got, want):
    return np.array_equal(R.bits(got), R.bits(want))


def test_the_radii_are_the_ones_the_cases_name():
    assert [R.radius(s) for s in (0.25, 0.75, 1.0, 1.5, 2.0)] == [1, 3, 4, 6, 8] and _L().GAUSS_MAX_RADIUS == R.MAX_RADIUS == 8


def _tile_shapes():
    td, th, tw = _L().GAUSS_TILE
    return [(13, 17, 37)] + [(td + e, th + e, tw + e) for e in (-1, 0, 1)]


@pytest.mark.parametrize("which", range(4))
def test_tile_edges(which):
    """radii (6, 1, 4), (8, 8, 8) and (0, 3, 0), one sample each, on a shape off the tile and at tile - 1 / tile / tile + 1 on every axis"""
    shape = _tile_shapes()[which]
    sig = [SIG_614, SIG_888, SIG_030]
    x = _rand((3, 1) + shape, 10 + which)
    got = _filter(x, sig)
    for i in range(3):
        assert _same(got[i], R.smooth(x[i], sig[i])), (shape, sig[i])


@pytest.mark.parametrize("shape", [(3, 2, 5), (1, 1, 1)])
def test_volumes_smaller_than_the_halo(shape):
    x = _rand((2, 1) + shape, 20)
    sig = [(1.5, 1.5, 1.5), (2.0, 2.0, 2.0)]                                             # radius 6 and 8
    got = _filter(x, sig)
    for i in range(2):
        assert _same(got[i], R.smooth(x[i], sig[i])), (shape, i)


def test_samples_channels_and_the_verbatim_copy():
    shape = (9, 18, 35)                                                                  # two tiles along every axis
    x = _rand((3, 2) + shape, 30)
    x[1, 0, 2, 3, 4] = np.float32(-0.0)
    x.view(np.uint32)[1, 1, 8, 17, 34] = 0x7FC12345                                      # a NaN with a payload
    sig = [(1.0, 1.5, 0.25), (0.0, 0.0, 0.0), (0.75, 0.0, 2.0)]
    got = _filter(x, sig)
    assert _same(got[0], R.smooth(x[0], sig[0])) and _same(got[2], R.smooth(x[2], sig[2]))
    assert _same(got[1], x[1]) and R.bits(got[1])[1, 8, 17, 34] == 0x7FC12345 and R.bits(got[1])[0, 2, 3, 4] == np.int32(-2 ** 31)
    # sample i's output does not depend on n
    for i in (0, 2):
        assert _same(_filter(x[i:i + 1], sig[i]), got[i:i + 1])
    assert _same(_filter(x, sig[0])[2], R.smooth(x[2], sig[0]))                          # one triple for every sample


@pytest.mark.parametrize("W", [37, 40])
def test_both_staging_forms(W):
    """src and dst 4 bytes off a 16-byte boundary: 4-byte loads; the same W = 40 volume on the boundary: 16-byte loads"""
    A = _A()
    shape = (2, 1, 5, 6, W)
    x = _rand(shape, 40 + W)
    want = np.stack([R.smooth(x[i], SIG_614) for i in range(2)])
    numel = x.size
    bsrc, bdst = torch.zeros(numel + 8, device=DEV), torch.zeros(numel + 8, device=DEV)
    off = (16 - bsrc.data_ptr() % 16) % 16 // 4
    for shift in (1, 0):
        src, dst = bsrc[off + shift:off + shift + numel].view(shape), bdst[off + shift:off + shift + numel].view(shape)
        assert src.data_ptr() % 16 == 4 * shift and dst.data_ptr() % 16 == 4 * shift
        src.copy_(torch.from_numpy(x))
        bdst.fill_(-7.0)
        A.gaussian_filter(src, SIG_614, out=dst)
        torch.cuda.synchronize()
        assert _same(dst.cpu().numpy(), want), (W, shift)
        flat = bdst.cpu().numpy()
        assert np.all(flat[:off + shift] == -7.0) and np.all(flat[off + shift + numel:] == -7.0)      # nothing outside the batch is written


def test_sharpen():
    A = _A()
    shape = (2, 2, 9, 17, 33)
    x = _rand(shape, 50)
    s1, s2 = [(1.0, 0.5, 0.75), (0.5, 1.0, 1.0)], [(0.5, 0.5, 0.6), (0.5, 0.75, 0.5)]
    dx = torch.from_numpy(x).to(DEV)
    for alpha in (10.0, 30.0, 0.0):
        got = A.gaussian_sharpen(dx, s1, s2, alpha)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        for i in range(2):
            assert _same(got[i], R.sharpen(x[i], s1[i], s2[i], alpha)), (alpha, i)
            if alpha == 0.0:
                assert _same(got[i], R.smooth(x[i], s1[i]))
    got = A.gaussian_sharpen(dx, s1[0], s2[0], [10.0, 30.0]).cpu().numpy()               # one alpha per sample
    assert _same(got[0], R.sharpen(x[0], s1[0], s2[0], 10.0)) and _same(got[1], R.sharpen(x[1], s1[0], s2[0], 30.0))


def test_impulse_and_constant():
    sig = (1.5, 0.25, 1.0)
    wd, wh, ww = (R.taps(s) for s in sig)
    shape = (17, 18, 37)
    x = np.zeros((1, 1) + shape, dtype=np.float32)
    x[0, 0, 8, 15, 31] = 1.0                                                             # its response crosses tile faces on every axis
    got = _filter(x, sig)[0, 0]
    want = (wd[:, None, None] * (wh[None, :, None] * ww[None, None, :]).astype(np.float32)).astype(np.float32)
    assert _same(got[2:15, 14:17, 27:36], want) and np.count_nonzero(got) == want.size
    c = np.float32(0.7)
    got = _filter(np.full((1, 1) + shape, c, dtype=np.float32), sig)[0, 0]
    chain = c
    for w in (ww, wh, wd):                                                               # the interior: the taps' sum chain, pass by pass
        acc = np.float32(0.0)
        for t in w:
            acc = np.float32(acc + np.float32(t * chain))
        chain = acc
    assert np.all(R.bits(got[6:11, 1:17, 4:33]) == R.bits(chain)) and _same(got, R.smooth(np.full(shape, c, dtype=np.float32), sig))
    assert got[0, 0, 0] < got[8, 9, 18] and got[16, 9, 18] < got[8, 9, 18]               # the faces see the zero padding


def test_refusals():
    """every refusal is a host-side check that returns MISEG_E_BADARG before any launch: the output keeps its fill"""
    L, A = _L(), _A()
    so = L.load()
    src = torch.rand((16, 1, 3, 4, 5), device=DEV)
    dst = torch.full((16, 1, 3, 4, 5), -7.0, device=DEV)

    def call(n=1, struct_size=None, same=False, radius=None, nan_tap=False, alpha=0.0, dims=(3, 4, 5)):
        arr = (L.GaussSample * 17)()
        for i in range(17):
            arr[i] = A.gaussian_sample((1.0, 0.5, 0.25), alpha, alpha != 0.0)
        if radius is not None:
            arr[n - 1].radius[1] = radius
        if nan_tap:
            arr[n - 1].taps[2][1] = float("nan")
        q = L.GaussianFilter(C.sizeof(L.GaussianFilter) if struct_size is None else struct_size, src.data_ptr(), src.data_ptr() if same else dst.data_ptr(), n, 1,
                             dims[0], dims[1], dims[2], C.cast(arr, C.c_void_p))
        return so.miseg_gaussian_filter3d(C.byref(q), None), so.miseg_last_error().decode()

    for kw, word in ((dict(radius=9), "radius"), (dict(n=16, radius=-1), "radius"), (dict(same=True), "overlap"), (dict(n=0), "samples"), (dict(n=17), "samples"),
                     (dict(nan_tap=True), "non-finite tap"), (dict(alpha=float("inf")), "alpha"), (dict(struct_size=C.sizeof(L.GaussianFilter) - 8), "struct_size"),
                     (dict(dims=(3, 0, 5)), "below 1")):
        rc, msg = call(**kw)
        assert rc == L_BADARG and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool((dst == -7.0).all())
    assert call()[0] == 0 and call(n=16, alpha=2.0)[0] == 0                              # the same arguments, unspoilt, are served
    torch.cuda.synchronize()
    assert bool((dst != -7.0).all())
    with pytest.raises(ValueError):
        A.gaussian_filter(src, (1.0, 1.0, 1.0), out=src)
    with pytest.raises(ValueError):
        A.gaussian_filter(src, (2.2, 1.0, 1.0))                                          # radius 9


def _volume():
    A = _A()
    g = torch.Generator().manual_seed(14)
    img = torch.rand((2, 20, 24, 18), generator=g)
    lab = torch.randint(0, 5, (20, 24, 18), generator=g)
    return A.ResidentVolume(img.to(DEV), lab.to(DEV), modality=1)


SMOOTH, SHARPEN = (1.2, 0.3, 0.8), ((0.9, 0.6, 0.5), (0.5, 0.55, 0.5), 17.0)


def _expect(gathered, params):
    """the restatement applied to the gather's own output, sample by sample: smooth, then sharpen"""
    out = []
    for g, p in zip(gathered, params):
        if p.get("smooth") is not None:
            g = R.smooth(g, p["smooth"])
        if p.get("sharpen") is not None:
            g = R.sharpen(g, *p["sharpen"])
        out.append(g)
    return np.stack(out)


def test_augmenter_behind_the_affine_gather():
    """smooth on sample 0, sharpen on sample 1, neither on sample 2, with a flip, a quarter turn and noise: three passes behind miseg_augment_affine"""
    A = _A()
    vol, roi = _volume(), (12, 12, 10)
    aug = A.GpuAugmenter(roi, patches_training_sample=3, seed=5)
    base = [dict(origin=[1 + i, 2 * i, 3], flip=[i & 1, 0, 1], rot_k=(1, 0, 3)[i], scale=0.05, shift=-0.02, noise=(0.0, 0.05)) for i in range(3)]
    params = [dict(base[0], smooth=SMOOTH), dict(base[1], sharpen=SHARPEN), dict(base[2])]
    gi, gl = A.augment_affine(vol.image, vol.label, roi, base, seed=aug.seed, draw=0)    # the gather of the first call: draw 0
    out = aug(vol, params)
    torch.cuda.synchronize()
    g = gi.cpu().numpy()
    assert out["image"] is not aug._blur and _same(out["image"].cpu().numpy(), _expect(g, params))
    assert torch.equal(out["label"], gl) and _same(out["image"][2].cpu().numpy(), g[2]) and aug.draws == 1
    # both options absent: today's path and today's bits (the second call's noise is draw 1's)
    plain = aug(vol, base)
    gi1, gl1 = A.augment_affine(vol.image, vol.label, roi, base, seed=aug.seed, draw=1)
    assert torch.equal(plain["image"].view(torch.int32), gi1.view(torch.int32)) and torch.equal(plain["label"], gl1)
    kept = out["image"].clone()
    again = aug(vol, params)                                                             # the kept buffer is reused and never handed out
    assert again["image"] is not aug._blur and torch.equal(kept, out["image"])


@pytest.mark.parametrize("passes", [1, 2, 3])
def test_augmenter_behind_the_crop_gather(passes):
    """no affine / gamma / noise key: miseg_augment_crop writes the batch, then one (smooth), two (sharpen) or three passes"""
    A = _A()
    vol, roi = _volume(), (12, 12, 10)
    aug = A.GpuAugmenter(roi, patches_training_sample=3, seed=5)
    base = [dict(origin=[i, 3, 2 * i], flip=[0, i & 1, 1], rot_k=i, scale=-0.03, shift=0.04) for i in range(3)]
    old = aug(vol, base)
    assert aug._blur is None                                                             # no option, no second buffer
    extra = [dict(smooth=SMOOTH) if passes & 1 else {}, dict(sharpen=SHARPEN) if passes >= 2 else {}, dict(smooth=None, sharpen=None)]
    params = [dict(b, **e) for b, e in zip(base, extra)]
    out = aug(vol, params)
    torch.cuda.synchronize()
    g = old["image"].cpu().numpy()
    assert out["image"] is not aug._blur and _same(out["image"].cpu().numpy(), _expect(g, params))
    assert torch.equal(out["label"], old["label"]) and _same(out["image"][2].cpu().numpy(), g[2]) and aug.draws == 0
