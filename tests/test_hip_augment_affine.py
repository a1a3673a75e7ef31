"""GPU tests of rotation / zoom / gamma / noise on the device augmenter (csrc/augment.hip::miseg_augment_affine, data/augment.py; DESIGN.md
section 7.11) against the numpy restatement of tests/augment_affine_ref.py: bit for bit where the fp32 arithmetic is exact (the identity, the
quarter turns, dyadic matrices), within bounds derived from the roundings of each chain elsewhere.  Every measured worst case is printed
before it is asserted; the figures of an MI355X run stand in DESIGN.md section 7.11.

Measured (MI355X): generic sets 1 / 2 / 3: image 1.86e-6 / 2.11e-6 / 2.27e-6 = 0.13 / 0.16 / 0.16 of the bound (E_c 1.61e-5 / 2.24e-5 / 1.93e-5), no
label wrong anywhere, 0.143 / 0.078 / 0.039 % excluded; gamma 0.5 / 1 / 2.7: 1.62e-7 / 9.47e-8 / 2.11e-7 = at most 0.07 / 0.08 / 0.57 of the bound;
noise: 4.31e-7 = at most 0.49 of the bound."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import augment_affine_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
DELTA = 2.5e-4            # labels are compared where the position is farther than this from a nearest-neighbour tie
L_BADARG, L_UNSUPPORTED = -1, -2          # MISEG_E_BADARG, MISEG_E_UNSUPPORTED


def _A():
    from mi_seg_amd.data import augment
    return augment


def _scratch():
    return torch.zeros(64, dtype=torch.int32, device=DEV)


def _run(img, lab, roi, samples, padding="border", seed=0, draw=0, minmax=None):
    """-> (image float32 numpy [n, C, roi], label numpy [n, roi]); the gamma scratch is checked to come back zeroed"""
    minmax = _scratch() if minmax is None else minmax
    oi, ol = _A().augment_affine(img, lab, roi, samples, padding_mode=padding, seed=seed, draw=draw, minmax=minmax)
    torch.cuda.synchronize()
    assert int(minmax.abs().sum()) == 0
    return oi.cpu().numpy(), ol[:, 0].cpu().numpy()


def _image_bound(r, sm, roi):
    """|kernel - restatement| of a sample without gamma and noise: the position is off by at most E_c per axis, which moves the trilinear value
    by at most E_c times the sum over the axes of the largest neighbour difference; the seven lerps are given 4 ulp of the largest
    neighbour (DESIGN.md section 7.11 counts their roundings); fl(1 + scale) and the fma of the scale and shift round once each"""
    mul = abs(float(np.float32(1.0) + np.float32(sm["scale"])))
    b = (R.coord_error_bound(roi, sm) * r["spread"] + 4 * R.ULP * r["vmax"]) * mul
    return b + R.U24 * (np.abs(r["resampled"]) * mul + np.abs(r["image"]))


def _rand_volume(shape, Cc, seed, ldtype=torch.int64, values=(0, 3, 5, 7, 11)):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand((Cc,) + tuple(shape), generator=g)
    lab = torch.tensor(values)[torch.randint(0, len(values), tuple(shape), generator=g)].to(ldtype)
    return img, lab


def test_identity_is_the_old_kernel():
    A = _A()
    g = torch.Generator().manual_seed(5)
    img = torch.randn((2, 20, 24, 18), generator=g).to(DEV)
    for ldt in (torch.uint8, torch.float32, torch.int64):
        lab = torch.randint(0, 9, (20, 24, 18), generator=g).to(ldt).to(DEV)
        vol = A.ResidentVolume(img, lab, modality=1)
        aug = A.GpuAugmenter((12, 12, 10), patches_training_sample=3, randFlipd_prob=0.5, randRotate90d_prob=0.7, randScaleIntensityd_prob=0.6,
                             randShiftIntensityd_prob=0.6, seed=7)
        params = [{k: v for k, v in p.items() if k not in ("affine", "gamma", "noise")} for p in aug.draw(vol)]
        assert any(p["rot_k"] & 1 for p in params) and any(any(p["flip"]) for p in params)
        old = aug(vol, params)                                                   # no new key: miseg_augment_crop
        oi, ol = A.augment_affine(vol.image, vol.label, (12, 12, 10), params)   # identity m, zero t, no gamma, no noise, no scratch
        assert torch.equal(oi.view(torch.int32), old["image"].view(torch.int32)) and torch.equal(ol, old["label"])


def test_quarter_turn_is_rot_k():
    A = _A()
    g = torch.Generator().manual_seed(6)
    img = torch.randn((2, 16, 14, 15), generator=g).to(DEV)
    lab = torch.randint(0, 9, (16, 14, 15), generator=g).to(DEV)
    vol = A.ResidentVolume(img, lab)
    aug = A.GpuAugmenter(12)
    for angle, k in ((-math.pi / 2, 1), (math.pi / 2, 3)):
        for origin, flip in (((0, 0, 0), (0, 0, 0)), ((4, 2, 3), (0, 0, 1)), ((2, 1, 0), (0, 0, 0))):
            base = dict(origin=list(origin), flip=list(flip), scale=0.07, shift=-0.03)
            old = aug(vol, [dict(base, rot_k=k)])
            m = A.affine_matrix((0, 0, angle))
            for padding in ("border", "zeros"):                                 # the turned patch stays inside its crop: no padding is read
                oi, ol = A.augment_affine(vol.image, vol.label, (12, 12, 12), [dict(base, rot_k=0, m=m, t=(0, 0, 0))], padding_mode=padding)
                assert torch.equal(oi.view(torch.int32), old["image"].view(torch.int32)) and torch.equal(ol, old["label"]), (angle, origin, padding)


DYADIC = [  # (m, t, origin): entries of m from {0, +-1/4, +-1/2, +-1, +-2}, t in multiples of 1/4
    (np.diag([2.0, 2.0, 2.0]), (0.25, -0.25, 0.5), (2, 1, 2)),                                   # leaves the volume through all six faces
    ([[0.5, 0.25, 0], [-0.25, 1, 0.5], [0, -0.5, 2]], (-1.75, 0.5, 0.25), (0, 3, 0)),
    ([[-1, 0, 0.25], [0, 0.5, -2], [0.25, 0, 1]], (2.5, -0.75, 3.0), (4, 0, 4)),
    ([[0, 1, 0], [-2, 0, 0], [0, 0, -0.5]], (0, 0, 0), (4, 3, 4)),
]


@pytest.mark.parametrize("padding", ["border", "zeros"])
def test_exact_dyadic_cases(padding):
    """every coordinate and weight is exact in fp32 and every lerp of an 8-bit integer image too: the result is the float64 restatement's,
    rounded to fp32 (which changes nothing), whatever the order or contraction of the arithmetic"""
    g = torch.Generator().manual_seed(8)
    shape, roi = (10, 9, 8), (6, 6, 4)
    img = torch.randint(0, 256, (2,) + shape, generator=g).float()
    lab = torch.randint(1, 6, shape, generator=g)                               # no label 0 in the volume: a 0 in the output is padding
    samples = [R.identity_sample(o, flip=(i & 1, 0, (i >> 1) & 1), rot_k=i & 3, m=m, t=t) for i, (m, t, o) in enumerate(DYADIC)]
    ref = R.augment_affine_ref(img.numpy(), lab.numpy(), roi, samples, padding)
    s_all = np.stack([r["s"] for r in ref])
    for a, n in enumerate(shape):                                               # reads leave the volume through each of the six faces
        assert s_all[:, a].min() < 0 and s_all[:, a].max() > n - 1
    oi, ol = _run(img.to(DEV), lab.to(DEV), roi, samples, padding)
    for i, r in enumerate(ref):
        assert np.array_equal(oi[i].view(np.int32), r["image"].astype(np.float32).view(np.int32)), i
        assert np.array_equal(ol[i], r["label"]), i
        n = np.floor(r["s"] + 0.5)
        outside = np.zeros(n.shape[1:], dtype=bool)
        for a, ext in enumerate(shape):
            outside |= (n[a] < 0) | (n[a] >= ext)
        assert outside.any() and np.array_equal(ol[i] == 0, outside if padding == "zeros" else np.zeros_like(outside))


GENERIC = [((0.52, -0.31, 0.17), (0.8, 1.3, 1.05), (0.4, -1.2, 2.3), (8, 12, 10)),
           ((-0.52, 0.52, -0.52), (1.3, 1.3, 1.3), (-3.1, 0.7, 1.9), (0, 24, 20)),
           ((0.11, 0.44, 0.52), (1.21, 0.8, 0.93), (1.5, 2.5, -0.6), (16, 0, 3))]


def test_generic_angles():
    A = _A()
    shape, roi = (40, 44, 36), (24, 20, 16)
    img, lab = _rand_volume(shape, 2, 9, torch.int32)
    zz, yy, xx = torch.meshgrid(*(torch.arange(n, dtype=torch.float32) for n in shape), indexing="ij")
    img[1] = 0.5 + 0.5 * torch.sin(0.31 * zz + 0.2) * torch.cos(0.23 * yy) * torch.sin(0.17 * xx + 1.0)        # a smooth channel: small neighbour differences
    samples = [R.identity_sample(o, flip=(i == 1, 0, i == 2), rot_k=0, m=A.affine_matrix(rot, zoom), t=t, scale=0.05 * i, shift=-0.02 * i)
               for i, (rot, zoom, t, o) in enumerate(GENERIC)]
    ref = R.augment_affine_ref(img.numpy(), lab.numpy(), roi, samples, "border")
    oi, ol = _run(img.to(DEV), lab.to(DEV), roi, samples, "border")
    values = set(np.unique(lab.numpy()).tolist())
    for i, (sm, r) in enumerate(zip(samples, ref)):
        e_c = R.coord_error_bound(roi, sm)
        assert e_c < DELTA / 4, e_c
        err, bound = np.abs(oi[i] - r["image"]), _image_bound(r, sm, roi)
        clear = R.half_distance(r["s"]) > DELTA
        wrong = int((ol[i][clear] != r["label"][clear]).sum())
        print(f"generic set {i}: E_c {e_c:.3e}; image max err {err.max():.3e}, max err / bound {float((err / bound).max()):.3f}; "
              f"labels excluded {100 * (1 - clear.mean()):.3f} %, wrong outside the exclusion {wrong}, wrong in all {int((ol[i] != r['label']).sum())}")
        assert np.all(err <= bound)
        assert 1 - clear.mean() <= 0.005
        assert wrong == 0
        assert set(np.unique(ol[i]).tolist()) <= values


@pytest.mark.parametrize("n,Cc", [(1, 1), (16, 3), (16, 1), (1, 3)])
def test_tails_and_counts(n, Cc):
    """105 voxels a patch: one partly filled workgroup; 1 and 16 samples; every sample against the restatement, with every option somewhere"""
    A = _A()
    shape, roi = (9, 8, 6), (7, 5, 3)
    img, lab = _rand_volume(shape, Cc, 10 + n + Cc, torch.uint8)
    g = np.random.default_rng(n * 10 + Cc)
    samples = []
    for i in range(n):
        ident = i % 4 == 3
        m = None if ident else A.affine_matrix(g.uniform(-0.4, 0.4, 3), g.uniform(0.8, 1.3, 3))
        samples.append(R.identity_sample([int(g.integers(0, s - r + 1)) for s, r in zip(shape, roi)], flip=g.integers(0, 2, 3).tolist(), rot_k=int(g.integers(0, 2)) * 2,
                                         m=m, t=(0, 0, 0) if ident else g.uniform(-1, 1, 3), scale=float(g.uniform(-0.1, 0.1)), shift=float(g.uniform(-0.1, 0.1)),
                                         noise=(0.1, 0.2) if i % 3 == 1 else (0.0, 0.0)))
    for padding in ("border", "zeros"):
        ref = R.augment_affine_ref(img.numpy(), lab.numpy(), roi, samples, padding, seed=3, draw=9)
        oi, ol = _run(img.to(DEV), lab.to(DEV), roi, samples, padding, seed=3, draw=9)
        for i, (sm, r) in enumerate(zip(samples, ref)):
            bound = _image_bound(r, sm, roi)
            if sm["noise_std"] > 0:
                bound = bound + sm["noise_std"] * R.noise_z_bound(r["u1"]) + 3 * R.U24 * (np.abs(r["image"]) + np.abs(r["image"] - r["before_noise"]))
            assert np.all(np.abs(oi[i] - r["image"]) <= bound), (padding, i)
            clear = R.half_distance(r["s"]) > DELTA
            assert np.array_equal(ol[i][clear], r["label"][clear]), (padding, i)


def _exact_volume(shape, Cc, seed):
    """values in multiples of 1/64 in [-1, 1): with a dyadic matrix the resampled values are exact in fp32, so gamma and noise are judged alone"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-64, 64, (Cc,) + tuple(shape), generator=g).float() / 64, torch.randint(0, 5, tuple(shape), generator=g)


def test_gamma():
    shape, roi = (10, 9, 8), (6, 6, 4)
    img, lab = _exact_volume(shape, 2, 12)
    const = torch.full((2,) + shape, 0.375)
    worst = 0.0
    for gamma in (0.5, 1.0, 2.7):
        # sample 0: the integer path; sample 1: zeros padding around negative values (the padding's 0 lies inside the range); sample 2: border
        samples = [R.identity_sample((2, 1, 3), flip=(1, 0, 0), gamma=gamma),
                   R.identity_sample((2, 1, 2), m=np.diag([2.0, 2.0, 2.0]), t=(0.25, -0.25, 0.5), gamma=gamma),
                   R.identity_sample((0, 3, 0), m=[[0.5, 0.25, 0], [-0.25, 1, 0.5], [0, -0.5, 2]], t=(-1.75, 0.5, 0.25), gamma=gamma)]
        for padding in ("zeros", "border"):
            ref = R.augment_affine_ref(img.numpy(), lab.numpy(), roi, samples, padding)
            oi, ol = _run(img.to(DEV), lab.to(DEV), roi, samples, padding)
            for i, r in enumerate(ref):
                assert r["lo"] < 0 and np.array_equal(r["resampled"].astype(np.float32).astype(np.float64), r["resampled"])
                err, bound = np.abs(oi[i] - r["image"]), R.gamma_bound(r["resampled"], gamma, r["lo"], r["range"])
                worst = max(worst, float((err / np.maximum(bound, 1e-30)).max()))
                print(f"gamma {gamma} {padding} sample {i}: max err {err.max():.3e} (range {r['range']:.3f}), max err / bound {float((err / np.maximum(bound, 1e-30)).max()):.3f}")
                assert np.all(err <= bound), (gamma, padding, i)
                assert np.array_equal(ol[i], r["label"])
        oc, _ = _run(const.to(DEV), lab.to(DEV), roi, samples, "border")        # a constant patch returns the constant
        assert np.all(oc == np.float32(0.375))
    assert worst <= 1.0
    # gamma on sample 1 only: samples 0 and 2 carry the bits of the run without gamma
    plain = [dict(s, gamma=0.0, scale=0.05, shift=0.01) for s in samples]
    mixed = [dict(s, gamma=1.7 if i == 1 else 0.0) for i, s in enumerate(plain)]
    a, _ = _run(img.to(DEV), lab.to(DEV), roi, plain, "zeros")
    b, _ = _run(img.to(DEV), lab.to(DEV), roi, mixed, "zeros")
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[2].view(np.int32), b[2].view(np.int32))
    assert not np.array_equal(a[1], b[1])


def test_noise():
    shape, roi, Cc = (14, 13, 12), (12, 12, 12), 3
    img, lab = _exact_volume(shape, Cc, 13)
    mean, std = 0.25, 0.5
    base = [R.identity_sample((i % 3, 1, 0), flip=(0, i & 1, 0), noise=(mean, std)) for i in range(5)]
    dimg, dlab = img.to(DEV), lab.to(DEV)
    o3, _ = _run(dimg, dlab, roi, base[:3], seed=21, draw=4)
    ref = R.augment_affine_ref(img.numpy(), lab.numpy(), roi, base[:3], "border", seed=21, draw=4)
    for i, r in enumerate(ref):
        v = r["before_noise"]                                                   # the gathered values: exact
        want = mean + std * R.noise_z64(r["u1"], r["u2"])                       # from the exact uint64 uniforms
        # fl(std * z), fl(mean + .), fl(v + .): three roundings behind z's own bound
        bound = std * R.noise_z_bound(r["u1"]) + R.U24 * (np.abs(want - mean) + np.abs(want) + np.abs(v + want))
        err = np.abs(o3[i].astype(np.float64) - (v + want))
        print(f"noise sample {i}: max err {err.max():.3e}, max err / bound {float((err / bound).max()):.3f}")
        assert np.all(err <= bound), i
        z = (o3[i].astype(np.float64) - v).reshape(-1)
        N = z.size
        assert N == 3 * 12 ** 3
        assert abs(z.mean() - mean) <= 5 * std / math.sqrt(N) and abs(z.std() - std) <= 5 * std / math.sqrt(2 * N), (z.mean(), z.std())
    again, _ = _run(dimg, dlab, roi, base[:3], seed=21, draw=4)
    other, _ = _run(dimg, dlab, roi, base[:3], seed=21, draw=5)
    assert np.array_equal(again.view(np.int32), o3.view(np.int32)) and not np.array_equal(other, o3)
    o5, _ = _run(dimg, dlab, roi, base, seed=21, draw=4)                        # sample i's noise does not depend on n
    assert np.array_equal(o5[2].view(np.int32), o3[2].view(np.int32))


def test_whole_chain_twice():
    A = _A()
    shape, roi = (20, 24, 18), (12, 12, 10)
    img, lab = _rand_volume(shape, 2, 14)
    samples = [R.identity_sample((i, 2 * i, 1), flip=(i & 1, 0, 1), rot_k=i & 3, m=A.affine_matrix((0.1 * i, -0.2, 0.3), (1.1, 0.9, 1.2)), t=(0.3, -0.4, 0.5 * i),
                                 scale=0.05, shift=-0.02, gamma=1.0 + 0.5 * i, noise=(0.0, 0.05 * (i + 1))) for i in range(4)]
    scratch = _scratch()
    a = _run(img.to(DEV), lab.to(DEV), roi, samples, "zeros", seed=2, draw=7, minmax=scratch)
    b = _run(img.to(DEV), lab.to(DEV), roi, samples, "zeros", seed=2, draw=7, minmax=scratch)       # the same scratch, handed back zeroed
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1]) and np.isfinite(a[0]).all()
    ref = R.augment_affine_ref(img.numpy(), lab.numpy(), roi, samples, "zeros", seed=2, draw=7)
    # the chain's order (gamma, then scale / shift, then noise).  With rb the resample bound, v, lo and max are each off by at most rb; for
    # gamma >= 1 the power has slope <= gamma on [0, 1], so v' = x^gamma * range + lo moves by at most (2 gamma + 3) rb
    for i, (sm, r) in enumerate(zip(samples, ref)):
        rb = float((R.coord_error_bound(roi, sm) * r["spread"] + 4 * R.ULP * r["vmax"]).max())
        mul = float(np.float32(1.0) + np.float32(sm["scale"]))
        bound = ((2 * sm["gamma"] + 3) * rb + R.gamma_bound(r["resampled"], sm["gamma"], r["lo"], r["range"])) * mul + \
            sm["noise_std"] * R.noise_z_bound(r["u1"]) + 4 * R.U24 * (np.abs(r["image"]) + np.abs(r["before_noise"]))
        assert np.all(np.abs(a[0][i] - r["image"]) <= bound), i


def test_refusals():
    """each refusal returns its code before any launch: the outputs keep their fill"""
    from mi_seg_amd.hip import lib as L
    A = _A()
    so = L.load()
    img = torch.rand((1, 9, 8, 6), device=DEV)
    lab = torch.ones((9, 8, 6), dtype=torch.uint8, device=DEV)
    oi = torch.full((16, 1, 7, 5, 3), -7.0, device=DEV)
    ol = torch.full((16, 1, 7, 5, 3), 9, dtype=torch.uint8, device=DEV)
    scratch = _scratch()

    def call(n=1, roi=(7, 5, 3), label_bytes=1, padding=0, struct_size=None, minmax=True, **kw):
        arr = (L.AugAffineSample * 17)()
        for i in range(17):
            arr[i] = A.affine_sample(R.identity_sample((0, 0, 0), **kw))
        q = L.AugmentAffine(C.sizeof(L.AugmentAffine) if struct_size is None else struct_size, img.data_ptr(), lab.data_ptr(), label_bytes, 1, 9, 8, 6, roi[0], roi[1],
                            roi[2], n, oi.data_ptr(), ol.data_ptr(), C.cast(arr, C.c_void_p), padding, 1, 2, scratch.data_ptr() if minmax else None)
        return so.miseg_augment_affine(C.byref(q), None), so.miseg_last_error().decode()

    for kw, code, word in ((dict(struct_size=C.sizeof(L.AugmentAffine) - 8), L_BADARG, "struct_size"), (dict(n=0), L_UNSUPPORTED, "samples"),
                           (dict(n=17), L_UNSUPPORTED, "samples"), (dict(label_bytes=2), L_UNSUPPORTED, "label element"),
                           (dict(padding=2), L_UNSUPPORTED, "padding_mode"), (dict(rot_k=1), L_BADARG, "quarter turns"),
                           (dict(rot_k=3), L_BADARG, "quarter turns"), (dict(gamma=1.5, minmax=False), L_BADARG, "minmax"),
                           (dict(t=(float("nan"), 0, 0)), L_BADARG, "non-finite")):
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool((oi == -7.0).all()) and bool((ol == 9).all()) and int(scratch.abs().sum()) == 0
    assert call()[0] == 0 and call(n=16, gamma=1.5)[0] == 0                    # the same arguments, unspoilt, are served
    torch.cuda.synchronize()
    assert bool((oi != -7.0).all()) and int(scratch.abs().sum()) == 0


def test_gpu_augmenter_end_to_end():
    A = _A()
    from mi_seg_amd.data.synthetic import synthetic_volume
    img, lab = synthetic_volume((48, 56, 40), 3, 1)
    vol = A.ResidentVolume(img[0].to(DEV), lab[0, 0].to(DEV), modality=1)
    aug = A.GpuAugmenter(32, patches_training_sample=4, randFlipd_prob=1.0, randRotate90d_prob=1.0, randScaleIntensityd_prob=1.0, randShiftIntensityd_prob=1.0,
                         randAffined_prob=1.0, rotate_range=(0.3, 0.3, 0.3), scale_range=(0.2, 0.2, 0.2), translate_range=(3, 3, 3), randAdjustContrastd_prob=1.0,
                         randGaussianNoised_prob=1.0, seed=4)
    for padding in ("border", "zeros"):
        aug.padding_mode = padding
        params = aug.draw(vol)
        assert all(p["affine"] is not None and p["gamma"] is not None and p["noise"] is not None for p in params)
        out = aug(vol, params)
        assert out["image"].shape == (4, 1, 32, 32, 32) and out["image"].dtype == torch.float32 and bool(torch.isfinite(out["image"]).all())
        assert out["label"].shape == (4, 1, 32, 32, 32) and out["label"].dtype == torch.int64
        assert set(out["label"].unique().tolist()) <= set(vol.label.unique().tolist())
        assert out["modality"].tolist() == [1] * 4
    assert aug.draws == 2 and int(aug._minmax.abs().sum()) == 0
    # dicts without the new keys still go through the old entry point and leave the draw counter alone
    old = aug(vol, [{k: v for k, v in p.items() if k not in ("affine", "gamma", "noise")} for p in params])
    assert aug.draws == 2 and old["image"].shape == (4, 1, 32, 32, 32)
