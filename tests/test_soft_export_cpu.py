"""CPU tests of the soft prediction export (hip/ops.py::soft_export's torch path, PredictionGeometry.lerp_tables, training/predict.py's new
options, write_nifti's scaling fields) against the numpy restatement of tests/soft_export_ref.py."""
import hashlib

import numpy as np
import pytest
import torch

import soft_export_ref as ref
from test_hip_predict import SAMPLING, tied_logits
from test_predict_cpu import make_geom, signed_permutation_affines


def _mods():
    from mi_seg_amd.data import nifti, preprocess
    from mi_seg_amd.hip import ops
    from mi_seg_amd.training import predict
    return nifti, preprocess, ops, predict


def orientation_geom(i):
    N, _, _, _ = _mods()
    order, flips = N.ras_orientation(signed_permutation_affines()[i])
    file_shape = (23, 17, 11)
    ras = [file_shape[a] for a in order]
    return make_geom(file_shape, order, flips, (ras[0] // 2 + 1, ras[1], ras[2] * 2 - 3), (3, 0, 1), (2, 0, 0))


def same_tables(got, want):
    (gt, ga), (wt, wa) = got, want
    assert list(ga) == list(wa)
    for g, w in zip(gt, wt):
        assert g[0].dtype == torch.int32 and g[1].dtype == torch.int32 and g[2].dtype == torch.float32
        for x, y in zip(g, w):
            assert np.array_equal(x.numpy(), y), (x, y)


def np_tables(tables):
    return [tuple(np.asarray(v) for v in t) for t in tables]


@pytest.mark.parametrize("i", range(48))
def test_lerp_tables_every_orientation(i):
    g = orientation_geom(i)
    for mode in ("trilinear", "nearest"):
        same_tables(g.lerp_tables(mode), ref.lerp_tables(g, mode))
    tables, axes = g.lerp_tables()
    for a in range(3):
        lo, hi, t = (v.numpy() for v in tables[a])
        k = axes[a]
        first, last = g.pad_before[k], g.pad_before[k] + g.resampled_shape[k] - 1
        assert lo.min() >= first and hi.max() <= last and ((hi == lo) | (hi == lo + 1)).all() and (t >= 0).all() and (t < 1).all()
        assert (t[hi == lo] == 0).all()


@pytest.mark.parametrize("case", range(len(SAMPLING)))
def test_lerp_tables_sampling_geometries(case):
    g = make_geom(*SAMPLING[case])
    for mode in ("trilinear", "nearest"):
        same_tables(g.lerp_tables(mode), ref.lerp_tables(g, mode))


def test_lerp_tables_edges():
    # m == n: t is all zero and lo is the (flipped) arange, offset by the pad before; pads after change nothing
    g = make_geom((31, 29, 64), (1, 2, 0), (True, False, True), (29, 64, 31), (1, 0, 2), (1, 2, 3))
    tables, axes = g.lerp_tables()
    for a in range(3):
        k = axes[a]
        n = g.ras_shape[k]
        r = np.arange(n)[::-1] if g.flips[k] else np.arange(n)
        lo, hi, t = (v.numpy() for v in tables[a])
        assert np.array_equal(lo, r + g.pad_before[k]) and (t == 0).all()
        assert np.array_equal(hi, np.minimum(r + 1, n - 1) + g.pad_before[k])
    # m = 1 (every tap is the one voxel) and n = 1 (one file voxel at the centre of m)
    g = make_geom((1, 9, 6), (0, 1, 2), (False, True, False), (5, 1, 6), (2, 3, 0), (0, 1, 0))
    same_tables(g.lerp_tables(), ref.lerp_tables(g))
    tables, _ = g.lerp_tables()
    lo, hi, t = (v.numpy() for v in tables[0])
    assert lo.tolist() == [4] and hi.tolist() == [5] and t.tolist() == [0.0]           # f = 0.5 * 5 - 0.5 = 2, + pad 2
    lo, hi, t = (v.numpy() for v in tables[1])
    assert (lo == 3).all() and (hi == 3).all() and (t == 0).all()
    with pytest.raises(ValueError, match="mode"):
        g.lerp_tables("cubic")


def test_nearest_tables_reproduce_index_tables():
    for g in [make_geom(*c) for c in SAMPLING] + [orientation_geom(i) for i in (0, 13, 47)]:
        tables, axes = g.lerp_tables("nearest")
        it, ia = g.index_tables()
        assert list(axes) == list(ia)
        for (lo, hi, t), want in zip(tables, it):
            assert torch.equal(lo, want) and torch.equal(hi, want) and (t == 0).all()


def scores_for(g, Cc, seed, tied=False):
    if tied:
        cls = torch.randint(0, Cc, g.padded_shape, generator=torch.Generator().manual_seed(seed))
        return tied_logits(cls, Cc, seed)
    return torch.randn((Cc,) + g.padded_shape, generator=torch.Generator().manual_seed(seed))


def check_cpu_equals_ref(g, Cc, seed, tied=False, dtype=torch.uint16):
    _, _, ops, R = _mods()
    x = scores_for(g, Cc, seed, tied)
    tables, axes = g.lerp_tables()
    lut = R.label_lut(Cc)
    labels, prob = ops.soft_export(x, tables, axes, lut, dtype, softmax=False, probabilities=torch.float32)
    want = ref.blend(x.numpy(), np_tables(tables), axes)
    assert prob.dtype == torch.float32 and np.array_equal(prob.numpy().view(np.uint32), want.view(np.uint32))
    nbytes = torch.empty(0, dtype=dtype).element_size()
    assert labels.dtype == dtype and tuple(labels.shape) == tuple(reversed(g.file_shape))
    assert np.array_equal(labels.numpy(), ref.labels(want, lut.numpy(), nbytes))


@pytest.mark.parametrize("i", [0, 5, 11, 22, 30, 47])
def test_cpu_path_equals_restatement_orientations(i):
    check_cpu_equals_ref(orientation_geom(i), 8, i)
    check_cpu_equals_ref(orientation_geom(i), 8, i, tied=True)


@pytest.mark.parametrize("case", range(len(SAMPLING)))
@pytest.mark.parametrize("Cc,dtype", [(2, torch.uint8), (8, torch.uint16), (14, torch.uint32)])
def test_cpu_path_equals_restatement_sampling(case, Cc, dtype):
    check_cpu_equals_ref(make_geom(*SAMPLING[case]), Cc, 100 * case + Cc, dtype=dtype)


@pytest.mark.parametrize("case", range(len(SAMPLING)))
@pytest.mark.parametrize("Cc", [2, 8, 14])
def test_cpu_softmax_labels_and_margin_share(case, Cc):
    """torch's exp against numpy's: scores within the softmax tolerance, labels equal wherever the restatement's top-two margin is at least
    1e-5, and such thin margins are rare: at most 5e-4 of the voxels (a quarter of the GPU test's 0.2 % cap) for random normal logits"""
    _, _, ops, R = _mods()
    g = make_geom(*SAMPLING[case])
    x = scores_for(g, Cc, 0)
    tables, axes = g.lerp_tables()
    lut = torch.arange(Cc, dtype=torch.int32)
    labels, prob = ops.soft_export(x, tables, axes, lut, torch.uint8, softmax=True, probabilities=torch.float32)
    want = ref.blend(ref.softmax(x.numpy()), np_tables(tables), axes)
    err = np.abs(prob.numpy() - want).max()
    print(f"case {case} C {Cc}: max |p - p_ref| = {err:.3e} (tolerance {ref.softmax_tolerance(Cc):.3e})")
    assert err <= ref.softmax_tolerance(Cc)
    sure = ref.top_two_margin(want) >= 1e-5
    assert (~sure).mean() <= 5e-4
    assert np.array_equal(labels.numpy()[sure], ref.labels(want, lut.numpy(), 1)[sure])
    q = ops.soft_export(x, tables, axes, lut, softmax=True, want_labels=False, probabilities=torch.uint8)[1]
    assert q.dtype == torch.uint8 and (np.abs(q.numpy().astype(np.float64) - 255.0 * want) <= 0.5 + 255 * ref.softmax_tolerance(Cc)).all()


def nan_rule_scores(shape):
    x = torch.randn((5,) + shape, generator=torch.Generator().manual_seed(3))
    x[torch.rand(x.shape, generator=torch.Generator().manual_seed(4)) < 0.2] = float("nan")
    nan = float("nan")
    x[:, 0, 0, 0] = torch.tensor([nan, 9.0, 1.0, 1.0, 1.0])
    x[:, 0, 0, 1] = torch.tensor([1.0, nan, 3.0, 3.0, 0.0])
    x[:, 0, 0, 2] = torch.tensor([1.0, 1.0, 1.0, 1.0, nan])
    return x


@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16, torch.uint32])
def test_all_zero_t_is_the_nearest_export(dtype):
    """m == n (every t zero) and mode="nearest" tables: the labels of invert_prediction(mode="nearest"), the scores a plain gather; an inf or
    NaN at a hi tap does not leak in"""
    _, _, ops, R = _mods()
    g = make_geom((9, 10, 11), (0, 1, 2), (False, False, False), (9, 10, 11), (0, 0, 0), (0, 0, 0))
    x = nan_rule_scores(g.padded_shape)
    x[3, 4, 5, 6] = float("inf")                   # the hi tap of the voxel before it on every axis
    lut = R.label_lut(5)
    want = R.invert_prediction(x, g, lut, dtype=dtype)
    got = R.invert_prediction(x, g, lut, dtype=dtype, mode="trilinear", softmax=False)
    assert got.dtype == dtype and np.array_equal(got.numpy(), want.numpy())
    assert got[0, 0, :3].tolist() == [0, int(lut[2]) & ((1 << (8 * got.element_size())) - 1), 0]
    tables, axes = g.lerp_tables()
    prob = ops.soft_export(x, tables, axes, lut, softmax=False, want_labels=False, probabilities=torch.float32)[1]
    assert np.array_equal(prob.numpy().view(np.uint32), x.permute(0, 3, 2, 1).contiguous().numpy().view(np.uint32))
    for case in SAMPLING:                          # nearest tables on resampling geometries
        g = make_geom(*case)
        x = scores_for(g, 5, 7)
        tables, axes = g.lerp_tables("nearest")
        labels = ops.soft_export(x, tables, axes, lut, dtype, softmax=False)[0]
        assert np.array_equal(labels.permute(2, 1, 0).numpy(), R.invert_prediction(x, g, lut, dtype=dtype).numpy())


def test_wrapper_refusals():
    _, _, ops, R = _mods()
    g = make_geom(*SAMPLING[0])
    x = scores_for(g, 4, 1)
    tables, axes = g.lerp_tables()
    lut = torch.arange(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="nothing to return"):
        ops.soft_export(x, tables, axes, lut, want_labels=False)
    with pytest.raises(ValueError, match=r"uint8 probabilities need scores in \[0, 1\]"):
        ops.soft_export(x, tables, axes, lut, softmax=False, probabilities=torch.uint8)
    assert ops.soft_export(x.sigmoid(), tables, axes, lut, softmax=False, probabilities=torch.uint8, unit_range=True)[1].dtype == torch.uint8
    bad = [tuple(v.clone() for v in t) for t in tables]
    bad[1][1][2] = bad[1][0][2] + 2
    with pytest.raises(ValueError, match=r"hi outside \[lo, lo \+ 1\]"):
        ops.soft_export(x, bad, axes, lut)
    bad = [tuple(v.clone() for v in t) for t in tables]
    bad[0][0][0] = -1
    with pytest.raises(ValueError, match="outside"):
        ops.soft_export(x, bad, axes, lut)
    with pytest.raises(ValueError, match="permutation"):
        ops.soft_export(x, tables, (0, 0, 2), lut)
    with pytest.raises(ValueError, match="mode"):
        R.invert_prediction(x, g, lut, mode="cubic")


def test_write_nifti_scaling_fields(tmp_path):
    N, _, _, _ = _mods()
    rng = np.random.default_rng(5)
    arr = rng.integers(0, 900, (7, 5, 3)).astype(np.uint16)
    A = np.array([[-0.7, 0.1, 0.0, 12.0], [0.2, 0.8, 0.0, -3.5], [0.0, 0.0, 1.6, 7.0], [0, 0, 0, 1.0]])
    path = str(tmp_path / "a.nii")
    N.write_nifti(path, arr, A, compresslevel=1, mtime=0)
    # sha256 of the same call's file on the parent commit, before write_nifti had the scaling arguments
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == "49417e4d45bafbf03cc44f6e82e0651229ccef076290d1e25a327d29e7ad9ab5"
    plain = open(path, "rb").read()
    N.write_nifti(path, arr, A, compresslevel=1, mtime=0, scl_slope=1.0, scl_inter=0.0)
    assert open(path, "rb").read() == plain
    q = rng.integers(0, 256, (4, 5, 6, 3)).astype(np.uint8)
    q[0, 0, 0] = (0, 255, 128)
    for name in ("p.nii", "p.nii.gz"):
        N.write_nifti(str(tmp_path / name), q, A, scl_slope=1.0 / 255.0)
        back, aff = N.read_nifti(str(tmp_path / name))
        assert back.dtype == np.float32 and back.shape == q.shape and np.allclose(aff, A, atol=1e-6)
        assert np.allclose(back, q / 255.0, rtol=0, atol=2.0 ** -23)
        assert back[0, 0, 0, 1] == np.float32(255) * np.float32(1.0 / 255.0)


def test_command_line_options():
    _, _, _, R = _mods()
    a = R.build_parser().parse_args([])
    assert (a.invert_mode, a.invert_quantity, a.save_probabilities, a.probability_dtype) == ("nearest", "probabilities", False, "float32")
    opt = R.export_options(a)
    assert opt == dict(mode="nearest", quantity="probabilities", save=False, kind="logits", dtype=torch.float32)
    a = R.build_parser().parse_args(["--invert_mode", "trilinear", "--invert_quantity", "logits", "--save_probabilities", "--probability_dtype", "uint8"])
    opt = R.export_options(a)
    assert (opt["mode"], opt["quantity"], opt["save"], opt["dtype"], opt["kind"]) == ("trilinear", "logits", True, torch.uint8, "logits")
    for bad in (["--invert_mode", "cubic"], ["--invert_quantity", "votes"], ["--probability_dtype", "float16"]):
        with pytest.raises(SystemExit):
            R.build_parser().parse_args(bad)
    flips = ["--infer_tta_flips", "0"]
    vote = R.build_parser().parse_args(flips + ["--ensemble_mode", "vote", "--save_probabilities", "--probability_dtype", "uint8"])
    with pytest.raises(SystemExit, match="vote counts, which are not normalised"):
        R.export_options(vote)
    with pytest.raises(SystemExit, match="vote counts, which are not normalised"):
        R.main(flips + ["--ensemble_mode", "vote", "--save_probabilities", "--probability_dtype", "uint8"])
    assert R.export_options(R.build_parser().parse_args(flips + ["--ensemble_mode", "vote", "--save_probabilities"]))["kind"] == "vote"
    prob = R.export_options(R.build_parser().parse_args(flips + ["--ensemble_mode", "mean_prob", "--save_probabilities", "--probability_dtype", "uint8"]))
    assert prob["kind"] == "mean_prob" and prob["dtype"] == torch.uint8
    # one member: the inferer returns logits whatever --ensemble_mode says
    assert R.export_options(R.build_parser().parse_args(["--ensemble_mode", "vote", "--save_probabilities", "--probability_dtype", "uint8"]))["kind"] == "logits"
    assert R.probability_path("/r/ct_test_2001_label.nii.gz") == "/r/ct_test_2001_label_prob.nii.gz"
    assert R.probability_path("mr_label.nii") == "mr_label_prob.nii.gz"
    help_text = R.build_parser().format_help()
    assert "--invert_mode" in help_text and "not normalised" in " ".join(help_text.split())
