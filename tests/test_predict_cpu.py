"""CPU tests of the prediction export (training/predict.py, reference predict_whs.py): the orientation rule and its inverse on every signed
axis permutation, the CPU path of invert_prediction against a plain numpy composition of the reference's inverse transforms, the label remap,
the command line and the file round trip."""
import itertools
import os

import numpy as np
import pytest
import torch


def _mods():
    from mi_seg_amd.data import nifti, preprocess
    from mi_seg_amd.training import predict
    return nifti, preprocess, predict


REF_MAP = {1: 500, 2: 600, 3: 420, 4: 550, 5: 205, 6: 820, 7: 850}


def remap_tensor(tensor, map_dict):
    """the reference's sequential remap (predict_whs.py:29-32)"""
    for key, value in map_dict.items():
        tensor[tensor == key] = value
    return tensor


def signed_permutation_affines():
    """all 48 signed axis permutations, anisotropic voxels and a non-zero origin"""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            A = np.zeros((4, 4))
            for a, w in enumerate(perm):
                A[w, a] = signs[a] * (0.7, 0.8, 1.6)[a]
            A[:3, 3] = (-12.5, 30.25, 7.0)
            A[3, 3] = 1.0
            out.append(A)
    return out


def gather_np(vol, tables, axes):
    """out[x][y][z] = vol[...] with the index along vol axis axes[a] = tables[a][coordinate a]"""
    idx = [None] * 3
    for a in range(3):
        shape = [1, 1, 1]
        shape[a] = -1
        idx[axes[a]] = np.asarray(tables[a]).reshape(shape)
    return vol[idx[0], idx[1], idx[2]]


def first_max_np(x):
    arg = np.zeros(x.shape[1:], dtype=np.int64)
    mx = x[0].copy()
    for c in range(1, x.shape[0]):
        up = x[c] > mx
        mx[up] = x[c][up]
        arg[up] = c
    return arg


def nearest_np(n_in, n_out):
    """miseg_resample3d's nearest rule in fp32 with its contracted multiply-add: floor(fma(dst + 0.5, in / out, -0.5) + 0.5), clamped"""
    r = np.float32(n_in) / np.float32(n_out)
    out = []
    for d in range(n_out):
        t = np.float32(float(np.float32(d) + np.float32(0.5)) * float(r) - 0.5)
        out.append(min(max(int(np.floor(t + np.float32(0.5))), 0), n_in - 1))
    return np.array(out)


def inverse_np(logits, geom, lut):
    """the reference's way back as plain numpy: argmax (first maximum), crop the pad, nearest resampling to the RAS size, undo the
    orientation, remap"""
    cls = first_max_np(logits)
    cls = cls[tuple(slice(b, b + m) for b, m in zip(geom.pad_before, geom.resampled_shape))]
    for k in range(3):
        cls = np.take(cls, nearest_np(geom.resampled_shape[k], geom.ras_shape[k]), axis=k)
    for k in range(3):
        if geom.flips[k]:
            cls = np.flip(cls, k)
    cls = np.transpose(cls, np.argsort(geom.order))
    return np.asarray(lut, dtype=np.int64)[cls]


def make_geom(file_shape, order, flips, resampled, pad_before, pad_after, affine=None):
    _, P, _ = _mods()
    ras = tuple(file_shape[a] for a in order)
    return P.PredictionGeometry(tuple(file_shape), np.eye(4) if affine is None else affine, list(order), list(flips), ras, tuple(resampled),
                                tuple(pad_before), tuple(pad_after))


def tied_logits_np(cls, C, seed):
    """integer-valued logits whose first maximum is `cls`, with exact ties in later channels"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 3, (C,) + cls.shape).astype(np.float32)
    idx = np.arange(C).reshape((C,) + (1,) * cls.ndim)
    tie = (rng.integers(0, 2, x.shape) == 1) & (idx > cls[None])
    x = np.where((idx == cls[None]) | tie, np.float32(5.0), x)
    assert np.array_equal(first_max_np(x), cls)
    return x


@pytest.mark.parametrize("A", signed_permutation_affines())
def test_ras_orientation_and_tables_undo_reorient_to_ras(A):
    N, P, _ = _mods()
    rng = np.random.default_rng(0)
    vol = rng.integers(0, 1000, (5, 6, 7)).astype(np.int32)
    ras, _ = N.reorient_to_ras(vol, A)
    order, flips = N.ras_orientation(A)
    assert sorted(order) == [0, 1, 2] and len(flips) == 3
    moved = np.transpose(vol, order)
    for k in range(3):
        if flips[k]:
            moved = np.flip(moved, k)
    assert np.array_equal(moved, ras)                                     # reorient_to_ras is the permutation + flips of ras_orientation
    g = make_geom(vol.shape, order, flips, ras.shape, (0, 0, 0), (0, 0, 0), A)
    tables, axes = g.index_tables()
    assert all(t.dtype == torch.int32 for t in tables)
    assert np.array_equal(gather_np(ras, [t.numpy() for t in tables], axes), vol)


@pytest.mark.parametrize("case", [
    ((9, 7, 11), (1, 2, 0), (True, False, True), (5, 7, 17), (2, 0, 1), (1, 0, 3)),      # down / equal / up, pads on two axes
    ((13, 5, 6), (2, 0, 1), (False, True, True), (13, 9, 4), (0, 3, 0), (0, 2, 0)),     # equal / up / down
    ((17, 19, 3), (0, 1, 2), (True, True, False), (6, 23, 3), (0, 0, 0), (0, 0, 0)),    # LPS-like, no pad
])
@pytest.mark.parametrize("C", [2, 8, 14])
def test_cpu_invert_prediction_equals_numpy_composition(case, C):
    _, _, R = _mods()
    file_shape, order, flips, resampled, pb, pa = case
    g = make_geom(file_shape, order, flips, resampled, pb, pa)
    rng = np.random.default_rng(C)
    cls = rng.integers(0, C, g.padded_shape)
    logits = tied_logits_np(cls, C, C + 1)
    lut = R.label_lut(C)
    got = R.invert_prediction(torch.from_numpy(logits), g, lut)
    assert got.dtype == torch.uint16 and tuple(got.shape) == file_shape
    assert got.permute(2, 1, 0).is_contiguous()                           # an [X, Y, Z] view of a [Z, Y, X] buffer
    want = inverse_np(logits, g, lut.numpy())
    assert np.array_equal(got.numpy().astype(np.int64), want)
    for dtype, mask in ((torch.uint8, 0xFF), (torch.uint32, 0xFFFFFFFF)):
        got = R.invert_prediction(torch.from_numpy(logits), g, lut, dtype=dtype)
        assert got.dtype == dtype and np.array_equal(got.numpy().astype(np.int64), want & mask)


def test_nearest_index_is_the_fp32_rule():
    _, P, _ = _mods()
    for n_in in (1, 2, 3, 5, 7, 64, 97, 180, 512):
        for n_out in (1, 2, 3, 4, 9, 64, 129, 363, 512):
            assert np.array_equal(P.nearest_index(n_in, n_out), nearest_np(n_in, n_out)), (n_in, n_out)


def test_cpu_argmax_rule_with_nans():
    _, _, R = _mods()
    from mi_seg_amd.hip import ops
    x = torch.tensor([[np.nan, 1.0, 0.0, 2.0], [5.0, np.nan, 0.0, 2.0], [9.0, 7.0, np.nan, 2.0]], dtype=torch.float32)
    assert ops.first_max_argmax(x).tolist() == [0, 2, 0, 0]               # NaN in channel 0 -> 0; a later NaN never wins; ties -> first


@pytest.mark.parametrize("C", [8, 14])
def test_label_lut_equals_the_sequential_remap(C):
    _, _, R = _mods()
    assert R.LABEL_MAP == REF_MAP
    lut = R.label_lut(C)
    classes = torch.arange(C)
    assert torch.equal(lut.long(), remap_tensor(classes.clone(), REF_MAP))
    assert lut[8:].tolist() == list(range(8, C))


def test_parser_defaults_match_the_reference():
    _, _, R = _mods()
    a = R.build_parser().parse_args([])
    assert (a.checkpoint, a.sample, a.space_x, a.space_y, a.space_z, a.no_gpu) == ("", "", 1.0, 1.0, 1.0, False)
    assert (a.data_dir, a.json_list, a.result_dir) == ("dataset/MM-WHS", "CT_test.json", "dataset/MM_WHS/MM_WHS_test/CT/")
    assert (a.model_name, a.roi_x, a.infer_overlap, a.sw_batch_size) == ("unetr", 96, 0.5, 1)     # the model options ride along


def test_output_names_and_result_dir(tmp_path):
    _, _, R = _mods()
    assert R.output_path("/d/imagesTs/ct_test_2001_image.nii.gz", "out") == os.path.join("out", "ct_test_2001_label.nii.gz")
    assert R.output_path("mr_test_2001_image.nii", "/r") == os.path.join("/r", "mr_test_2001_label.nii")
    args = R.build_parser().parse_args(["--result_dir", str(tmp_path / "a" / "b")])
    assert R.predict(torch.nn.Identity(), [], args) == [] and (tmp_path / "a" / "b").is_dir()


def test_no_gpu_is_refused():
    _, _, R = _mods()
    with pytest.raises(SystemExit, match="HIP device only"):
        R.main(["--no_gpu"])


@pytest.mark.parametrize("name", ["x_label.nii", "x_label.nii.gz"])
def test_zyx_buffer_written_through_its_xyz_view(tmp_path, name):
    N, _, R = _mods()
    buf = torch.randint(0, 900, (5, 7, 9), dtype=torch.int32).to(torch.uint16)         # [Z, Y, X]
    view = buf.permute(2, 1, 0)
    host = R.to_host(view)
    assert host.shape == (9, 7, 5) and host.flags.f_contiguous and host.dtype == np.uint16
    A = np.diag([0.7, 0.8, 1.6, 1.0])
    A[:3, 3] = (1.0, -2.0, 3.0)
    paths = [tmp_path / ("1_" + name), tmp_path / ("2_" + name)]
    for p in paths:
        N.write_nifti(str(p), host, A, compresslevel=1, mtime=0)
    arr, aff = N.read_nifti(str(paths[0]))
    assert arr.dtype == np.uint16 and np.array_equal(arr, view.numpy()) and np.allclose(aff, A)
    if name.endswith(".gz"):
        import gzip
        assert gzip.decompress(paths[0].read_bytes()) == gzip.decompress(paths[1].read_bytes())
        assert paths[0].read_bytes()[:10] == paths[1].read_bytes()[:10]     # mtime 0: the gzip header does not depend on the time
