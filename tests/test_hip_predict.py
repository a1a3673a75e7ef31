"""GPU tests of the prediction export (csrc/training.hip::miseg_label_export, training/predict.py, reference predict_whs.py): the kernel
against the device composition of existing pieces (torch.argmax, crop, miseg_resample3d nearest, flip / permute, LUT) on every orientation,
sampling, channel count and element width, the NaN rule, the index tables against their numpy restatement, the full MM-WHS size, the ABI
checks, and the command end to end on two synthetic volumes."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest
import torch

from test_predict_cpu import make_geom, remap_tensor, signed_permutation_affines, REF_MAP

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mods():
    from mi_seg_amd.data import nifti, preprocess
    from mi_seg_amd.hip import lib, ops
    from mi_seg_amd.training import predict
    return nifti, preprocess, ops, lib, predict


def tied_logits(cls, C, seed):
    """integer-valued logits [C, ...] whose torch.argmax (first maximum) is `cls`, with exact ties in later channels"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 3, (C,) + tuple(cls.shape), generator=g).float()
    idx = torch.arange(C).view((C,) + (1,) * cls.dim())
    tie = torch.randint(0, 2, x.shape, generator=g).bool() & (idx > cls[None])
    x = torch.where((idx == cls[None]) | tie, torch.full_like(x, 5.0), x)
    assert torch.equal(x.argmax(dim=0), cls)
    return x


def bits(t):
    """the same bytes as a signed integer tensor (comparisons of the unsigned 16 / 32-bit dtypes are not available on every backend)"""
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def composition(logits, geom, lut, dtype=torch.uint16):
    """the way back from existing device pieces: torch.argmax, crop, miseg_resample3d nearest on int32, flip / permute, LUT -> [X, Y, Z]"""
    _, P, _, _, _ = _mods()
    cls = logits.argmax(dim=0).to(torch.int32)
    cls = cls[tuple(slice(b, b + m) for b, m in zip(geom.pad_before, geom.resampled_shape))]
    cls = P.resample(cls[None], geom.ras_shape, "nearest")[0]
    flips = [k for k in range(3) if geom.flips[k]]
    if flips:
        cls = cls.flip(flips)
    cls = cls.permute(*np.argsort(geom.order).tolist())
    mask = (1 << (8 * torch.empty(0, dtype=dtype).element_size())) - 1
    signed = {torch.uint8: torch.uint8, torch.uint16: torch.int16, torch.uint32: torch.int32}[dtype]
    return (lut.to(cls.device).long() & mask)[cls.long()].to(signed).view(dtype)


def run_case(file_shape, order, flips, resampled, pb, pa, Cc, dtype, seed):
    _, _, _, _, R = _mods()
    g = make_geom(file_shape, order, flips, resampled, pb, pa)
    cls = torch.randint(0, Cc, g.padded_shape, generator=torch.Generator().manual_seed(seed))
    logits = tied_logits(cls, Cc, seed).to(DEV)
    lut = R.label_lut(Cc)
    got = R.invert_prediction(logits, g, lut, dtype=dtype)
    assert got.is_cuda and got.dtype == dtype and tuple(got.shape) == tuple(file_shape) and got.permute(2, 1, 0).is_contiguous()
    want = composition(logits, g, lut, dtype)
    assert same(got, want)
    return g, logits, lut, got


@pytest.mark.parametrize("i", range(48))
def test_kernel_equals_composition_every_orientation(i):
    N, _, _, _, _ = _mods()
    A = signed_permutation_affines()[i]
    order, flips = N.ras_orientation(A)
    file_shape = (23, 17, 11)
    ras = [file_shape[a] for a in order]
    run_case(file_shape, order, flips, (ras[0] // 2 + 1, ras[1], ras[2] * 2 - 3), (3, 0, 1), (2, 0, 0), 8, torch.uint16, i)


SAMPLING = [
    ((70, 9, 33), (0, 1, 2), (True, True, False), (40, 9, 50), (0, 4, 2), (0, 3, 1)),     # down / equal / up, pads
    ((5, 130, 66), (2, 0, 1), (False, True, False), (5, 65, 97), (0, 0, 0), (0, 0, 0)),    # no pad
    ((31, 29, 64), (1, 2, 0), (True, False, True), (31, 29, 64), (1, 1, 1), (1, 2, 3)),    # equal sampling, pad only
]


@pytest.mark.parametrize("case", range(len(SAMPLING)))
@pytest.mark.parametrize("Cc", [2, 8, 14])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16, torch.uint32])
def test_kernel_equals_composition_sampling_channels_widths(case, Cc, dtype):
    g, logits, lut, got = run_case(*SAMPLING[case], Cc, dtype, 100 * case + Cc)
    _, _, _, _, R = _mods()
    cpu = R.invert_prediction(logits.cpu(), g, lut, dtype=dtype)            # the CPU path of invert_prediction is the same map
    assert same(cpu, got.cpu())


def test_nan_rule():
    """the kernels' strict `>`: a NaN in channel 0 gives class 0, a NaN in a later channel never wins"""
    _, _, ops, _, R = _mods()
    g = make_geom((9, 10, 11), (0, 1, 2), (False, False, False), (9, 10, 11), (0, 0, 0), (0, 0, 0))
    x = torch.randn((5,) + g.padded_shape, generator=torch.Generator().manual_seed(3))
    x[torch.rand(x.shape, generator=torch.Generator().manual_seed(4)) < 0.2] = float("nan")
    nan = float("nan")
    x[:, 0, 0, 0] = torch.tensor([nan, 9.0, 1.0, 1.0, 1.0])
    x[:, 0, 0, 1] = torch.tensor([1.0, nan, 3.0, 3.0, 0.0])
    x[:, 0, 0, 2] = torch.tensor([1.0, 1.0, 1.0, 1.0, nan])
    got = R.invert_prediction(x.to(DEV), g, torch.arange(5, dtype=torch.int32), dtype=torch.uint8).cpu().long()
    assert got[0, 0, :3].tolist() == [0, 2, 0]
    assert torch.equal(got, ops.first_max_argmax(x))


def test_tables_device_equal_numpy():
    _, P, _, _, _ = _mods()
    rng = np.random.default_rng(7)
    pairs = {(int(a), int(b)) for a, b in rng.integers(1, 600, (2500, 2))}
    pairs |= {(m, n) for m in (1, 2, 3, 5, 9, 40, 65, 164, 180) for n in (1, 2, 3, 9, 11, 23, 29, 64, 130, 363, 512)}
    for c in SAMPLING:
        pairs |= {(m, c[0][a]) for m, a in zip(c[3], c[1])}
    for m, n in sorted(pairs):
        dev = P.resample(torch.arange(m, dtype=torch.int32, device=DEV).view(1, m, 1, 1), (n, 1, 1), "nearest").view(n).cpu().numpy()
        assert np.array_equal(dev, P.nearest_index(m, n)), (m, n)
    g = make_geom(*SAMPLING[0])
    dt, da = g.index_tables(DEV)
    ht, ha = g.index_tables()
    assert da == ha and all(torch.equal(a.cpu(), b) for a, b in zip(dt, ht))


def test_full_size():
    """512 x 512 x 363 from 180 x 180 x 164 logits (8 classes, a pad on one axis), LPS-like orientation"""
    _, _, _, _, R = _mods()
    torch.manual_seed(0)
    g = make_geom((512, 512, 363), (0, 1, 2), (True, True, False), (180, 180, 164), (0, 0, 2), (0, 0, 3))
    logits = torch.randn((8,) + g.padded_shape, device=DEV)
    lut = R.label_lut(8)
    got = R.invert_prediction(logits, g, lut)
    assert same(got, composition(logits, g, lut))


def test_abi_argument_checks():
    _, _, ops, L, R = _mods()
    so = L.load()
    logits = torch.zeros(4, 6, 7, 8, device=DEV)
    tabs = [torch.zeros(n, dtype=torch.int32, device=DEV) for n in (5, 6, 7)]
    lut = torch.arange(4, dtype=torch.int32, device=DEV)
    ws = torch.empty(1024, dtype=torch.uint8, device=DEV)
    out = torch.empty(7, 6, 5, dtype=torch.uint16, device=DEV)

    def params(**kw):
        base = dict(struct_size=C.sizeof(L.LabelExport), logits=logits.data_ptr(), C=4, D=6, H=7, W=8, box_d0=0, box_h0=0, box_w0=0, box_nd=1,
                    box_nh=1, box_nw=1, nx=5, ny=6, nz=7, axis_x=0, axis_y=1, axis_z=2, table_x=tabs[0].data_ptr(), table_y=tabs[1].data_ptr(),
                    table_z=tabs[2].data_ptr(), lut=lut.data_ptr(), workspace=ws.data_ptr(), out=out.data_ptr(), out_bytes=2)
        base.update(kw)
        return L.LabelExport(**base)

    def call(p):
        return so.miseg_label_export(C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    assert call(params()) == 0
    torch.cuda.synchronize()
    assert (bits(out) == 0).all()
    BAD = -1                                                               # MISEG_E_BADARG
    for kw in (dict(struct_size=8), dict(logits=0), dict(table_y=0), dict(lut=0), dict(workspace=0), dict(out=0), dict(C=0), dict(C=65),
               dict(out_bytes=3), dict(axis_z=1), dict(box_nw=9), dict(box_d0=6)):
        rc = call(params(**kw))
        assert rc == BAD, (kw, rc)
    assert so.miseg_label_export_workspace_bytes(3, 4, 5) >= 60
    g = make_geom((5, 6, 7), (0, 1, 2), (False, False, False), (6, 7, 8), (0, 0, 0), (0, 0, 0))
    tables, axes = g.index_tables(DEV)
    for bad in (-1, 6):
        t = [x.clone() for x in tables]
        t[0][2] = bad
        with pytest.raises(ValueError, match="outside"):
            ops.label_export(logits, t, axes, lut)
    with pytest.raises(ValueError, match="permutation"):
        ops.label_export(logits, tables, (0, 0, 2), lut)


def _write_qform_only(path, arr, b, c, d, offs, pix, qfac):
    """a NIfTI-1 file whose geometry is a qform alone (sform_code 0)"""
    N, _, _, _, _ = _mods()
    N.write_nifti(path, arr, np.diag(list(pix) + [1.0]))
    raw = bytearray(open(path, "rb").read())
    struct.pack_into("<f", raw, 76, qfac)
    struct.pack_into("<2h", raw, 252, 1, 0)
    struct.pack_into("<6f", raw, 256, b, c, d, *offs)
    open(path, "wb").write(bytes(raw))


MODEL_ARGS = ["--model_name", "swin_unetr", "--feature_size", "12", "--num_heads", "3", "--out_channels", "8", "--roi_x", "32", "--roi_y", "32",
              "--roi_z", "32", "--vit_norm_name", "instance_cond", "--encoder_norm_name", "instance_cond", "--decoder_norm_name", "instance",
              "--sw_batch_size", "2"]


def _host_reference(model, item, args, modality):
    """the way back from existing pieces on the host: sliding_window_inference, torch.argmax, numpy inverse, sequential remap"""
    _, P, _, _, _ = _mods()
    from mi_seg_amd.training.inferer import sliding_window_inference
    roi = (args.roi_x, args.roi_y, args.roi_z)
    image, g = P.load_image_for_prediction(item["image"], (args.space_x, args.space_y, args.space_z), roi, DEV)
    with torch.no_grad():
        logits = sliding_window_inference(image, roi, args.sw_batch_size, model, overlap=args.infer_overlap,
                                          modalities=torch.tensor([modality], device=DEV))
    cls = logits[0].argmax(0).cpu().numpy()
    cls = cls[tuple(slice(b, b + m) for b, m in zip(g.pad_before, g.resampled_shape))]
    for k in range(3):
        cls = np.take(cls, P.nearest_index(g.resampled_shape[k], g.ras_shape[k]), axis=k)
    for k in range(3):
        if g.flips[k]:
            cls = np.flip(cls, k)
    cls = np.transpose(cls, np.argsort(g.order))
    return remap_tensor(torch.from_numpy(np.ascontiguousarray(cls)), REF_MAP).numpy().astype(np.uint16)


def test_predict_end_to_end(tmp_path, capsys):
    N, P, _, _, R = _mods()
    from mi_seg_amd.data.checkpoint import export_state
    from mi_seg_amd.networks.utils.utils import model_from_argparse_args
    from mi_seg_amd.utils.detfill import fill_module_
    data = tmp_path / "data"
    (data / "imagesTs").mkdir(parents=True)
    rng = np.random.default_rng(11)
    ct = rng.normal(0, 300, (41, 37, 23)).astype(np.int16)
    A = np.array([[-0.7 * 0.98, 0.8 * 0.17, 0.0, 120.0], [-0.7 * 0.17, -0.8 * 0.98, 0.0, 95.5], [0.0, 0.0, 1.6, -210.0], [0, 0, 0, 1.0]])
    N.write_nifti(str(data / "imagesTs" / "ct_test_2001_image.nii.gz"), ct, A)
    mr = rng.normal(200, 50, (30, 27, 35)).astype(np.float32)
    _write_qform_only(str(data / "imagesTs" / "mr_test_2001_image.nii"), mr, 0.0, 0.0, 1.0, (10.0, -5.0, 3.0), (1.2, 1.1, 0.9), -1.0)
    for name, mod, img in (("CT_test.json", "CT", "imagesTs/ct_test_2001_image.nii.gz"), ("MR_test.json", "MR", "imagesTs/mr_test_2001_image.nii")):
        (data / name).write_text(json.dumps({"modality": {"0": mod}, "test": [{"image": img}]}))
    args = R.build_parser().parse_args(MODEL_ARGS)
    args.feature_size = args.feature_size[0]
    model = model_from_argparse_args(args)
    fill_module_(model)
    ck = str(tmp_path / "ck.pt")
    export_state(model, ck)
    model = model.to(DEV).eval()

    def run(out_dir, json_list):
        return R.main(MODEL_ARGS + ["--checkpoint", ck, "--data_dir", str(data), "--json_list", json_list, "--result_dir", str(out_dir)])

    outs = {}
    for json_list, mod in (("CT_test.json", 0), ("MR_test.json", 1)):
        paths = run(tmp_path / "r1", json_list)
        assert len(paths) == 1
        outs[mod] = paths[0]
        img_path = json.loads((data / json_list).read_text())["test"][0]["image"]
        assert paths[0] == str(tmp_path / "r1" / os.path.basename(img_path).replace("image", "label"))
        arr_in, aff_in = N.read_nifti(str(data / img_path))
        arr, aff = N.read_nifti(paths[0])
        assert arr.dtype == np.uint16 and arr.shape == arr_in.shape and np.allclose(aff, aff_in, atol=1e-5)
        a2 = args.__class__(**vars(args))
        a2.roi_x = a2.roi_y = a2.roi_z = 32
        a2.device = DEV
        want = _host_reference(model, {"image": str(data / img_path)}, a2, mod)
        assert np.array_equal(arr, want)
        assert set(np.unique(arr).tolist()) <= {0, 500, 600, 420, 550, 205, 820, 850}
        run(tmp_path / "r2", json_list)
        assert (tmp_path / "r1" / os.path.basename(paths[0])).read_bytes() == (tmp_path / "r2" / os.path.basename(paths[0])).read_bytes()
    printed = capsys.readouterr().out
    assert "inverse" in printed and "device-to-host" in printed and "ct_test_2001_label.nii.gz" in printed
    mr_path = str(data / "imagesTs" / "mr_test_2001_image.nii")
    as_ct = _host_reference(model, {"image": mr_path}, a2, 0)
    assert not np.array_equal(N.read_nifti(outs[1])[0], as_ct)              # the MR item ran with modality 1


def test_no_gpu_is_refused_with_a_device():
    _, _, _, _, R = _mods()
    with pytest.raises(SystemExit, match="HIP device only"):
        R.main(MODEL_ARGS + ["--no_gpu"])
