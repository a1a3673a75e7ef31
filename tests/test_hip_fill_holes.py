"""GPU tests of the fill-holes kernels (csrc/components.hip, miseg_fill_holes) against the CPU restatement
(training/postprocess.py::fill_holes_numpy) and the hand-built expectations of test_fill_holes_cpu.py.  Class maps are integers: every
comparison is exact.

The labelling works on tiles of 8 x 8 x 64 voxels (D x H x W) and every label's pass is confined to the label's bounding box grown by one voxel.
The shapes are the smallest that cross the tile on every axis (9 x 10 x 70, 17 x 9 x 130) or hold 3 x 3 x 3 tiles (19 x 21 x 150); the hand cases
run as they are and once more moved onto the corner (8, 8, 64) that eight tiles share, where their boxes are cut by tile borders on every axis."""
import ctypes as C

import numpy as np
import pytest
import torch

from components_common import large_batch, mods as _mods, snake
from test_fill_holes_cpu import SMALL, blob_map, hand_cases, noise_map

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG = (19, 21, 150)


def check(cls, Cc, applied=None, connectivity=3, min_filled=0):
    """the op on the class map(s) `cls` ([D, H, W] or [B, D, H, W]) in both element widths, with statistics, against the restatement, which
    has to fill at least `min_filled` voxels itself; returns the restatement's result"""
    ops, _, PP = _mods()
    cls = np.asarray(cls)
    vols = np.ascontiguousarray(cls[None] if cls.ndim == 3 else cls)
    want, wst = PP.fill_holes_numpy(vols, Cc, applied, connectivity, return_stats=True)
    assert wst.sum() == np.count_nonzero(want != vols) and wst.sum() >= min_filled, (int(wst.sum()), min_filled)
    small = vols.min() >= 0 and vols.max() <= 255
    for in_dt in ([torch.uint8] if small else []) + [torch.int32]:
        for out_dt in (torch.uint8, torch.int32):
            pred = torch.from_numpy(vols).to(in_dt).to(DEV)
            got, st = ops.fill_holes(pred=pred, num_classes=Cc, applied_labels=applied, connectivity=connectivity, out_dtype=out_dt, stats=True)
            assert got.dtype == out_dt and got.shape == vols.shape and got.is_cuda
            assert torch.equal(got.cpu(), torch.from_numpy(want).to(out_dt)), (in_dt, out_dt, connectivity)
            assert torch.equal(st.cpu(), torch.from_numpy(wst)), (in_dt, out_dt, connectivity)
            assert torch.equal(pred.cpu(), torch.from_numpy(vols).to(in_dt))              # the input is not touched
    return want[0] if cls.ndim == 3 else want


@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    name, cls, Cc, applied, conn, want = case
    assert np.array_equal(check(cls, Cc, applied, conn), want)
    if min(cls.shape) == 1:
        return
    # the same volume set into background with its voxel (4, 4, 4) on the tile corner (8, 8, 64); the faces of the small volume are no faces
    # any more, so the expectation is the restatement's (the cavity cases fill the same voxels: they never relied on a face)
    big = np.zeros((17, 17, 80), dtype=cls.dtype)
    big[4:4 + cls.shape[0], 4:4 + cls.shape[1], 60:60 + cls.shape[2]] = cls
    got = check(big, Cc, applied, conn)
    if "docstring" not in name and "out-of-range" not in name:
        assert np.array_equal(got[4:4 + cls.shape[0], 4:4 + cls.shape[1], 60:60 + cls.shape[2]], want)


def carved(order, open_end):
    """a solid block of label 1 with a one-voxel-wide serpentine cavity (gap 2: one voxel of wall between its lines) that starts one voxel
    inside the face d = 0; open_end: the start is cut through to that face"""
    cls = np.ones(BIG, dtype=np.int32)
    inner = tuple(s - 2 for s in BIG)
    path = np.zeros(BIG, dtype=bool)
    path[1:-1, 1:-1, 1:-1] = snake(inner, order, 2)
    cls[path] = 0
    if open_end:
        cls[0, 1, 1] = 0
    return cls, path


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0), (1, 2, 0)])
def test_serpentine_cavity(order):
    """one cavity that passes tile borders hundreds of times, lines along W, D or H: ending on a face nothing is filled, ending one voxel
    short of it all of it is - one missed union across a tile border flips the whole tail either way"""
    cls, path = carved(order, True)
    for conn in (1, 3):
        assert np.array_equal(check(cls, 2, None, conn), cls)
    cls, path = carved(order, False)
    assert path[1, 1, 1] and np.count_nonzero(path) > 5000
    for conn in (1, 3):
        assert (check(cls, 2, None, conn, min_filled=np.count_nonzero(path)) == 1).all()
    # the far end cut through instead: the opening is the LAST voxel of the component, its root the first
    far = np.argwhere(path)[-1]
    assert far[0] == BIG[0] - 2
    cls[far[0] + 1, far[1], far[2]] = 0
    assert np.array_equal(check(cls, 2, None, 1), cls)


def test_tile_corner_contact():
    """an open channel ending at (7, 7, 63) and a closed cavity starting across the corner that eight tiles share, then across a tile edge:
    the cavity leaks through the contact exactly when the neighbourhood has it"""
    base = np.ones((17, 17, 130), dtype=np.int32)
    base[7, 7, 0:64] = 0                                       # from the face w = 0 to the corner
    for other, leaks_from in (((8, 8), 3), ((8, 7), 2), ((7, 8), 2)):          # corner contact; edge contacts (the second with dw = +1 backward)
        cls = base.copy()
        cls[other[0], other[1], 64:70] = 0
        for conn in (1, 2, 3):
            got = check(cls, 2, None, conn)
            filled = np.count_nonzero(got != cls)
            assert filled == (0 if conn >= leaks_from else 6), (other, conn)
            assert (got[7, 7, 0:64] == 0).all()


@pytest.mark.parametrize("connectivity", [1, 2, 3])
@pytest.mark.parametrize("seed,shape,Cc", [(0, SMALL, 4), (1, (17, 9, 130), 8), (2, SMALL, 2)])
def test_random_blob_maps(connectivity, seed, shape, Cc):
    cls = blob_map(seed, shape, Cc)
    check(cls, Cc, None, connectivity, min_filled=1)
    check(cls, Cc, (Cc - 1,), connectivity)
    check(np.where(cls == 1, 77, cls), Cc, None, connectivity)                 # an out-of-range value in place of a label: passable, filled over


@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_percolation_noise(connectivity):
    """the complement of label 1 just above the percolation point of the neighbourhood: long winding open components, many closed ones"""
    check(noise_map(3, (17, 9, 130), connectivity), 3, (1,), connectivity, min_filled=1)
    check(noise_map(4, BIG, connectivity), 3, None, connectivity, min_filled=1)


def test_batch_of_two_fills_nothing_across_the_sample_end():
    ops, _, _ = _mods()
    cls = np.stack([blob_map(3, SMALL, 3), blob_map(4, SMALL, 3)])
    cls[0, -2:] = 1                                            # the end of sample 0 and the start of sample 1 are adjacent in memory:
    cls[1, :2] = 1                                             # solid label 1 on both sides, with background at the very end / start
    cls[0, -1, -1, -4:] = 0
    cls[1, 0, 0, :4] = 0
    got = check(cls, 3, None, 3, min_filled=1)
    assert (got[0, -1, -1, -4:] == 0).all() and (got[1, 0, 0, :4] == 0).all()
    for b in range(2):
        alone = ops.fill_holes(pred=torch.from_numpy(cls[b:b + 1]).to(DEV), num_classes=3)
        assert np.array_equal(alone.cpu().numpy()[0], got[b])


def large_batch_patterns():
    """8 class maps of 3 x 3 x 3 voxels with 3 classes: only the centre voxel can be a hole"""
    pats = np.zeros((8, 3, 3, 3), dtype=np.uint8)
    pats[0:2] = 1                          # solid label 1 with the centre 0: filled
    pats[0:2, 1, 1, 1] = 0
    pats[1, 1, 1, 0] = 0                   # the same with the hole cut through to the face w = 0: not filled
    pats[2] = 2                            # solid label 2 around a voxel of label 1: filled with 2
    pats[2, 1, 1, 1] = 1
    rng = np.random.default_rng(0)
    pats[3:] = rng.integers(0, 3, (5, 3, 3, 3))
    return pats


@pytest.mark.parametrize("out_dt", [torch.uint8, torch.int32], ids=["u8", "i32"])
def test_batch_above_the_grid_limit(out_dt):
    """65537 samples: more than a grid has rows, so every kernel's loop over the samples takes a second round; sample b is pattern b % 8 and the
    restatement runs on the 8 patterns only"""
    ops, _, PP = _mods()
    pats = large_batch_patterns()
    want, wst = PP.fill_holes_numpy(pats, 3, return_stats=True)
    changed = [k for k in range(8) if not np.array_equal(want[k], pats[k])]
    assert 2 <= len(changed) < 8, changed                              # some patterns are filled, some are left as they are
    assert want[0, 1, 1, 1] == 1 and np.array_equal(want[1], pats[1]) and want[2, 1, 1, 1] == 2 and wst[0, 1] == 1 and wst[2, 2] == 1
    k, vols = large_batch(pats)
    got, st = ops.fill_holes(pred=torch.from_numpy(vols).to(DEV), num_classes=3, out_dtype=out_dt, stats=True)
    assert got.dtype == out_dt and got.shape == vols.shape and st.shape == (len(k), 3)
    assert torch.equal(got.cpu(), torch.from_numpy(want[k]).to(out_dt))
    assert torch.equal(st.cpu(), torch.from_numpy(wst[k]))


def test_64_classes():
    cls = blob_map(5, SMALL, 64, salt=0.05)
    check(cls, 64, None, 1, min_filled=1)
    rng = np.random.default_rng(5)
    cls[rng.random(cls.shape) < 0.6] = 63
    check(cls, 64, (63,), 1, min_filled=1)
    check(cls, 64, None, 3)
    check(np.where(cls > 40, cls + 30, cls), 64, (5, 63), 2)                   # values of 71..93 are no class


def test_logits_against_class_map():
    """logits input = class-map input of their first-maximum argmax: exact ties in later channels, a NaN channel, NaN in channel 0"""
    ops, _, PP = _mods()
    from test_hip_predict import tied_logits
    Cc = 5
    cls = torch.from_numpy(np.stack([blob_map(6, SMALL, Cc), blob_map(7, SMALL, Cc)])).long()
    x = torch.stack([tied_logits(cls[b], Cc, b) for b in range(2)])
    x[0, 3] = float("nan")                                                # never wins: the argmax is that of the other channels
    cls[0] = ops.first_max_argmax(x[0])
    x[1, 0, 0, 0, :5] = float("nan")                                      # NaN in channel 0: class 0
    cls[1] = ops.first_max_argmax(x[1])
    assert (cls[1, 0, 0, :5] == 0).all() and (cls[0] != 3).all()
    want, wst = PP.fill_holes_numpy(cls.numpy(), Cc, None, 2, return_stats=True)
    assert wst.sum() > 0
    for dt in (torch.uint8, torch.int32):
        a, sa = ops.fill_holes(logits=x.to(DEV), connectivity=2, out_dtype=dt, stats=True)
        b, sb = ops.fill_holes(pred=cls.to(torch.uint8).to(DEV), num_classes=Cc, connectivity=2, out_dtype=dt, stats=True)
        assert torch.equal(a, b) and torch.equal(sa, sb) and np.array_equal(a.cpu().numpy(), want.astype(a.cpu().numpy().dtype))
        assert np.array_equal(sa.cpu().numpy(), wst)
    cpu = ops.fill_holes(logits=x, connectivity=2)                        # CPU tensors: the restatement
    assert not cpu.is_cuda and np.array_equal(cpu.numpy(), want.astype(np.uint8))


def _params(L, **kw):
    base = dict(struct_size=C.sizeof(L.FillHoles), logits=0, cls=0, cls_bytes=0, B=1, C=3, D=9, H=10, W=70, applied=6, connectivity=3, workspace=0, out=0,
                out_bytes=1, stats=0)
    base.update(kw)
    return L.FillHoles(**base)


def test_out_may_alias_cls():
    _, L, PP = _mods()
    so = L.load()
    cls = blob_map(11, SMALL, 3)
    want = PP.fill_holes_numpy(cls, 3)
    assert not np.array_equal(want, cls)
    ws = torch.empty(so.miseg_fill_holes_workspace_bytes(1, *SMALL), dtype=torch.uint8, device=DEV)
    for dt, nb in ((torch.uint8, 1), (torch.int32, 4)):
        buf = torch.from_numpy(cls).to(dt).to(DEV)
        p = _params(L, cls=buf.data_ptr(), cls_bytes=nb, out=buf.data_ptr(), out_bytes=nb, workspace=ws.data_ptr())
        assert so.miseg_fill_holes(C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        assert np.array_equal(buf.cpu().numpy(), want.astype(buf.cpu().numpy().dtype))


def test_reproducible_and_graph_capturable():
    ops, _, _ = _mods()
    make = lambda seed: torch.from_numpy(noise_map(seed, BIG, 1) + blob_map(seed, BIG, 2))[None].to(torch.uint8).to(DEV)      # values 0..3
    cls = make(4)
    run = lambda: ops.fill_holes(pred=cls, num_classes=4, connectivity=1, out_dtype=torch.int32, stats=True)
    a, sa = run()
    b, sb = run()
    assert torch.equal(a, b) and torch.equal(sa, sb) and int(sa.sum()) > 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c, sc = run()
    c.zero_()
    sc.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(a, c) and torch.equal(sa, sc)
    cls.copy_(make(5))                                                     # a replay reads the input anew
    g.replay()
    torch.cuda.synchronize()
    d, sd = run()
    assert torch.equal(c, d) and torch.equal(sc, sd) and not torch.equal(c, a)


def test_abi_rejects_bad_arguments():
    """every rejected call fails on the host, with a message, before any launch: the output buffer keeps its bytes"""
    ops, L, _ = _mods()
    so = L.load()
    assert so.miseg_abi_version() == 16 and L.ABI_VERSION == 16
    assert so.miseg_abi_struct_size(b"miseg_fill_holes_params") == C.sizeof(L.FillHoles)
    cls = torch.ones(*SMALL, dtype=torch.uint8, device=DEV)
    logits = torch.zeros(1, 3, *SMALL, device=DEV)
    out = torch.full(SMALL, 77, dtype=torch.uint8, device=DEV)
    nbytes = so.miseg_fill_holes_workspace_bytes(1, *SMALL)
    assert nbytes >= 5 * 6300 + 64 * 6 * 4 and nbytes <= 5 * 6300 + 64 * 6 * 4 + 1024
    assert so.miseg_fill_holes_workspace_bytes(0, *SMALL) == 0 and so.miseg_fill_holes_workspace_bytes(1, 9, 0, 70) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    good = dict(cls=cls.data_ptr(), cls_bytes=1, out=out.data_ptr(), workspace=ws.data_ptr())
    call = lambda p: so.miseg_fill_holes(C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    bad = [dict(struct_size=8), dict(logits=logits.data_ptr()), dict(cls=0), dict(cls_bytes=2), dict(C=0), dict(C=65), dict(connectivity=0), dict(connectivity=4),
           dict(out=0), dict(workspace=0), dict(out_bytes=2), dict(B=0), dict(D=0), dict(W=65536)]
    for kw in bad:
        rc = call(_params(L, **{**good, **kw}))
        assert rc == -1 and so.miseg_last_error(), kw
    assert b"struct_size" in (call(_params(L, **{**good, "struct_size": 8})), so.miseg_last_error())[1]
    assert call(_params(L, **{**good, "D": 65535, "H": 65535, "W": 1})) == -2          # 2^31 voxels and more: unsupported
    torch.cuda.synchronize()
    assert (out == 77).all()
    assert call(_params(L, **good)) == 0
    torch.cuda.synchronize()
    assert (out == 1).all()
    with pytest.raises(ValueError, match="exactly one"):
        ops.fill_holes(logits=logits, pred=cls[None], num_classes=3)
    with pytest.raises(ValueError, match="applied label"):
        ops.fill_holes(pred=cls[None], num_classes=3, applied_labels=(3,))
    with pytest.raises(ValueError, match="num_classes"):
        ops.fill_holes(pred=cls[None])
    with pytest.raises(ValueError, match="out_dtype"):
        ops.fill_holes(pred=cls[None], num_classes=3, out_dtype=torch.int64)


def test_transform_on_the_device():
    """the transform's class-map and one-hot forms on device tensors (the one-hot channels as batch entries of two classes) equal the CPU forms"""
    _, _, PP = _mods()
    Cc = 4
    cls = blob_map(21, SMALL, Cc)
    onehot = torch.nn.functional.one_hot(torch.from_numpy(cls).long(), Cc).movedim(-1, 0).float()
    single = torch.from_numpy(cls)[None].float()
    single[0, 0, 0, :3] = torch.tensor([0.5, 64.0, 99.0])
    for applied in (None, (1, 3)):
        t = PP.FillHoles(applied_labels=applied, connectivity=2)
        for x in (single, onehot):
            got, want = t(x.to(DEV)), t(x)
            assert got.is_cuda and torch.equal(got.cpu(), want) and not torch.equal(want, x)


def test_predict_with_keep_largest_and_fill_holes(tmp_path, capsys):
    """the command with --keep_largest --fill_holes, and with --fill_holes alone, on a tiny synthetic model: the written file is the CPU
    pipeline applied to the same logits, and without the flags the file is the plain export"""
    ops, _, _ = _mods()
    from mi_seg_amd.data import nifti as N
    from mi_seg_amd.data import preprocess as P
    from mi_seg_amd.data.checkpoint import export_state
    from mi_seg_amd.networks.utils.utils import model_from_argparse_args
    from mi_seg_amd.training import predict as R
    from mi_seg_amd.training.inferer import sliding_window_inference
    from mi_seg_amd.utils.detfill import fill_module_
    from test_hip_predict import MODEL_ARGS
    import json
    data = tmp_path / "data"
    (data / "imagesTs").mkdir(parents=True)
    ct = np.random.default_rng(11).normal(0, 300, (41, 37, 23)).astype(np.int16)
    A = np.array([[-0.7 * 0.98, 0.8 * 0.17, 0.0, 120.0], [-0.7 * 0.17, -0.8 * 0.98, 0.0, 95.5], [0.0, 0.0, 1.6, -210.0], [0, 0, 0, 1.0]])
    image = str(data / "imagesTs" / "ct_test_2001_image.nii.gz")
    N.write_nifti(image, ct, A)
    (data / "CT_test.json").write_text(json.dumps({"modality": {"0": "CT"}, "test": [{"image": "imagesTs/ct_test_2001_image.nii.gz"}]}))
    args = R.build_parser().parse_args(MODEL_ARGS)
    args.feature_size = args.feature_size[0]
    model = model_from_argparse_args(args)
    fill_module_(model)
    ck = str(tmp_path / "ck.pt")
    export_state(model, ck)
    model = model.to(DEV).eval()
    common = MODEL_ARGS + ["--checkpoint", ck, "--data_dir", str(data), "--json_list", "CT_test.json"]
    plain = R.main(common + ["--result_dir", str(tmp_path / "plain")])
    assert "fill-holes" not in capsys.readouterr().out
    roi = (32, 32, 32)
    vol, g = P.load_image_for_prediction(image, (1.0, 1.0, 1.0), roi, DEV)
    with torch.no_grad():
        logits = sliding_window_inference(vol, roi, args.sw_batch_size, model, overlap=args.infer_overlap, modalities=torch.tensor([0], device=DEV)).cpu()
    lut = R.label_lut(8)
    assert np.array_equal(N.read_nifti(plain[0])[0], R.invert_prediction(logits, g, lut).numpy())
    runs = ((["--keep_largest", "--fill_holes"], True, {}),
            (["--fill_holes", "--fill_holes_connectivity", "1", "--fill_holes_labels", "1", "2", "5"], False, dict(applied_labels=(1, 2, 5), connectivity=1)))
    for extra, keep, kw in runs:
        paths = R.main(common + ["--result_dir", str(tmp_path / "fh")] + extra)
        printed = capsys.readouterr().out
        assert "fill-holes" in printed and ("keep-largest" in printed) == keep
        if keep:
            assert printed.index("keep-largest") < printed.index("fill-holes")
            cls = ops.fill_holes(pred=ops.keep_largest_component(logits=logits), num_classes=8, **kw)          # CPU tensors: the restatements
        else:
            cls = ops.fill_holes(logits=logits, **kw)
        want = R.invert_prediction(None, g, lut, pred=cls[0]).numpy()
        arr, _ = N.read_nifti(paths[0])
        assert arr.dtype == np.uint16 and np.array_equal(arr, want)


def test_evaluate_on_the_device_equals_cpu():
    """evaluate.test(fill_holes=), alone and after keep_largest, on device logits (fused: one filtered map feeds every metric) against the same
    call on the replayed CPU logits (the one-hot chain with the transforms inside)"""
    _, _, PP = _mods()
    from mi_seg_amd.training import evaluate as E
    from mi_seg_amd.training import metrics as M
    from test_surface_distance_cpu import same
    Cc = 4
    model = torch.nn.Conv3d(1, Cc, 3, padding=1)
    with torch.no_grad():
        model.weight.copy_(torch.randn(model.weight.shape, generator=torch.Generator().manual_seed(0)))
        model.bias.copy_(torch.tensor([0.8, 0.0, -0.2, -0.4]))
    model = model.to(DEV)
    loader = []
    for i in range(2):
        gen = torch.Generator().manual_seed(10 + i)
        loader.append({"image": torch.randn(2, 1, 12, 13, 70, generator=gen), "label": torch.randint(0, Cc, (2, 1, 12, 13, 70), generator=gen).float(),
                       "modality": torch.tensor([i % 2, (i + 1) % 2])})
    seen = []

    def on_device(x, modalities=None):
        seen.append(model(x).detach())
        return seen[-1]

    def run(device, inferer, **kw):
        res = {}
        ret = E.test(model, loader, device, M.DiceMetric(include_background=True, reduction="mean_batch", get_not_nans=True), E.AsDiscrete(to_onehot=Cc),
                     E.AsDiscrete(argmax=True, to_onehot=Cc), model_inferer=inferer, amp=False,
                     surface_distance=M.SurfaceDistanceMetric(include_background=True, symmetric=True, reduction="mean_batch", get_not_nans=True),
                     additional_metrics=[M.GeneralizedDiceScore(include_background=False)], results=res, **kw)
        return ret, res

    fh = PP.FillHoles(connectivity=1)
    for kw in (dict(fill_holes=fh), dict(keep_largest=PP.KeepLargestConnectedComponent(connectivity=3), fill_holes=fh)):
        seen.clear()
        ret_dev, res_dev = run(DEV, on_device, **kw)
        replay = iter([s.cpu() for s in seen])
        ret_cpu, res_cpu = run("cpu", lambda x, modalities=None: next(replay), **kw)
        assert res_dev.keys() == res_cpu.keys()
        for part in res_dev:
            if part == "additional_metrics":
                assert res_dev[part] == pytest.approx(res_cpu[part], rel=1e-6)
            elif part.startswith("dice"):
                # per sample the values are equal to the bit (checked below); these are fp32 means over the batch, summed in the device's order
                # and in the host's: a few ulp of fp32 apart at most, the bar of the keep-largest end-to-end test
                assert list(res_dev[part].values()) == pytest.approx(list(res_cpu[part].values()), rel=1e-6), part
            else:
                assert res_dev[part].keys() == res_cpu[part].keys()
                same(list(res_dev[part].values()), list(res_cpu[part].values()), rel=1e-9)
        assert ret_dev[0] == pytest.approx(ret_cpu[0], rel=1e-6)
        same([ret_dev[1]], [ret_cpu[1]], rel=1e-9)
        filters = [kw[k] for k in ("keep_largest", "fill_holes") if k in kw]
        changed = 0
        for logits, batch in zip(seen, loader):              # per sample: integer counts through the same float arithmetic, equal to the bit
            pred = before = filters[0].class_map(logits=logits, out_dtype=torch.int32)
            for f in filters[1:]:
                pred = f.class_map(pred=pred, num_classes=Cc, out_dtype=torch.int32)
            chain = []
            for x in logits.cpu():
                t = E.AsDiscrete(argmax=True)(x)
                for f in filters:
                    t = f(t)
                chain.append(E.AsDiscrete(to_onehot=Cc)(t))
            chain = torch.stack(chain)
            label = torch.stack([E.AsDiscrete(to_onehot=Cc)(y) for y in batch["label"]])
            assert torch.equal(pred.cpu(), chain.argmax(1).int())
            assert torch.equal(M.dice_from_class_map(pred, batch["label"], Cc).cpu(), M.dice_metric(chain, label))
            changed += int((pred != (before if len(filters) > 1 else logits.argmax(1))).sum())
        assert changed > 0                                   # the fill-holes stage itself changes these maps
    replay = iter([s.cpu() for s in seen])
    assert run("cpu", lambda x, modalities=None: next(replay))[1] != res_cpu          # the filters change these noisy maps' metrics
