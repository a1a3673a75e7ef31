"""GPU tests of the keep-largest-connected-component kernels (csrc/components.hip, miseg_keep_largest) against the CPU
restatement (training/postprocess.py::keep_largest_numpy) and, on the tiny shapes, the brute-force flood fill of test_keep_largest_cpu.py.
Class maps are integers: every comparison is exact.

The labelling works on tiles of 8 x 8 x 64 voxels (D x H x W): union-find inside a tile in LDS, unions across tile borders on the parent volume.
The shapes below are the smallest that reach every part: single voxels and slabs thinner than a tile; 19 x 21 x 150 - odd, no side a multiple of
the tile, more than two tiles (3 x 3 x 3) on every axis; contacts exactly at the tile corner (7,7,63)-(8,8,64)."""
import ctypes as C

import numpy as np
import pytest
import torch

from components_common import large_batch, mods as _mods, snake
from test_keep_largest_cpu import oracle, random_map

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG = (19, 21, 150)


def check(cls, Cc, applied=None, independent=True, connectivity=3, brute=False):
    """the op on the class map(s) `cls` ([D, H, W] or [B, D, H, W]) in both element widths, with statistics, against the restatement"""
    ops, _, PP = _mods()
    cls = np.asarray(cls)
    vols = cls[None] if cls.ndim == 3 else cls
    want, wst = PP.keep_largest_numpy(vols, Cc, applied, independent, connectivity, return_stats=True)
    if brute:
        for b in range(vols.shape[0]):
            o, st = oracle(vols[b], Cc, applied, independent, connectivity, stats=True)
            assert np.array_equal(o, want[b]) and np.array_equal(st, wst[b])
    small = vols.min() >= 0 and vols.max() <= 255
    for in_dt in ([torch.uint8] if small else []) + [torch.int32]:
        for out_dt in (torch.uint8, torch.int32):
            pred = torch.from_numpy(vols).to(in_dt).to(DEV)
            got, st = ops.keep_largest_component(pred=pred, num_classes=Cc, applied_labels=applied, independent=independent, connectivity=connectivity,
                                                 out_dtype=out_dt, stats=True)
            assert got.dtype == out_dt and got.shape == vols.shape and got.is_cuda
            assert torch.equal(got.cpu(), torch.from_numpy(want).to(out_dt)), (in_dt, out_dt, independent, connectivity)
            assert torch.equal(st.cpu(), torch.from_numpy(wst)), (in_dt, out_dt, independent, connectivity)
            assert torch.equal(pred.cpu(), torch.from_numpy(vols).to(in_dt))              # the input is not touched
    return want[0] if cls.ndim == 3 else want


def test_single_voxels_and_slabs():
    """1 x 1 x 1, 1 x H x W and D x 1 x 1: thinner than a tile on two axes, longer on the third (H = 9 and D = 17 pass tile borders, W = 70 too)"""
    for v in (0, 1):
        assert check(np.full((1, 1, 1), v, dtype=np.int32), 2, brute=True)[0, 0, 0] == v
    for shape, p in (((1, 9, 70), 0.45), ((17, 1, 1), 0.6), ((1, 1, 131), 0.7), ((9, 1, 70), 0.45)):
        for conn in (1, 2, 3):
            for independent in (True, False):
                check(random_map(conn, shape, 3, p), 3, None, independent, conn, brute=True)


@pytest.mark.parametrize("order,gap", [((0, 1, 2), 2), ((2, 1, 0), 2), ((1, 2, 0), 4), ((0, 1, 2), 4)])
def test_serpentine_crosses_every_tile_border(order, gap):
    """the long-chain case of the merge loop and the flatten: one component that passes tile borders hundreds of times, lines along W, D or H;
    with a gap of 4 there is room between the lines for islands of the same class that touch the path nowhere"""
    m = snake(BIG, order, gap)
    cls = np.where(m, 2, 0).astype(np.int32)
    rng = np.random.default_rng(1)
    pad = np.pad(m, 1)
    free = ~np.any([pad[1 + a:1 + a + BIG[0], 1 + b:1 + b + BIG[1], 1 + c:1 + c + BIG[2]] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], axis=0)
    cls[free & (rng.random(BIG) < 0.06)] = 2                               # (below every neighbourhood's percolation point: small islands)
    cls[free & (cls == 0) & (rng.random(BIG) < 0.3)] = 1
    for conn in (1, 3):
        got = check(cls, 3, None, True, conn)
        assert (got[m] == 2).all() and np.count_nonzero(got == 2) == np.count_nonzero(m)      # one component, the largest: the whole path
    assert gap == 2 or np.count_nonzero(cls == 2) > np.count_nonzero(m) + 100
    got = check(cls, 3, (2,), False, 1)
    assert np.count_nonzero(got == 2) == np.count_nonzero(m) and np.array_equal(got == 1, cls == 1)


def test_tile_corner_contact():
    """voxels (7,7,63) and (8,8,64) meet only at the corner shared by eight tiles: one component under connectivity 3, two under 1 and 2"""
    cls = np.zeros(BIG, dtype=np.int32)
    cls[7, 7, 61:64] = 1                   # 3 voxels ending at the corner
    cls[8, 8, 64:66] = 1                   # 2 voxels starting across it
    cls[15, 3, 100:104] = 1                # 4 voxels elsewhere
    got = check(cls, 2, None, True, 3)
    assert got.sum() == 5 and got[15, 3, 100:104].sum() == 0
    for conn in (1, 2):
        got = check(cls, 2, None, True, conn)
        assert got.sum() == 4 and got[15, 3, 100:104].sum() == 4
    # an edge contact across a tile edge, (7,7,63)-(8,7,64): connectivity 2 joins it, 1 does not
    cls[8, 8, 64:66] = 0
    cls[8, 7, 64:66] = 1
    assert check(cls, 2, None, True, 2).sum() == 5 and check(cls, 2, None, True, 1).sum() == 4
    # (7,7,63)-(7,8,64): a backward neighbour with dw = +1 across the W border
    cls[8, 7, 64:66] = 0
    cls[7, 8, 64:66] = 1
    assert check(cls, 2, None, True, 2).sum() == 5 and check(cls, 2, None, True, 1).sum() == 4


@pytest.mark.parametrize("connectivity,p", [(1, 0.31), (2, 0.14), (3, 0.10)])
@pytest.mark.parametrize("independent", [True, False])
def test_percolation_noise(connectivity, p, independent):
    """foreground near the percolation point of each neighbourhood over 4 classes: thousands of components, many of equal size"""
    q = p if not independent else min(3 * p, 0.9)            # independent: each of the 3 foreground classes near the point on its own
    cls = random_map(7 + connectivity, BIG, 4, q)
    check(cls, 4, None, independent, connectivity)
    check(cls, 4, (1, 3), independent, connectivity)
    check(cls, 4, (0, 2), independent, connectivity)


def test_batch_of_two_connects_nothing_across_samples():
    cls = np.stack([random_map(1, (9, 10, 70), 3, 0.3), random_map(2, (9, 10, 70), 3, 0.5)])
    cls[0, -1, -1, -4:] = 1                # the end of sample 0 and the start of sample 1 are adjacent in memory
    cls[1, 0, 0, :4] = 1
    for independent in (True, False):
        got = check(cls, 3, None, independent, 3)
        ops, _, _ = _mods()
        for b in range(2):
            alone = ops.keep_largest_component(pred=torch.from_numpy(cls[b:b + 1]).to(DEV), num_classes=3, independent=independent)
            assert np.array_equal(alone.cpu().numpy()[0], got[b])


def large_batch_patterns():
    """8 class maps of 3 x 3 x 3 voxels with 3 classes"""
    pats = np.zeros((8, 3, 3, 3), dtype=np.uint8)
    pats[0, 0, 0, 0:2] = 1                 # two components of class 1, of 2 and of 3 voxels: the first goes
    pats[0, 2, 2, :] = 1
    pats[1, 0, 0, 0:2] = 1                 # two of 2 voxels each: the one holding linear index 0 stays
    pats[1, 2, 2, 1:3] = 1
    for k in range(2, 8):
        pats[k] = random_map(k, (3, 3, 3), 3, 0.5)
    return pats


@pytest.mark.parametrize("out_dt", [torch.uint8, torch.int32], ids=["u8", "i32"])
def test_batch_above_the_grid_limit(out_dt):
    """65537 samples: more than a grid has rows, so every kernel's loop over the samples takes a second round; sample b is pattern b % 8 and the
    restatement runs on the 8 patterns only"""
    ops, _, PP = _mods()
    pats = large_batch_patterns()
    want, wst = PP.keep_largest_numpy(pats, 3, return_stats=True)
    changed = [k for k in range(8) if not np.array_equal(want[k], pats[k])]
    assert 2 <= len(changed) < 8, changed                              # some patterns lose voxels, some are left as they are
    assert (want[0, 2, 2] == 1).all() and want[0].sum() == 3 and (want[1, 0, 0, 0:2] == 1).all() and want[1].sum() == 2
    k, vols = large_batch(pats)
    got, st = ops.keep_largest_component(pred=torch.from_numpy(vols).to(DEV), num_classes=3, out_dtype=out_dt, stats=True)
    assert got.dtype == out_dt and got.shape == vols.shape and st.shape == (len(k), 3, 3)
    assert torch.equal(got.cpu(), torch.from_numpy(want[k]).to(out_dt))
    assert torch.equal(st.cpu(), torch.from_numpy(wst[k]))


def test_64_classes():
    rng = np.random.default_rng(5)
    cls = rng.integers(0, 64, (9, 10, 70)).astype(np.int32)
    cls[rng.random(cls.shape) < 0.5] = 63
    got = check(cls, 64, (63,), True, 1)
    assert np.array_equal(got != 63, (cls != 63) | (got == 0)) and np.count_nonzero(got == 63) < np.count_nonzero(cls == 63)
    check(cls, 64, None, True, 1)
    check(cls, 64, None, False, 1)
    check(np.where(cls > 40, cls + 30, cls), 64, (63, 5), True, 2)          # values of 71..93 are no class: copied through


def test_logits_against_class_map():
    """logits input = class-map input of their first-maximum argmax: exact ties in later channels, a NaN channel, NaN in channel 0"""
    ops, _, PP = _mods()
    from test_hip_predict import tied_logits
    Cc = 5
    cls = torch.from_numpy(random_map(3, (2, 9, 10, 70), Cc, 0.45)).long()
    x = torch.stack([tied_logits(cls[b], Cc, b) for b in range(2)])
    x[0, 3] = float("nan")                                                # never wins: the argmax is that of the other channels
    cls[0] = ops.first_max_argmax(x[0])
    x[1, 0, 0, 0, :5] = float("nan")                                      # NaN in channel 0: class 0
    cls[1] = ops.first_max_argmax(x[1])
    assert (cls[1, 0, 0, :5] == 0).all() and (cls[0] != 3).all()
    for independent in (True, False):
        want = PP.keep_largest_numpy(cls.numpy(), Cc, None, independent, 2)
        for dt in (torch.uint8, torch.int32):
            a, sa = ops.keep_largest_component(logits=x.to(DEV), independent=independent, connectivity=2, out_dtype=dt, stats=True)
            b, sb = ops.keep_largest_component(pred=cls.to(torch.uint8).to(DEV), num_classes=Cc, independent=independent, connectivity=2, out_dtype=dt, stats=True)
            assert torch.equal(a, b) and torch.equal(sa, sb) and np.array_equal(a.cpu().numpy(), want.astype(a.cpu().numpy().dtype))
    cpu = ops.keep_largest_component(logits=x, independent=False, connectivity=2)           # CPU tensors: the restatement
    assert not cpu.is_cuda and np.array_equal(cpu.numpy(), want.astype(np.uint8))


def _params(L, **kw):
    base = dict(struct_size=C.sizeof(L.KeepLargest), logits=0, cls=0, cls_bytes=0, B=1, C=3, D=9, H=10, W=70, applied=6, independent=1, connectivity=3,
                workspace=0, out=0, out_bytes=1, stats=0)
    base.update(kw)
    return L.KeepLargest(**base)


def test_out_may_alias_cls():
    _, L, PP = _mods()
    so = L.load()
    cls = random_map(11, (9, 10, 70), 3, 0.4)
    want = PP.keep_largest_numpy(cls, 3)
    ws = torch.empty(so.miseg_keep_largest_workspace_bytes(1, 9, 10, 70), dtype=torch.uint8, device=DEV)
    for dt, nb in ((torch.uint8, 1), (torch.int32, 4)):
        buf = torch.from_numpy(cls).to(dt).to(DEV)
        p = _params(L, cls=buf.data_ptr(), cls_bytes=nb, out=buf.data_ptr(), out_bytes=nb, workspace=ws.data_ptr())
        assert so.miseg_keep_largest(C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        assert np.array_equal(buf.cpu().numpy(), want.astype(buf.cpu().numpy().dtype))


def test_reproducible_and_graph_capturable():
    ops, _, _ = _mods()
    cls = torch.from_numpy(random_map(4, BIG, 4, 0.3)[None]).to(torch.uint8).to(DEV)
    run = lambda: ops.keep_largest_component(pred=cls, num_classes=4, connectivity=1, out_dtype=torch.int32, stats=True)
    a, sa = run()
    b, sb = run()
    assert torch.equal(a, b) and torch.equal(sa, sb)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c, sc = run()
    c.zero_()
    sc.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(a, c) and torch.equal(sa, sc)
    cls.copy_(torch.from_numpy(random_map(5, BIG, 4, 0.3)[None]).to(torch.uint8))          # a replay reads the input anew
    g.replay()
    torch.cuda.synchronize()
    d, sd = run()
    assert torch.equal(c, d) and torch.equal(sc, sd) and not torch.equal(c, a)


def test_abi_rejects_bad_arguments():
    """every rejected call fails on the host, with a message, before any launch: the output buffer keeps its bytes"""
    ops, L, _ = _mods()
    so = L.load()
    assert so.miseg_abi_version() == 16 and L.ABI_VERSION == 16
    cls = torch.ones(9, 10, 70, dtype=torch.uint8, device=DEV)
    logits = torch.zeros(1, 3, 9, 10, 70, device=DEV)
    out = torch.full((9, 10, 70), 77, dtype=torch.uint8, device=DEV)
    nbytes = so.miseg_keep_largest_workspace_bytes(1, 9, 10, 70)
    assert nbytes >= 9 * 6300 + 64 * 8 and nbytes <= 9 * 6300 + 4096
    assert so.miseg_keep_largest_workspace_bytes(0, 9, 10, 70) == 0 and so.miseg_keep_largest_workspace_bytes(1, 9, 0, 70) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    good = dict(cls=cls.data_ptr(), cls_bytes=1, out=out.data_ptr(), workspace=ws.data_ptr())
    call = lambda p: so.miseg_keep_largest(C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream))
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
        ops.keep_largest_component(logits=logits, pred=cls[None], num_classes=3)
    with pytest.raises(ValueError, match="applied label"):
        ops.keep_largest_component(pred=cls[None], num_classes=3, applied_labels=(3,))
    with pytest.raises(ValueError, match="num_classes"):
        ops.keep_largest_component(pred=cls[None])
    with pytest.raises(ValueError, match="out_dtype"):
        ops.keep_largest_component(pred=cls[None], num_classes=3, out_dtype=torch.int64)


def test_transform_on_the_device():
    """the transform's class-map and one-hot forms on device tensors (the one-hot channels as batch entries of two classes) equal the CPU forms"""
    _, _, PP = _mods()
    Cc = 4
    cls = random_map(21, (9, 10, 70), Cc, 0.35)
    onehot = torch.nn.functional.one_hot(torch.from_numpy(cls).long(), Cc).movedim(-1, 0).float()
    for independent in (True, False):
        for applied in (None, (1, 3)):
            t = PP.KeepLargestConnectedComponent(applied_labels=applied, independent=independent, connectivity=2)
            single = torch.from_numpy(cls)[None].float()
            for x in (single, onehot):
                got = t(x.to(DEV))
                assert got.is_cuda and torch.equal(got.cpu(), t(x))


def test_label_export_of_a_class_map():
    """label_export(pred=map) = label_export(logits) when the map is the logits' argmax, for both map widths, every output width, a box smaller
    than the volume; a value outside the classes is written as 0"""
    ops, _, _ = _mods()
    from mi_seg_amd.training import predict as R
    from test_hip_predict import same, tied_logits
    from test_predict_cpu import make_geom
    for case, (file_shape, order, flips, resampled, pb, pa) in enumerate([((70, 9, 33), (0, 1, 2), (True, True, False), (40, 9, 50), (0, 4, 2), (0, 3, 1)),
                                                                          ((5, 130, 66), (2, 0, 1), (False, True, False), (5, 65, 97), (0, 0, 0), (0, 0, 0))]):
        g = make_geom(file_shape, order, flips, resampled, pb, pa)
        cls = torch.randint(0, 8, g.padded_shape, generator=torch.Generator().manual_seed(case))
        logits = tied_logits(cls, 8, case).to(DEV)
        lut = R.label_lut(8)
        for dtype in (torch.uint8, torch.uint16, torch.uint32):
            want = R.invert_prediction(logits, g, lut, dtype=dtype)
            for mdt in (torch.uint8, torch.int32):
                got = R.invert_prediction(None, g, lut, dtype=dtype, pred=cls.to(mdt).to(DEV))
                assert same(got, want)
                assert same(R.invert_prediction(None, g, lut, dtype=dtype, pred=cls.to(mdt)), want.cpu())
        odd = cls.to(torch.int32)
        odd[cls == 3] = -5
        odd[cls == 4] = 200
        want = R.invert_prediction(None, g, lut, pred=odd)
        assert same(R.invert_prediction(None, g, lut, pred=odd.to(DEV)).cpu(), want)
        known = R.invert_prediction(logits, g, lut).cpu().view(torch.int16)
        assert torch.equal(want.view(torch.int16), torch.where((known == lut[3]) | (known == lut[4]), torch.zeros_like(known), known))


def test_predict_with_keep_largest(tmp_path, capsys):
    """the command with --keep_largest on a tiny synthetic model: the written file is the CPU restatement applied to the same logits, and
    without the flag the file is the one the command wrote before"""
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
    assert "keep-largest" not in capsys.readouterr().out
    roi = (32, 32, 32)
    vol, g = P.load_image_for_prediction(image, (1.0, 1.0, 1.0), roi, DEV)
    with torch.no_grad():
        logits = sliding_window_inference(vol, roi, args.sw_batch_size, model, overlap=args.infer_overlap, modalities=torch.tensor([0], device=DEV)).cpu()
    lut = R.label_lut(8)
    assert np.array_equal(N.read_nifti(plain[0])[0], R.invert_prediction(logits, g, lut).numpy())
    for extra, kw in ((["--keep_largest"], {}), (["--keep_largest", "--keep_largest_joint", "--keep_largest_connectivity", "1", "--keep_largest_labels", "1", "2", "5"],
                                                  dict(applied_labels=(1, 2, 5), independent=False, connectivity=1))):
        paths = R.main(common + ["--result_dir", str(tmp_path / "kl")] + extra)
        assert "keep-largest" in capsys.readouterr().out
        cls = ops.keep_largest_component(logits=logits, **kw)                      # CPU tensors: keep_largest_numpy
        want = R.invert_prediction(None, g, lut, pred=cls[0]).numpy()
        arr, _ = N.read_nifti(paths[0])
        assert arr.dtype == np.uint16 and np.array_equal(arr, want)


def test_evaluate_on_the_device_equals_cpu():
    """evaluate.test(keep_largest=) on device logits (fused: one filtered map feeds Dice, generalized Dice, ASD and HD) against the same call
    on the replayed CPU logits (the one-hot chain with the transform inside)"""
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
    for i in range(3):
        gen = torch.Generator().manual_seed(10 + i)
        loader.append({"image": torch.randn(2, 1, 12, 13, 70, generator=gen), "label": torch.randint(0, Cc, (2, 1, 12, 13, 70), generator=gen).float(),
                       "modality": torch.tensor([i % 2, (i + 1) % 2])})
    seen = []

    def on_device(x, modalities=None):
        seen.append(model(x).detach())
        return seen[-1]

    def run(device, inferer, keep):
        res = {}
        ret = E.test(model, loader, device, M.DiceMetric(include_background=True, reduction="mean_batch", get_not_nans=True), E.AsDiscrete(to_onehot=Cc),
                     E.AsDiscrete(argmax=True, to_onehot=Cc), model_inferer=inferer, amp=False,
                     surface_distance=M.SurfaceDistanceMetric(include_background=True, symmetric=True, reduction="mean_batch", get_not_nans=True),
                     hausdorff_distance=M.HausdorffDistanceMetric(include_background=False, percentile=95, reduction="mean_batch", get_not_nans=True),
                     additional_metrics=[M.GeneralizedDiceScore(include_background=False)], results=res, keep_largest=keep)
        return ret, res

    for independent in (True, False):
        seen.clear()
        t = PP.KeepLargestConnectedComponent(independent=independent, connectivity=1)
        ret_dev, res_dev = run(DEV, on_device, t)
        replay = iter([s.cpu() for s in seen])
        ret_cpu, res_cpu = run("cpu", lambda x, modalities=None: next(replay), t)
        assert res_dev.keys() == res_cpu.keys()
        for part in res_dev:
            if part == "additional_metrics":
                assert res_dev[part] == pytest.approx(res_cpu[part], rel=1e-6)
            elif part.startswith("dice"):
                # the per-sample values are equal to the bit (checked below); these are fp32 means of them over the batch, summed in the
                # device's order and in the host's: a few ulp of fp32 (6e-8 each) apart at most, the bar of the existing end-to-end test
                assert list(res_dev[part].values()) == pytest.approx(list(res_cpu[part].values()), rel=1e-6), part
            else:
                assert res_dev[part].keys() == res_cpu[part].keys()
                same(list(res_dev[part].values()), list(res_cpu[part].values()), rel=1e-9)
        assert ret_dev[0] == pytest.approx(ret_cpu[0], rel=1e-6)
        same([ret_dev[1]], [ret_cpu[1]], rel=1e-9)
        for logits, batch in zip(seen, loader):              # per sample: integer counts through the same float arithmetic, equal to the bit
            pred = t.class_map(logits=logits, out_dtype=torch.int32)
            chain = torch.stack([E.AsDiscrete(to_onehot=Cc)(t(E.AsDiscrete(argmax=True)(x))) for x in logits.cpu()])
            label = torch.stack([E.AsDiscrete(to_onehot=Cc)(y) for y in batch["label"]])
            assert torch.equal(pred.cpu(), chain.argmax(1).int())
            assert torch.equal(M.dice_from_class_map(pred, batch["label"], Cc).cpu(), M.dice_metric(chain, label))
            assert torch.equal(M.generalized_dice_from_class_map(pred, batch["label"], Cc, False).cpu(), M.compute_generalized_dice(chain, label, False))
    replay = iter([s.cpu() for s in seen])
    assert run("cpu", lambda x, modalities=None: next(replay), None)[1] != res_cpu          # the filter changes these noisy maps' metrics
