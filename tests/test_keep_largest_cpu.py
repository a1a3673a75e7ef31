"""CPU tests of the keep-largest-connected-component post-processing (training/postprocess.py): a brute-force flood
fill written here from the rules against keep_largest_numpy (numpy labelling, and scipy's where it imports), the geometry and class-handling
cases by hand, the transform's two input forms, the command line's defaults and evaluate.test with and without the transform.  Class maps
are integers: every comparison is exact."""
import itertools

import numpy as np
import pytest
import torch

from mi_seg_amd.training import postprocess as PP


def oracle(cls, C, applied=None, independent=True, connectivity=3, stats=False):
    """the rules by flood fill on one volume [D, H, W]: components of the applied voxels (same class, or any applied class when joint) in
    raster order of their first voxel; per group the largest stays, the earliest among equals; everything else of the group becomes 0"""
    cls = np.asarray(cls)
    applied = set(range(1, C)) if applied is None else set(applied)
    D, H, W = cls.shape
    offs = [o for o in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(v != 0 for v in o) <= connectivity]
    on = lambda v: 0 <= int(v) < C and int(v) in applied
    seen = np.zeros(cls.shape, dtype=bool)
    comps = {}                                     # group -> [(voxels, first class)]
    for start in itertools.product(range(D), range(H), range(W)):
        if seen[start] or not on(cls[start]):
            continue
        seen[start] = True
        todo, vox = [start], []
        while todo:
            p = todo.pop()
            vox.append(p)
            for o in offs:
                q = (p[0] + o[0], p[1] + o[1], p[2] + o[2])
                if not (0 <= q[0] < D and 0 <= q[1] < H and 0 <= q[2] < W) or seen[q] or not on(cls[q]):
                    continue
                if independent and cls[q] != cls[p]:
                    continue
                seen[q] = True
                todo.append(q)
        comps.setdefault(int(cls[start]) if independent else -1, []).append((vox, int(cls[start])))
    out = cls.copy()
    st = np.zeros((C, 3), dtype=np.int64)
    dropped = np.zeros(cls.shape, dtype=bool)
    for group in comps.values():
        best = max(range(len(group)), key=lambda i: (len(group[i][0]), -i))      # raster order of first voxels: the earliest of the largest
        for i, (vox, c0) in enumerate(group):
            st[c0, 2] += 1
            if i != best:
                for p in vox:
                    dropped[p] = True
    out[dropped] = 0
    for c in range(C):
        st[c, 0] = np.count_nonzero(cls == c)
        st[c, 1] = np.count_nonzero((cls == c) & ~dropped)
    return (out, st) if stats else out


def both(cls, C, applied=None, independent=True, connectivity=3):
    """keep_largest_numpy with the numpy labelling (and scipy's where it imports), checked against the oracle; returns the result"""
    cls = np.asarray(cls)
    want, wst = oracle(cls, C, applied, independent, connectivity, stats=True)
    modes = [False] + ([True] if PP._ndimage() is not None else [])
    for use_scipy in modes:
        got, st = PP.keep_largest_numpy(cls, C, applied, independent, connectivity, use_scipy=use_scipy, return_stats=True)
        assert got.dtype == cls.dtype and np.array_equal(got, want), (use_scipy, independent, connectivity)
        assert np.array_equal(st, wst), (use_scipy, independent, connectivity)
    return want


def random_map(seed, shape, C, p):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < p, rng.integers(1, C, shape), 0).astype(np.int32)


@pytest.mark.parametrize("connectivity", [1, 2, 3])
@pytest.mark.parametrize("independent", [True, False])
def test_random_maps_vs_oracle(connectivity, independent):
    p = {1: 0.33, 2: 0.16, 3: 0.12}[connectivity] * (2.2 if independent else 1.0)     # near percolation: many components, many equal sizes
    for seed, shape in enumerate([(12, 12, 12), (5, 11, 12), (1, 9, 12), (7, 1, 1), (3, 4, 1)]):
        cls = random_map(seed, shape, 4, p)
        both(cls, 4, None, independent, connectivity)
        both(cls, 4, (1, 3), independent, connectivity)
        both(cls, 4, (0, 2), independent, connectivity)          # the background can be filtered like any class


def test_scipy_path_is_exercised():
    pytest.importorskip("scipy")
    cls = random_map(9, (10, 11, 12), 5, 0.3)
    for independent in (True, False):
        a = PP.keep_largest_numpy(cls, 5, None, independent, 2, use_scipy=True)
        b = PP.keep_largest_numpy(cls, 5, None, independent, 2, use_scipy=False)
        assert np.array_equal(a, b) and np.array_equal(a, oracle(cls, 5, None, independent, 2))


def test_numpy_labelling_gives_the_smallest_index():
    cls = random_map(3, (6, 7, 8), 2, 0.45)
    lab = PP.label_components_numpy(cls > 0, 1)
    flat = lab.reshape(-1)
    assert (flat[cls.reshape(-1) == 0] == cls.size).all()
    for v in np.flatnonzero(cls.reshape(-1)):
        assert flat[v] <= v and flat[flat[v]] == flat[v]


def test_face_edge_and_corner_contacts():
    """a 3-voxel bar (the largest) with a single voxel touching it by a face, an edge or a corner only"""
    for contact, (d, h, w) in (("face", (1, 1, 4)), ("edge", (1, 2, 4)), ("corner", (2, 2, 4))):
        cls = np.zeros((4, 4, 6), dtype=np.int32)
        cls[1, 1, 1:4] = 1
        cls[d, h, w] = 1
        joined = {"face": (1, 2, 3), "edge": (2, 3), "corner": (3,)}[contact]
        for conn in (1, 2, 3):
            got = both(cls, 2, None, True, conn)
            assert got[d, h, w] == (1 if conn in joined else 0), (contact, conn)
            assert (got[1, 1, 1:4] == 1).all()


def test_no_wrap_around_rows_slices():
    """the last voxel of a W row and the first of the next (adjacent in memory), and the same across slices, are not neighbours"""
    cls = np.zeros((3, 3, 5), dtype=np.int32)
    cls[0, 0, 3:5] = 1                     # two voxels ending a row
    cls[0, 1, 0] = 1                       # the next row's first voxel: linear index + 1 of the row's end
    cls[0, 2, 4] = 1
    cls[1, 0, 0] = 1                       # first voxel of the next slice
    got = both(cls, 2, None, True, 1)
    assert got.sum() == 2 and (got[0, 0, 3:5] == 1).all()
    got = both(cls, 2, None, True, 3)
    assert got.sum() == 2 and (got[0, 0, 3:5] == 1).all()


def test_tie_goes_to_the_smaller_first_index():
    cls = np.zeros((2, 5, 9), dtype=np.int32)
    cls[1, 3, 1:4] = 1
    cls[0, 4, 5:8] = 1                     # same size, earlier in raster order
    cls[1, 0, 7:9] = 1
    got = both(cls, 2)
    assert (got[0, 4, 5:8] == 1).all() and got.sum() == 3
    # a component that starts later but reaches an earlier row is judged by its smallest index, not by where one would first "meet" it
    cls = np.zeros((1, 4, 6), dtype=np.int32)
    cls[0, 1, 0:3] = 2
    cls[0, 0, 5] = 2
    cls[0, 1, 5] = 2
    cls[0, 2, 5] = 2
    got = both(cls, 3)
    assert got.sum() == 6 and (got[0, :3, 5] == 2).all()


def test_single_voxel_and_empty():
    cls = np.zeros((1, 1, 1), dtype=np.int32)
    assert both(cls, 2)[0, 0, 0] == 0
    cls[0, 0, 0] = 1
    assert both(cls, 2)[0, 0, 0] == 1
    cls = np.zeros((3, 3, 3), dtype=np.int32)
    cls[1, 1, 1] = 2
    assert np.array_equal(both(cls, 4), cls)              # classes 1 and 3 are applied and empty: nothing happens


def test_touching_classes_independent_and_joint():
    cls = np.zeros((1, 3, 10), dtype=np.int32)
    cls[0, 1, 0:3] = 1
    cls[0, 1, 3:5] = 2                     # touches class 1
    cls[0, 1, 7:9] = 1                     # an island of class 1
    cls[0, 0, 9] = 2                       # an island of class 2, touching the class-1 island by a corner
    ind = both(cls, 3, None, True, 3)
    assert ind[0, 1].tolist() == [1, 1, 1, 2, 2, 0, 0, 0, 0, 0] and ind[0, 0, 9] == 0
    joint = both(cls, 3, None, False, 3)
    assert joint[0, 1].tolist() == [1, 1, 1, 2, 2, 0, 0, 0, 0, 0] and joint[0, 0, 9] == 0      # one component of 5, its voxels keep their classes
    joint1 = both(cls, 3, None, False, 1)
    assert np.array_equal(joint1, joint)
    # joint mode keeps a smaller class attached to the largest component even where that class has a larger island of its own
    cls[0, 2, 5:10] = 2
    cls[0, 1, 7:9] = 0
    cls[0, 0, 9] = 0
    ind = both(cls, 3, None, True, 1)
    assert ind[0, 1, 3:5].tolist() == [0, 0] and (ind[0, 2, 5:10] == 2).all()
    joint = both(cls, 3, None, False, 1)
    assert joint[0, 1, :5].tolist() == [1, 1, 1, 2, 2] and (joint[0, 2] == 0).all()      # 5 = 5 voxels: the earlier component


def test_unapplied_class_untouched_and_connects_nothing():
    cls = np.zeros((1, 1, 9), dtype=np.int32)
    cls[0, 0] = [1, 1, 3, 1, 0, 3, 0, 2, 2]
    got = both(cls, 4, (1, 2), True, 1)
    assert got[0, 0].tolist() == [1, 1, 3, 0, 0, 3, 0, 2, 2]
    got = both(cls, 4, (1, 2), False, 1)                    # class 3 is no bridge in joint mode either
    assert got[0, 0].tolist() == [1, 1, 3, 0, 0, 3, 0, 0, 0]


def test_out_of_range_values_pass_through():
    cls = np.zeros((1, 2, 6), dtype=np.int32)
    cls[0, 0] = [1, 1, 7, 1, -2, 1]
    cls[0, 1] = [0, 0, 99, 0, 0, 0]
    got = both(cls, 3, None, True, 1)
    assert got[0, 0].tolist() == [1, 1, 7, 0, -2, 0] and got[0, 1, 2] == 99


def test_applied_label_checks():
    with pytest.raises(ValueError):
        PP.keep_largest_numpy(np.zeros((2, 2, 2), dtype=np.int32), 3, (3,))
    with pytest.raises(ValueError):
        PP.keep_largest_numpy(np.zeros((2, 2, 2), dtype=np.int32), 3, None, True, 4)
    with pytest.raises(ValueError):
        PP.keep_largest_numpy(np.zeros((2, 2, 2), dtype=np.int32), 65)
    assert PP.applied_mask(None, 64) == (1 << 64) - 2 and PP.applied_mask((0, 63), 64) == (1 << 63) | 1


def test_mask_helper():
    img = random_map(5, (6, 7, 8), 2, 0.3)
    for conn in (1, 2, 3, None):
        want = oracle(img, 2, None, True, 3 if conn is None else conn) != 0
        got = PP.get_largest_connected_component_mask(img, conn)
        assert got.dtype == bool and np.array_equal(got, want)
        t = PP.get_largest_connected_component_mask(torch.from_numpy(img), conn, use_scipy=False)
        assert t.dtype == torch.bool and np.array_equal(t.numpy(), want)
    two_d = img[0]
    assert np.array_equal(PP.get_largest_connected_component_mask(two_d, 2), oracle(two_d[None], 2, None, True, 2)[0] != 0)
    assert not PP.get_largest_connected_component_mask(np.zeros((3, 3), dtype=np.int32)).any()
    with pytest.raises(NotImplementedError):
        PP.get_largest_connected_component_mask(img, num_components=2)


@pytest.mark.parametrize("independent", [True, False])
def test_transform_onehot_and_single_channel_agree(independent):
    C = 4
    cls = random_map(21, (7, 8, 9), C, 0.35)
    for applied in (None, (1, 3)):
        t = PP.KeepLargestConnectedComponent(applied_labels=applied, independent=independent, connectivity=2)
        want = oracle(cls, C, applied, independent, 2)
        single = t(torch.from_numpy(cls)[None].float())
        assert single.dtype == torch.float32 and single.shape == (1, 7, 8, 9) and np.array_equal(single[0].numpy(), want)
        onehot = torch.nn.functional.one_hot(torch.from_numpy(cls).long(), C).movedim(-1, 0).float()
        got = t(onehot)
        assert got.shape == onehot.shape and got.dtype == onehot.dtype
        back = (got * torch.arange(C, dtype=torch.float32).view(C, 1, 1, 1)).sum(0)
        assert np.array_equal(back.numpy(), want)
        assert torch.equal(got[0], onehot[0])                                   # the background channel is not applied
        assert torch.equal(t(torch.from_numpy(cls)[None]), torch.from_numpy(want)[None])      # an integer sample keeps its dtype
    two_d = PP.KeepLargestConnectedComponent()(torch.from_numpy(cls[0])[None].float())
    assert np.array_equal(two_d[0].numpy(), oracle(cls[:1], C)[0])
    assert PP.KeepLargestConnectedComponent(is_onehot=True)(onehot[:1]).equal(onehot[:1])      # one channel, told to be one-hot: nothing applied


def test_num_components_other_than_one_is_refused():
    with pytest.raises(NotImplementedError):
        PP.KeepLargestConnectedComponent(num_components=2)
    PP.KeepLargestConnectedComponent(num_components=1)
    with pytest.raises(ValueError):
        PP.KeepLargestConnectedComponent(connectivity=4)


def test_parser_defaults():
    from mi_seg_amd.training import predict as R
    args = R.build_parser().parse_args([])
    assert args.keep_largest is False and args.keep_largest_connectivity == 3 and args.keep_largest_labels is None and args.keep_largest_joint is False
    assert R.keep_largest_options(args) is None
    args = R.build_parser().parse_args(["--keep_largest", "--keep_largest_labels", "1", "5", "--keep_largest_joint", "--keep_largest_connectivity", "1"])
    assert R.keep_largest_options(args) == dict(applied_labels=[1, 5], independent=False, connectivity=1)


def test_label_export_of_a_class_map_cpu():
    from mi_seg_amd.hip import ops
    from test_predict_cpu import make_geom
    g = make_geom((9, 7, 11), (2, 0, 1), (True, False, True), (8, 12, 6), (1, 0, 2), (0, 1, 0))
    logits = torch.randn((5,) + g.padded_shape, generator=torch.Generator().manual_seed(1))
    tables, axes = g.index_tables()
    lut = torch.tensor([0, 500, 600, 420, 550], dtype=torch.int32)
    want = ops.label_export(logits, tables, axes, lut)
    for dt in (torch.uint8, torch.int32):
        got = ops.label_export(None, tables, axes, lut, pred=ops.first_max_argmax(logits).to(dt))
        assert got.dtype == want.dtype and torch.equal(got.view(torch.int16), want.view(torch.int16))
    with pytest.raises(ValueError, match="exactly one"):
        ops.label_export(logits, tables, axes, lut, pred=ops.first_max_argmax(logits).to(torch.uint8))


def test_evaluate_with_and_without_the_transform(capsys):
    """keep_largest=None is the old loop to the byte; with the transform the result is the generic chain with the transform placed by hand
    between the argmax and the one-hot"""
    from mi_seg_amd.training import evaluate as E
    from mi_seg_amd.training import metrics as M
    C = 4
    model = torch.nn.Conv3d(1, C, 3, padding=1)
    with torch.no_grad():
        g = torch.Generator().manual_seed(0)
        model.weight.copy_(torch.randn(model.weight.shape, generator=g))
        model.bias.copy_(torch.tensor([0.8, 0.0, -0.2, -0.4]))
    loader = []
    for i in range(3):
        g = torch.Generator().manual_seed(10 + i)
        loader.append({"image": torch.randn(1, 1, 7, 9, 10, generator=g), "label": torch.randint(0, C, (1, 1, 7, 9, 10), generator=g).float(),
                       "modality": torch.tensor([i % 2])})

    def run(post_pred=None, **kw):
        res = {}
        gd = M.GeneralizedDiceScore(include_background=False)
        ret = E.test(model, loader, "cpu", M.DiceMetric(include_background=True, reduction="mean_batch", get_not_nans=True), E.AsDiscrete(to_onehot=C),
                     post_pred or E.AsDiscrete(argmax=True, to_onehot=C), model_inferer=lambda x, modalities=None: model(x), amp=False,
                     surface_distance=M.SurfaceDistanceMetric(include_background=False, symmetric=True, reduction="mean_batch", get_not_nans=True),
                     hausdorff_distance=M.HausdorffDistanceMetric(include_background=False, percentile=95, reduction="mean_batch", get_not_nans=True),
                     additional_metrics=[gd], results=res, **kw)
        return repr((ret, res)), capsys.readouterr().out

    old = run()
    assert run(keep_largest=None) == old
    t = PP.KeepLargestConnectedComponent(connectivity=1)
    got = run(keep_largest=t)
    discrete, onehot = E.AsDiscrete(argmax=True), E.AsDiscrete(to_onehot=C)
    by_hand = run(post_pred=lambda x: onehot(t(discrete(x))))
    assert got == by_hand
    assert got != old                                                       # the filter removed something on these noisy maps
