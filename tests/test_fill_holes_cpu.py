"""CPU tests of the fill-holes post-processing (training/postprocess.py): MONAI's dilation recipe on scipy against the
numpy labelling plus a face flag, the geometry and label-handling cases worked out by hand (hand_cases below; the device tests run them too),
the transform's two input forms, the argument checks, the command line's defaults and evaluate.test with the transform.  Class maps are
integers: every comparison is exact."""
import numpy as np
import pytest
import torch

from mi_seg_amd.training import postprocess as PP

SMALL = (9, 10, 70)             # crosses the device's 8 x 8 x 64 tile on every axis


def both(cls, C, applied=None, connectivity=3):
    """fill_holes_numpy with the numpy labelling and, where scipy imports, with MONAI's dilation recipe: equal maps and statistics"""
    cls = np.asarray(cls)
    want, wst = PP.fill_holes_numpy(cls, C, applied, connectivity, use_scipy=False, return_stats=True)
    assert want.dtype == cls.dtype and want.shape == cls.shape
    if PP._ndimage() is not None:
        got, st = PP.fill_holes_numpy(cls, C, applied, connectivity, use_scipy=True, return_stats=True)
        assert np.array_equal(got, want) and np.array_equal(st, wst), (applied, connectivity)
    labels = PP.fill_labels(applied, C)
    assert all(wst[..., c].sum() == 0 for c in range(C) if c not in labels)
    return want, wst


def blob_map(seed, shape, C, salt=0.03):
    """coarse random blocks of the classes 0..C-1 (3 x 4 x 7 voxels each) with `salt` of the voxels set to a random class: the salt inside a
    block is what gets filled"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, C, tuple(-(-s // k) for s, k in zip(shape, (3, 4, 7))))
    cls = coarse.repeat(3, 0).repeat(4, 1).repeat(7, 2)[:shape[0], :shape[1], :shape[2]].astype(np.int32)
    hit = rng.random(shape) < salt
    cls[hit] = rng.integers(0, C, shape)[hit]
    return cls


def noise_map(seed, shape, connectivity):
    """label 1 at a density that leaves its complement just above the site-percolation point of the neighbourhood (0.312 / 0.137 / 0.097 for
    6 / 18 / 26 neighbours): long winding open components next to many enclosed ones"""
    keep = {1: 0.34, 2: 0.15, 3: 0.11}[connectivity]
    rng = np.random.default_rng(seed)
    cls = np.ones(shape, dtype=np.int32)
    hit = rng.random(shape) < keep
    cls[hit] = rng.integers(0, 2, shape)[hit] * 2               # 0 or 2: both passable for label 1
    return cls


def cube():
    """a 7 x 7 x 7 volume with a 5 x 5 x 5 block of label 1 in its middle"""
    cls = np.zeros((7, 7, 7), dtype=np.int32)
    cls[1:6, 1:6, 1:6] = 1
    return cls


def hand_cases():
    """(name, class map, C, applied labels, connectivity, the expected map) - each expectation built here by hand from the rules"""
    cases = []
    for conn in (1, 2, 3):
        c = cube()
        c[3, 3, 3] = 0
        c[2, 3, 2:4] = 0                                        # a second cavity of two voxels, edge-adjacent to the first
        cases.append((f"enclosed cavity c={conn}", c, 2, None, conn, cube()))
        c = cube()
        c[0:4, 3, 3] = 0                                        # a tunnel from the face d = 0 to the middle
        cases.append((f"cavity open to a face c={conn}", c, 2, None, conn, c.copy()))
        # a chain of edge-diagonal steps from the middle to a dent in the block's surface: a leak for 18 / 26 neighbours, none for 6
        c = cube()
        c[3, 3, 3] = c[2, 2, 3] = c[1, 1, 3] = 0
        want = c.copy()
        if conn == 1:
            want[3, 3, 3] = want[2, 2, 3] = 1                   # (1, 1, 3) is a dent of the surface: open under every neighbourhood
        cases.append((f"edge-diagonal leak c={conn}", c, 2, None, conn, want))
        c = cube()
        c[3, 3, 3] = c[2, 2, 2] = c[1, 1, 1] = 0               # corner-diagonal steps: a leak for 26 neighbours only
        want = c.copy()
        if conn < 3:
            want[3, 3, 3] = want[2, 2, 2] = 1
        cases.append((f"corner-diagonal leak c={conn}", c, 2, None, conn, want))
        c = cube()
        c[4:6] *= 2                                             # the block's far part is label 2
        c[3:5, 3, 3] = 0                                        # a cavity walled by both labels: each pass sees the other label as a way out
        cases.append((f"two-label wall c={conn}", c, 3, None, conn, c.copy()))
        c = cube()
        c[3, 3, 2:4] = 2
        cases.append((f"label-2 blob inside label 1 c={conn}", c, 3, None, conn, cube()))
        cases.append((f"label-2 blob, only label 2 applied c={conn}", c, 3, (2,), conn, c.copy()))
        # MONAI's docstring example as the middle slice between two solid caps: the hole of 1 is enclosed; the one next to 2 is walled by 2 and
        # 3 together; the one in 3 lies on the edge
        row = np.array([1, 1, 1, 2, 2, 2, 3, 3], dtype=np.int32)
        c = np.tile(row, (3, 3, 1))
        c[1, 1] = [1, 0, 1, 2, 0, 0, 3, 0]
        want = c.copy()
        want[1, 1] = [1, 1, 1, 2, 0, 0, 3, 0]
        cases.append((f"MONAI docstring example c={conn}", c, 4, None, conn, want))
        c = np.ones((1, 9, 9), dtype=np.int32)                  # a ring in a single slice: every voxel lies on a face of the volume
        c[0, 3:6, 3:6] = 0
        for ax in range(3):
            m = np.moveaxis(c, 0, ax)
            cases.append((f"side of length 1 on axis {ax} c={conn}", m, 2, None, conn, m.copy()))
        c = cube()
        c[3, 3, 3] = 0
        cases.append((f"label 0 in applied_labels c={conn}", c, 2, (0, 1), conn, cube()))
        cases.append((f"only label 0 applied c={conn}", c, 2, (0,), conn, c.copy()))
        c = cube()
        c[3, 3, 3], c[0, 0, 0], c[6, 2, 3], c[2, 3, 3] = 200, 200, -7, 3
        want = cube()
        want[0, 0, 0], want[6, 2, 3] = 200, -7                  # outside a cavity: copied through; inside: overwritten (3 >= C too)
        cases.append((f"out-of-range values c={conn}", c, 3, None, conn, want))
    return cases


@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    _, cls, C, applied, conn, want = case
    got, st = both(cls, C, applied, conn)
    assert np.array_equal(got, want)
    assert st.sum() == np.count_nonzero(got != cls)
    assert np.array_equal(PP.fill_holes_numpy(cls[None], C, applied, conn)[0], want)          # the batched form


@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_scipy_recipe_equals_numpy_labelling(connectivity):
    filled = 0
    for seed in range(6):
        for C in (2, 4):
            cls = blob_map(seed, SMALL, C)
            got, st = both(cls, C, None, connectivity)
            filled += int(st.sum())
            both(cls, C, (C - 1,), connectivity)
    assert filled > 50                                           # these maps do have holes
    cls = noise_map(3, (17, 9, 130), connectivity)
    assert both(cls, 3, (1,), connectivity)[1].sum() > 0


def test_scipy_path_is_exercised():
    if PP._ndimage() is None:
        pytest.skip("scipy is not installed: the numpy labelling is the only path")
    import unittest.mock as mock
    with mock.patch.object(PP, "label_components_numpy", side_effect=AssertionError("numpy labelling called")):
        PP.fill_holes_numpy(blob_map(0, SMALL, 3), 3)


def test_ascending_order_and_stats():
    """label 2's pass sees what label 1's pass left: a 2 inside 1 is gone before its own hole could be filled"""
    c = np.zeros((9, 9, 9), dtype=np.int32)
    c[1:8, 1:8, 1:8] = 1
    c[3:6, 3:6, 3:6] = 2
    c[4, 4, 4] = 0
    got, st = both(c, 3, (2, 1), 1)                             # given out of order
    assert (got[1:8, 1:8, 1:8] == 1).all() and st.tolist() == [0, 27, 0]
    got, st = both(c, 3, (2,), 1)
    assert got[4, 4, 4] == 2 and st.tolist() == [0, 0, 1]


def test_argument_checks():
    cls = np.zeros((3, 3, 3), dtype=np.int32)
    for bad in (0, 4, "x"):
        with pytest.raises(ValueError):
            PP.fill_holes_numpy(cls, 2, connectivity=bad)
    with pytest.raises(ValueError, match="applied label"):
        PP.fill_holes_numpy(cls, 2, applied_labels=(2,))
    with pytest.raises(ValueError, match="num_classes"):
        PP.fill_holes_numpy(cls, 65)
    with pytest.raises(ValueError, match="shape"):
        PP.fill_holes_numpy(cls[0], 2)
    with pytest.raises(ValueError):
        PP.FillHoles(connectivity=5)
    with pytest.raises(ValueError, match="applied labels"):
        PP.FillHoles(applied_labels=(4,))(torch.zeros(3, 4, 4, 4))
    with pytest.raises(ValueError, match="applied label"):
        PP.FillHoles(applied_labels=(64,))(torch.zeros(1, 4, 4, 4))
    with pytest.raises(ValueError, match="channel-first"):
        PP.FillHoles()(torch.zeros(4))
    from mi_seg_amd.hip import ops
    t = torch.zeros(1, 3, 3, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="exactly one"):
        ops.fill_holes(logits=torch.zeros(1, 2, 3, 3, 3), pred=t, num_classes=2)
    with pytest.raises(ValueError, match="num_classes"):
        ops.fill_holes(pred=t)
    with pytest.raises(ValueError, match="out_dtype"):
        ops.fill_holes(pred=t, num_classes=2, out_dtype=torch.int64)
    with pytest.raises(ValueError, match="integer class map"):
        ops.fill_holes(pred=t.float(), num_classes=2)


def test_op_on_cpu_tensors():
    """hip/ops.py::fill_holes on CPU tensors is the restatement: logits through the first-maximum argmax, uint8 truncation of the output"""
    from mi_seg_amd.hip import ops
    c = cube()
    c[3, 3, 3], c[0, 0, 0] = 0, 300
    out, st = ops.fill_holes(pred=torch.from_numpy(c)[None], num_classes=2, stats=True)
    assert out.dtype == torch.uint8 and out[0, 3, 3, 3] == 1 and out[0, 0, 0, 0] == 300 - 256 and st.tolist() == [[0, 1]]
    out = ops.fill_holes(pred=torch.from_numpy(c)[None], num_classes=2, out_dtype=torch.int32)
    assert out[0, 0, 0, 0] == 300
    c[0, 0, 0] = 0
    logits = torch.nn.functional.one_hot(torch.from_numpy(c).long(), 2).movedim(-1, 0).float()[None]
    assert torch.equal(ops.fill_holes(logits=logits, out_dtype=torch.int32)[0], torch.from_numpy(cube()))


def test_transform_class_map_and_onehot():
    C = 4
    cls = blob_map(2, SMALL, C)
    want = PP.fill_holes_numpy(cls, C, None, 2)
    assert not np.array_equal(want, cls)
    t = PP.FillHoles(connectivity=2)
    single = torch.from_numpy(cls)[None].float()
    got = t(single)
    assert got.dtype == torch.float32 and torch.equal(got, torch.from_numpy(want)[None].float()) and torch.equal(single, torch.from_numpy(cls)[None].float())
    assert torch.equal(PP.FillHoles(applied_labels=(0, 3), connectivity=2)(single)[0], torch.from_numpy(PP.fill_holes_numpy(cls, C, (3,), 2)).float())
    # a class map keeps what is no label: non-integral values and values of 64 and above are passable, are overwritten inside a hole only
    odd = torch.from_numpy(cube())[None].float()
    odd[0, 3, 3, 3], odd[0, 0, 0, 0], odd[0, 6, 6, 6], odd[0, 2, 3, 3] = 0.5, 0.5, 99.0, 64.0
    got = PP.FillHoles()(odd)
    assert got[0, 3, 3, 3] == 1 and got[0, 2, 3, 3] == 1 and got[0, 0, 0, 0] == 0.5 and got[0, 6, 6, 6] == 99.0
    # one-hot: every applied channel is a binary map of its own (its holes are the voxels that are 0 in it), returned as 0 / 1
    onehot = torch.nn.functional.one_hot(torch.from_numpy(cls).long(), C).movedim(-1, 0).float()
    for applied in (None, (1, 3), (0, 2)):
        got = PP.FillHoles(applied_labels=applied, connectivity=1)(onehot)
        for ch in range(C):
            labels = range(1, C) if applied is None else [a for a in applied if a != 0]
            if ch in labels:
                assert torch.equal(got[ch], torch.from_numpy(PP.fill_holes_numpy((cls == ch).astype(np.int32), 2, (1,), 1)).float())
            else:
                assert torch.equal(got[ch], onehot[ch])
    # fewer spatial dims: leading axes of size 1, so every voxel lies on a face and nothing is filled
    ring = torch.ones(1, 9, 9)
    ring[0, 3:6, 3:6] = 0
    assert torch.equal(PP.FillHoles()(ring), ring)
    assert torch.equal(PP.FillHoles()(ring.numpy()), ring)


def test_parser_defaults():
    from mi_seg_amd.training import predict as R
    args = R.build_parser().parse_args([])
    assert args.fill_holes is False and args.fill_holes_labels is None and args.fill_holes_connectivity == 3
    assert R.fill_holes_options(args) is None
    args = R.build_parser().parse_args(["--fill_holes", "--fill_holes_labels", "2", "5", "--fill_holes_connectivity", "1"])
    assert R.fill_holes_options(args) == dict(applied_labels=[2, 5], connectivity=1)
    assert R.keep_largest_options(args) is None


def test_evaluate_with_the_transform():
    """evaluate.test(fill_holes=) on the CPU (the one-hot chain): the transform after the keep-largest one, alone, and not at all"""
    from mi_seg_amd.training import evaluate as E
    from mi_seg_amd.training import metrics as M
    Cc = 3
    gen = torch.Generator().manual_seed(0)
    label = torch.from_numpy(np.stack([blob_map(5 + b, SMALL, Cc, salt=0.0) for b in range(2)])[:, None]).float()
    noisy = torch.from_numpy(np.stack([blob_map(5 + b, SMALL, Cc, salt=0.05) for b in range(2)])[:, None])          # the same blocks, salted
    logits = torch.nn.functional.one_hot(noisy[:, 0].long(), Cc).movedim(-1, 1).float() + 0.1 * torch.rand(2, Cc, *SMALL, generator=gen)
    loader = [{"image": logits, "label": label, "modality": torch.tensor([0, 1])}]

    def run(**kw):
        res = {}
        E.test(torch.nn.Identity(), loader, "cpu", M.DiceMetric(include_background=True, reduction="mean_batch", get_not_nans=True),
               E.AsDiscrete(to_onehot=Cc), E.AsDiscrete(argmax=True, to_onehot=Cc), model_inferer=lambda x, modalities=None: x, amp=False, results=res, **kw)
        return res

    def by_hand(*filters):
        dice = []
        for b in range(2):
            cls = logits[b].argmax(0, keepdim=True).float()
            for f in filters:
                cls = f(cls)
            dice.append(M.dice_metric(E.AsDiscrete(to_onehot=Cc)(cls)[None], E.AsDiscrete(to_onehot=Cc)(label[b])[None])[0])
        return torch.stack(dice)

    fh, kl = PP.FillHoles(connectivity=1), PP.KeepLargestConnectedComponent(connectivity=1)
    plain, filled, chained = run(), run(fill_holes=fh), run(keep_largest=kl, fill_holes=fh)
    assert plain == run(fill_holes=None) and plain != filled and filled != chained
    for res, hand in ((filled, by_hand(fh)), (chained, by_hand(kl, fh))):
        for b in range(2):
            vals = [res["dice_modality"][f"val_modality{b}/class{c}"] for c in range(Cc)]
            assert vals == pytest.approx(hand[b].tolist(), rel=1e-6)
    assert sum(filled["dice_modality"].values()) > sum(plain["dice_modality"].values())          # the salt inside the blocks is gone
