"""Normalized surface Dice at per-class tolerances (MONAI's SurfaceDiceMetric / compute_surface_dice restated in training/metrics.py on the
edge sets and one-way lists of the surface distance) on the CPU: the numpy and scipy restatements against an oracle
that is the rule itself applied to the brute-force lists of test_hausdorff_cpu.py, the values worked out by hand, the integer bound the
kernel compares with, the argument checks, the background slicing, the from-logits form, the cumulative metric object and the evaluation
loop's keyword.  Every comparison is exact: the metric is a ratio of two integer counts.  No GPU."""
import math

import numpy as np
import pytest
import torch

from mi_seg_amd.training import metrics as M
from test_hausdorff_cpu import oracle_lists
from test_surface_distance_cpu import onehot, quirk_cases, random_case, same

SQRT2 = math.sqrt(2.0)
# AT attained distances and just under them
THRESHOLDS = [0.0, 1.0, SQRT2, float(np.nextafter(SQRT2, 0.0)), 2.0, math.sqrt(5.0), 3.0, 0.5]
BOUNDS = [0, 1, 2, 1, 4, 5, 9, 0]
RANDOM_CASES = {"random_a": (16, (17, 19, 23), 6, 2), "random_b": (3, (9, 10, 11), 4, 2), "random_c": (5, (8, 33, 70), 3, 1)}


# ------------------------------------------------------------------------------------------ oracle
def class_taus(C, shift):
    """C tolerances out of THRESHOLDS, a different one for every class"""
    return [THRESHOLDS[(shift + c) % len(THRESHOLDS)] for c in range(C)]


def nsd_from_lists(lists, shape, taus):
    """rule 2 on the one-way lists {(b, c): (d(P -> G), d(G -> P))}; taus: one tolerance per class c"""
    out = np.empty(shape)
    for (b, c), (pg, gp) in lists.items():
        total = len(pg) + len(gp)
        within = sum(1 for d in pg if float(d) <= taus[c]) + sum(1 for d in gp if float(d) <= taus[c])
        out[b, c] = math.nan if total == 0 else float(within) / float(total)
    return out


_CACHE = {}


def case(name):
    """(pred class map, gt class map, C, pred one-hot, gt one-hot, oracle lists) of a named case, computed once"""
    if name not in _CACHE:
        quirks = {c[0]: c for c in quirk_cases()}
        if name in quirks:
            pred, lab, C = quirks[name][1][:, 0].astype(np.int64), quirks[name][2][:, 0].astype(np.int64), 2
        else:
            seed, shape, C, B = RANDOM_CASES[name]
            pred, lab = random_case(seed, shape, C, B=B)
        p, g = onehot(pred, C), onehot(lab, C)
        _CACHE[name] = (pred, lab, C, p, g, oracle_lists(p, g))
    return _CACHE[name]


QUIRKS = [c[0] for c in quirk_cases()]
CASES = QUIRKS + list(RANDOM_CASES)


def exact(a, b):
    same(a, b, rel=0)


# ------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("use_scipy", [False, True])
def test_restatements_vs_oracle(name, use_scipy):
    if use_scipy:
        pytest.importorskip("scipy")
    _, _, C, p, g, lists = case(name)
    yp, y = torch.from_numpy(p).float(), torch.from_numpy(g).float()
    seen = set()
    for shift in range(len(THRESHOLDS)):
        taus = class_taus(C, shift)
        want = nsd_from_lists(lists, p.shape[:2], taus)
        seen.update(want[np.isfinite(want)].tolist())
        exact(M.surface_dice_numpy(p, g, taus, use_scipy=use_scipy), want)
        if use_scipy:              # the one-hot entry point takes scipy when it imports
            full = M.compute_surface_dice(yp, y, taus, include_background=True)
            assert full.dtype == torch.float64 and full.shape == p.shape[:2]
            exact(full.numpy(), want)
            exact(M.compute_surface_dice(yp, y, taus[1:], include_background=False).numpy(), want[:, 1:])
            exact(M.compute_surface_dice(yp, y, taus[1:]).numpy(), want[:, 1:])          # without the background by default
    if name in RANDOM_CASES:
        assert len(seen) > 3 and min(seen) < 0.5 and max(seen) > 0.9, sorted(seen)


def test_sqrt2_and_its_predecessor_differ():
    _, _, C, p, g, lists = case("random_b")
    a = nsd_from_lists(lists, p.shape[:2], [THRESHOLDS[2]] * C)
    b = nsd_from_lists(lists, p.shape[:2], [THRESHOLDS[3]] * C)
    assert THRESHOLDS[3] < THRESHOLDS[2] and np.nansum(a) > np.nansum(b)
    exact(M.surface_dice_numpy(p, g, [THRESHOLDS[2]] * C, use_scipy=False), a)
    exact(M.surface_dice_numpy(p, g, [THRESHOLDS[3]] * C, use_scipy=False), b)
    exact(b, nsd_from_lists(lists, p.shape[:2], [1.0] * C))            # no distance lies strictly between 1 and sqrt(2)


# P: the 13 x 13 square's perimeter (48 voxels), G: the 14 x 9 rectangle's (42): 90 distances.  line: P's ends {2, 6}, G's ends {4, 9}: the
# distances 2, 2 and 2, 3.  border: 120 edge voxels of P's 6 x 3 x 8 block, 96 of G's 4 x 5 x 6 block.
BY_HAND = {"slab": (4 / 90, 31 / 90, 55 / 90), "line": (0.0, 0.0, 0.75), "border": (98 / 216, 151 / 216, 207 / 216),
           "gt_empty": (0.0, 0.0, 0.0), "pred_empty": (0.0, 0.0, 0.0), "single_voxel_pred_only": (math.nan,) * 3,
           "single_voxel_both": (math.nan,) * 3, "both_empty": (math.nan,) * 3}
TABLE = {"slab": (0.0444, 0.3444, 0.6111), "line": (0.0, 0.0, 0.75), "border": (0.4537, 0.6990, 0.9583)}


@pytest.mark.parametrize("name", QUIRKS)
def test_values_by_hand(name):
    _, _, _, p, g, lists = case(name)
    for tau, expect in zip((0.0, 1.0, 2.0), BY_HAND[name]):
        got = M.surface_dice_numpy(p, g, [3.0, tau], use_scipy=False)[0, 1]
        exact([got], [expect])
        exact([nsd_from_lists(lists, (1, 2), [3.0, tau])[0, 1]], [expect])
        if name in TABLE:
            assert abs(got - TABLE[name][(0.0, 1.0, 2.0).index(tau)]) < 1e-4
    for tau in THRESHOLDS + [1e300]:
        if name in ("gt_empty", "pred_empty"):             # one edge set empty: both lists all inf
            assert M.surface_dice_numpy(p, g, [0.0, tau], use_scipy=False)[0, 1] == 0.0
        if math.isnan(BY_HAND[name][0]):
            assert math.isnan(M.surface_dice_numpy(p, g, [0.0, tau], use_scipy=False)[0, 1])


def test_integer_bound_against_a_sqrt_scan():
    """d <= tau on sqrt(d^2) in double <=> d^2 <= surface_dice_bound(tau)"""
    assert [M.surface_dice_bound(t) for t in THRESHOLDS] == BOUNDS
    for tau in THRESHOLDS + [0.999, 4095.0 * SQRT2, 7.0, float(np.nextafter(7.0, 0.0)), float(np.nextafter(7.0, 8.0)), 100.25]:
        k = M.surface_dice_bound(tau)
        hi = int(tau * tau) + 3
        lo = 0 if tau < 16 else hi - 6                      # sqrt is monotone: a window round tau^2 is a full scan
        assert math.sqrt(float(lo)) <= tau < math.sqrt(float(hi))
        scan = max(j for j in range(lo, hi + 1) if math.sqrt(float(j)) <= tau)
        assert k == scan, (tau, k, scan)
    lim = (1 << 26) - 1                                   # clamped above every squared distance of a 4096^3 volume, below the no-seed value
    assert 3 * 4095 ** 2 < lim < (1 << 30)
    for tau in (8192.0, 1e10, 1e300, 1.7e308):
        assert M.surface_dice_bound(tau) == lim


def test_argument_checks():
    _, _, _, p, g, _ = case("slab")
    yp, y = torch.from_numpy(p).float(), torch.from_numpy(g).float()
    for bad in ([1.0, 1.0], [], None):                     # one per class AFTER include_background=False
        with pytest.raises(ValueError):
            M.compute_surface_dice(yp, y, bad)
    with pytest.raises(ValueError):
        M.compute_surface_dice(yp, y, [1.0], include_background=True)
    with pytest.raises(ValueError):
        M.surface_dice_numpy(p, g, [1.0])
    with pytest.raises(ValueError):
        M.surface_metrics_from_logits(yp, y.argmax(1, keepdim=True), 2, want=("nsd",), class_thresholds=[1.0])
    with pytest.raises(ValueError):
        M.surface_metrics_from_logits(yp, y.argmax(1, keepdim=True), 2, want=("asd", "nsd"))
    for bad in (-1.0, -1e-300, math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError):
            M.SurfaceDiceMetric([bad])
        with pytest.raises(ValueError):
            M.compute_surface_dice(yp, y, [bad])
        with pytest.raises(ValueError):
            M.surface_dice_numpy(p, g, [1.0, bad])
        with pytest.raises(ValueError):
            M.surface_dice_from_logits(yp, y.argmax(1, keepdim=True), 2, [1.0, bad])
    with pytest.raises(NotImplementedError):
        M.SurfaceDiceMetric([1.0], distance_metric="chessboard")
    with pytest.raises(NotImplementedError):
        M.compute_surface_dice(yp, y, [1.0], distance_metric="taxicab")
    with pytest.raises(NotImplementedError):
        M.SurfaceDiceMetric([1.0], use_subvoxels=True)
    with pytest.raises(NotImplementedError):
        M.compute_surface_dice(yp, y, [1.0], use_subvoxels=True)
    with pytest.raises(ValueError):
        M.compute_surface_dice(yp, y[:, :1], [1.0])
    m = M.SurfaceDiceMetric([1.0, 2])
    assert (m.class_thresholds, m.include_background, m.distance_metric, m.reduction, m.get_not_nans, m.use_subvoxels) == \
        ([1.0, 2.0], False, "euclidean", "mean", False, False)


def test_from_logits_cpu_matches_the_onehot_form_and_the_oracle():
    pred, lab = random_case(8, (6, 7, 8), 5)
    logits = torch.randn(2, 5, 6, 7, 8)
    logits.scatter_(1, torch.from_numpy(pred)[:, None], 10.0)
    label = torch.from_numpy(lab)[:, None].to(torch.uint8)
    yp, y = torch.from_numpy(onehot(pred, 5)).float(), torch.from_numpy(onehot(lab, 5)).float()
    lists = oracle_lists(onehot(pred, 5), onehot(lab, 5))
    taus = class_taus(5, 1)
    want = nsd_from_lists(lists, (2, 5), taus)
    assert len(set(want[np.isfinite(want)].tolist())) > 3
    for inc in (True, False):
        t = taus[0 if inc else 1:]
        a = M.surface_dice_from_logits(logits, label, 5, t, include_background=inc)
        assert a.dtype == torch.float64
        exact(a.numpy(), want[:, 0 if inc else 1:])
        exact(a.numpy(), M.compute_surface_dice(yp, y, t, include_background=inc).numpy())
        asd, nsd, hd = M.surface_metrics_from_logits(logits, label, 5, include_background=inc, symmetric=True, percentile=95, want=("asd", "nsd", "hd"),
                                                     class_thresholds=t)
        exact(nsd.numpy(), a.numpy())
        asd0, hd0 = M.surface_metrics_from_logits(logits, label, 5, include_background=inc, symmetric=True, percentile=95)
        exact(asd.numpy(), asd0.numpy())
        exact(hd.numpy(), hd0.numpy())


def _three_samples():
    """class 1 in pred and label (a value in (0, 1)), class 2 predicted in sample 0 only and never labelled (0.0 there, NaN elsewhere),
    class 3 nowhere (NaN)"""
    pred = np.zeros((3, 6, 8, 7), dtype=np.int64)
    lab = np.zeros_like(pred)
    for b in range(3):
        lab[b, 1:4, 2:6, 1:5] = 1
        pred[b, 1:4, 2 + b:7, 1:4] = 1
    pred[0, 4:6, 0:3, 4:7] = 2
    return pred, lab


def test_metric_object_buffer_and_aggregate():
    pred, lab = _three_samples()
    yp, y = torch.from_numpy(onehot(pred, 4)).float(), torch.from_numpy(onehot(lab, 4)).float()
    taus = [0.0, SQRT2, 1.0]
    want = nsd_from_lists(oracle_lists(onehot(pred, 4), onehot(lab, 4)), (3, 4), [0.5] + taus)[:, 1:]
    assert ((want[:, 0] > 0) & (want[:, 0] < 1)).all() and want[0, 1] == 0.0 and np.isnan(want[1:, 1]).all() and np.isnan(want[:, 2]).all()
    nsd = M.SurfaceDiceMetric(taus, reduction="mean_batch", get_not_nans=True)
    b1 = nsd(y_pred=yp[:2], y=y[:2])
    b2 = nsd(y_pred=yp[2:], y=y[2:])
    assert b1.shape == (2, 3) and b2.shape == (1, 3) and b1.dtype == torch.float64
    exact(nsd.get_buffer().numpy(), want)
    agg, nn = nsd.aggregate()
    ref, refn = M.do_metric_reduction(torch.from_numpy(want), "mean_batch")
    exact(agg.numpy(), ref.numpy())
    assert agg[0].item() == pytest.approx(want[:, 0].mean(), rel=1e-15)
    assert agg[1].item() == 0.0 and nn.tolist() == [3.0, 1.0, 0.0] == refn.tolist()        # the 0.0 is kept and counted, NaN is left out
    plain = M.SurfaceDiceMetric(taus)
    plain(y_pred=yp, y=y)
    assert isinstance(plain.aggregate(), torch.Tensor) and 0.0 < plain.aggregate().item() < 1.0
    with_bg = M.SurfaceDiceMetric([0.5] + taus, include_background=True, reduction="none")
    exact(with_bg(y_pred=yp, y=y).numpy()[:, 1:], want)
    nsd.reset()
    assert nsd.get_buffer() is None


def test_evaluate_takes_the_metric(capsys):
    from mi_seg_amd.training import evaluate as E
    C = 4
    loader, logits = [], []
    for i in range(3):
        pred, lab = random_case(50 + i, (7, 8, 9), C, B=1)
        x = torch.zeros(1, C, 7, 8, 9)
        x.scatter_(1, torch.from_numpy(pred)[:, None], 1.0)
        logits.append(x)
        loader.append({"image": torch.zeros(1, 1, 7, 8, 9), "label": torch.from_numpy(lab)[:, None].float(), "modality": torch.tensor([i % 2])})
    preds = np.concatenate([x.argmax(1).numpy() for x in logits])
    labs = np.concatenate([b["label"][:, 0].long().numpy() for b in loader])

    def run(**kw):
        replay = iter(logits)
        res = {}
        ret = E.test(torch.nn.Identity(), loader, "cpu", M.DiceMetric(include_background=True, reduction="mean_batch", get_not_nans=True),
                     E.AsDiscrete(to_onehot=C), E.AsDiscrete(argmax=True, to_onehot=C), model_inferer=lambda x, modalities=None: next(replay),
                     amp=False, surface_distance=M.SurfaceDistanceMetric(include_background=True, symmetric=True, reduction="mean_batch",
                                                                         get_not_nans=True), results=res, **kw)
        return ret, res

    ret0, res0 = run()
    out0 = capsys.readouterr().out
    assert set(res0) == {"dice_modality", "dice_total", "surface_distance_modality", "surface_distance_total"}
    assert "Surface Dice" not in out0
    ret1, res1 = run(surface_dice=None)
    assert ret1 == ret0 and res1 == res0 and capsys.readouterr().out == out0
    taus = [1.0, SQRT2, 2.0]
    nsd = M.SurfaceDiceMetric(taus, include_background=False, reduction="mean_batch", get_not_nans=True)
    hd = M.HausdorffDistanceMetric(include_background=False, percentile=95, reduction="mean_batch", get_not_nans=True)
    ret2, res2 = run(surface_dice=nsd, hausdorff_distance=hd)
    out2 = capsys.readouterr().out
    assert ret2 == ret0 and nsd.get_buffer() is None                  # the return value does not change; the metric is reset
    assert set(res2) == set(res0) | {"hausdorff_distance_modality", "hausdorff_distance_total", "surface_dice_modality", "surface_dice_total"}
    assert all(res2[k] == res0[k] for k in res0)
    assert "Surface Dice per modality" in out2 and "val_total_surface_dice/class1" in out2
    want = nsd_from_lists(oracle_lists(onehot(preds, C), onehot(labs, C)), (3, C), [0.0] + taus)[:, 1:]
    tot, _ = M.do_metric_reduction(torch.from_numpy(want), "mean_batch")
    assert list(res2["surface_dice_total"]) == [f"val_total_surface_dice/class{c}" for c in range(1, C)]
    exact(list(res2["surface_dice_total"].values()), tot.numpy())
    for m in (0, 1):
        sel = torch.from_numpy(want[[i for i in range(3) if i % 2 == m]])
        per, _ = M.do_metric_reduction(sel, "mean_batch")
        got = [res2["surface_dice_modality"][f"val_modality{m}/class{c}"] for c in range(1, C)]
        exact(got, per.numpy())
        assert f"val_modality{m}/avg" in res2["surface_dice_modality"]
    ret3, res3 = run(surface_dice=M.SurfaceDiceMetric(taus))          # without get_not_nans: one mean over everything
    assert ret3 == ret0 and set(res3) == set(res0) | {"surface_dice_modality", "surface_dice_total"}
    assert list(res3["surface_dice_total"]) == ["val_total_surface_dice/class1"]
