"""Hausdorff distance (MONAI 1.1.0 compute_hausdorff_distance, restated in training/metrics.py) on the CPU: the numpy
and scipy restatements against an oracle built here from the brute-force edge sets and one-way lists of test_surface_distance_cpu.py plus the
percentile rule written out on a sorted list; the empty / all-inf rules, a value worked out by hand, the argument checks, the cumulative
metric object and the evaluation loop's new keyword.  No GPU."""
import math

import numpy as np
import pytest
import torch

from mi_seg_amd.training import metrics as M
from test_surface_distance_cpu import _edge_coords, _one_way, onehot, quirk_cases, random_case, same

REL = 1e-9
PERCENTILES = [None, 0, 100, 95, 50, 37.5]


# ------------------------------------------------------------------------------------------ oracle
def oracle_lists(pred, gt):
    """pred, gt: bool [B, C, D, H, W] -> {(b, c): (d(P -> G), d(G -> P))} as python lists, by pairwise nearest-edge search"""
    out = {}
    for b in range(pred.shape[0]):
        for c in range(pred.shape[1]):
            p, g = pred[b, c], gt[b, c]
            u = p | g
            if not u.any():
                out[b, c] = ([], [])
                continue
            idx = np.nonzero(u)
            lo, hi = [int(i.min()) for i in idx], [int(i.max()) for i in idx]
            ep, eg = _edge_coords(p, lo, hi), _edge_coords(g, lo, hi)
            out[b, c] = (_one_way(ep, eg), _one_way(eg, ep))
    return out


def rule1(d, percentile):
    """h of one list: NaN if empty, inf if all inf, the maximum for percentile None / 0, else the linear percentile on the sorted list"""
    if not d:
        return math.nan
    v = sorted(float(x) for x in d)
    if math.isinf(v[0]):
        return math.inf
    if not percentile:
        return v[-1]
    n = len(v)
    pos = (percentile / 100) * (n - 1)
    lo = math.floor(pos)
    hi = min(lo + 1, n - 1)
    return v[lo] + (v[hi] - v[lo]) * (pos - lo)


def hd_from_lists(lists, shape, percentile, directed):
    out = np.empty(shape)
    for (b, c), (pg, gp) in lists.items():
        h = rule1(pg, percentile)
        out[b, c] = h if directed else max(h, rule1(gp, percentile))
    return out


def oracle_hd(pred, gt, percentile, directed):
    return hd_from_lists(oracle_lists(pred, gt), pred.shape[:2], percentile, directed)


_CACHE = {}


def case(name):
    """(pred one-hot, gt one-hot, oracle lists) of a named case, computed once"""
    if name not in _CACHE:
        quirks = {c[0]: c for c in quirk_cases()}
        if name in quirks:
            p, g = onehot(quirks[name][1][:, 0].astype(np.int64), 2), onehot(quirks[name][2][:, 0].astype(np.int64), 2)
        else:
            shape = {"random_a": (17, 19, 23), "random_b": (33, 1, 40)}[name]
            pred, lab = random_case(16, shape, 6)
            p, g = onehot(pred, 6), onehot(lab, 6)
        _CACHE[name] = (p, g, oracle_lists(p, g))
    return _CACHE[name]


CASES = [c[0] for c in quirk_cases()] + ["random_a", "random_b"]


# ------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("use_scipy", [False, True])
def test_restatements_vs_oracle(name, use_scipy):
    if use_scipy:
        pytest.importorskip("scipy")
    p, g, lists = case(name)
    yp, y = torch.from_numpy(p).float(), torch.from_numpy(g).float()
    for pct in PERCENTILES:
        for directed in (False, True):
            want = hd_from_lists(lists, p.shape[:2], pct, directed)
            same(M.hausdorff_distance_numpy(p, g, pct, directed, use_scipy=use_scipy), want, rel=REL)
            if use_scipy:              # the one-hot entry point takes scipy when it imports
                for inc in (True, False):
                    got = M.compute_hausdorff_distance(yp, y, include_background=inc, percentile=pct, directed=directed)
                    assert got.dtype == torch.float64 and got.shape == (p.shape[0], p.shape[1] - (0 if inc else 1))
                    same(got.numpy(), want[:, 0 if inc else 1:], rel=REL)


def test_random_cases_hold_finite_inf_and_nan():
    for name in ("random_a", "random_b"):
        want = hd_from_lists(case(name)[2], case(name)[0].shape[:2], 95, False)
        assert np.isfinite(want).any() and np.isinf(want).any(), name
    pred, lab = random_case(16, (17, 19, 23), 6)
    pred[pred == 3] = 0                  # a class absent from both: NaN
    lab[lab == 3] = 0
    want = oracle_hd(onehot(pred, 6), onehot(lab, 6), 95, False)
    assert np.isnan(want[:, 3]).all() and np.isfinite(want).any() and np.isinf(want).any()
    same(M.hausdorff_distance_numpy(onehot(pred, 6), onehot(lab, 6), 95, False, use_scipy=False), want, rel=REL)


@pytest.mark.parametrize("name", CASES)
def test_maximum_forms_agree(name):
    """percentile None, 0 and 100 are the maximum of the list"""
    p, g, lists = case(name)
    for directed in (False, True):
        a = M.hausdorff_distance_numpy(p, g, None, directed, use_scipy=False)
        same(M.hausdorff_distance_numpy(p, g, 0, directed, use_scipy=False), a, rel=0)
        same(M.hausdorff_distance_numpy(p, g, 100, directed, use_scipy=False), a, rel=0)
        for (b, c), (pg, gp) in lists.items():
            m = max(pg) if pg else math.nan
            if not directed:
                m = max(m, max(gp)) if gp else m
            same([a[b, c]], [m], rel=REL)


@pytest.mark.parametrize("pct", PERCENTILES)
@pytest.mark.parametrize("directed", [False, True])
def test_empty_and_missed_classes(pct, directed):
    """a class missed entirely (or predicted where there is none) is inf at EVERY percentile, where numpy's interpolation gives NaN; no
    foreground, or a union of one voxel, is NaN"""
    for name in ("gt_empty", "pred_empty"):
        p, g, _ = case(name)
        assert math.isinf(M.hausdorff_distance_numpy(p, g, pct, directed, use_scipy=False)[0, 1]), name
    for name in ("both_empty", "single_voxel_pred_only", "single_voxel_both"):
        p, g, _ = case(name)
        assert math.isnan(M.hausdorff_distance_numpy(p, g, pct, directed, use_scipy=False)[0, 1]), name


def test_slab_by_hand():
    """P: the square h, w in [4, 16] of one plane, G: the rectangle h in [1, 14], w in [5, 13] of the same plane; the plane axis is squeezed, so
    the edges are the two perimeters.  The P-edge voxel farthest from G's perimeter is P's corner (16, 16), whose nearest G-edge voxel is G's
    corner (14, 13): sqrt(2^2 + 3^2).  Every G-edge voxel is within 3 of P's perimeter (G's top row h = 1 is 3 from P's row h = 4, its column
    w = 13 is 3 from P's column w = 16, its column w = 5 is 1 from P's column w = 4, its row h = 14 is 2 from P's row h = 16)."""
    p, g, _ = case("slab")
    assert M.hausdorff_distance_numpy(p, g, None, True, use_scipy=False)[0, 1] == pytest.approx(math.sqrt(13.0), rel=1e-15)
    assert M.hausdorff_distance_numpy(g, p, None, True, use_scipy=False)[0, 1] == pytest.approx(3.0, rel=1e-15)
    assert M.hausdorff_distance_numpy(p, g, None, False, use_scipy=False)[0, 1] == pytest.approx(math.sqrt(13.0), rel=1e-15)
    assert M.hausdorff_distance_numpy(g, p, None, False, use_scipy=False)[0, 1] == pytest.approx(math.sqrt(13.0), rel=1e-15)


def test_argument_checks():
    p, g, _ = case("slab")
    yp, y = torch.from_numpy(p).float(), torch.from_numpy(g).float()
    for bad in (-1, 100.5):
        with pytest.raises(ValueError):
            M.HausdorffDistanceMetric(percentile=bad)
        with pytest.raises(ValueError):
            M.compute_hausdorff_distance(yp, y, percentile=bad)
        with pytest.raises(ValueError):
            M.hausdorff_distance_numpy(p, g, bad)
        with pytest.raises(ValueError):
            M.surface_metrics_from_logits(yp, y.argmax(1, keepdim=True), 2, percentile=bad)
    with pytest.raises(NotImplementedError):
        M.HausdorffDistanceMetric(distance_metric="chessboard")
    with pytest.raises(NotImplementedError):
        M.compute_hausdorff_distance(yp, y, distance_metric="chessboard")
    with pytest.raises(ValueError):
        M.compute_hausdorff_distance(yp, y[:, :1])
    m = M.HausdorffDistanceMetric()
    assert (m.include_background, m.percentile, m.directed, m.reduction, m.get_not_nans) == (False, None, False, "mean", False)


def _three_samples():
    """class 1 present in pred and label (finite), class 2 predicted in sample 0 only and never labelled (inf there, NaN elsewhere), class 3
    nowhere (NaN)"""
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
    want = oracle_hd(onehot(pred, 4), onehot(lab, 4), 95, False)[:, 1:]
    assert np.isfinite(want[:, 0]).all() and math.isinf(want[0, 1]) and np.isnan(want[1:, 1]).all() and np.isnan(want[:, 2]).all()
    hd = M.HausdorffDistanceMetric(percentile=95, reduction="mean_batch", get_not_nans=True)
    b1 = hd(y_pred=yp[:2], y=y[:2])
    b2 = hd(y_pred=yp[2:], y=y[2:])
    assert b1.shape == (2, 3) and b2.shape == (1, 3) and b1.dtype == torch.float64
    same(hd.get_buffer().numpy(), want, rel=REL)
    agg, nn = hd.aggregate()
    assert agg[0].item() == pytest.approx(want[:, 0].mean(), rel=REL)
    assert math.isinf(agg[1].item()) and agg[2].item() == 0.0         # inf propagates, a class of NaNs alone reduces to 0 with no count
    assert nn.tolist() == [3.0, 1.0, 0.0]
    plain = M.HausdorffDistanceMetric(percentile=95)
    plain(y_pred=yp, y=y)
    assert isinstance(plain.aggregate(), torch.Tensor) and math.isinf(plain.aggregate().item())
    hd.reset()
    assert hd.get_buffer() is None


def test_from_logits_cpu_matches_the_oracle():
    pred, lab = random_case(8, (6, 7, 8), 5)
    logits = torch.randn(2, 5, 6, 7, 8)
    logits.scatter_(1, torch.from_numpy(pred)[:, None], 10.0)
    label = torch.from_numpy(lab)[:, None].to(torch.uint8)
    lists = oracle_lists(onehot(pred, 5), onehot(lab, 5))
    for inc in (True, False):
        asd, hd = M.surface_metrics_from_logits(logits, label, 5, include_background=inc, symmetric=True, percentile=95, directed=False)
        same(hd.numpy(), hd_from_lists(lists, (2, 5), 95, False)[:, 0 if inc else 1:], rel=REL)
        same(asd.numpy(), M.surface_distance_from_logits(logits, label, 5, include_background=inc, symmetric=True).numpy(), rel=0)
        one = M.hausdorff_distance_from_logits(logits, label, 5, include_background=inc, percentile=None, directed=True)
        same(one.numpy(), hd_from_lists(lists, (2, 5), None, True)[:, 0 if inc else 1:], rel=REL)


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
    assert "Hausdorff" not in out0
    ret1, res1 = run(hausdorff_distance=None)
    assert ret1 == ret0 and res1 == res0 and capsys.readouterr().out == out0
    hd = M.HausdorffDistanceMetric(include_background=False, percentile=95, reduction="mean_batch", get_not_nans=True)
    ret2, res2 = run(hausdorff_distance=hd)
    out2 = capsys.readouterr().out
    assert ret2 == ret0 and hd.get_buffer() is None                  # the return value does not change; the metric is reset
    assert set(res2) == set(res0) | {"hausdorff_distance_modality", "hausdorff_distance_total"}
    assert all(res2[k] == res0[k] for k in res0)
    assert "Hausdorff Distance per modality" in out2 and "val_total_hausdorff_distance/class1" in out2
    want = oracle_hd(onehot(preds, C), onehot(labs, C), 95, False)[:, 1:]
    tot, _ = M.do_metric_reduction(torch.from_numpy(want), "mean_batch")
    assert list(res2["hausdorff_distance_total"]) == [f"val_total_hausdorff_distance/class{c}" for c in range(1, C)]
    same(list(res2["hausdorff_distance_total"].values()), tot.numpy(), rel=REL)
    for m in (0, 1):
        sel = torch.from_numpy(want[[i for i in range(3) if i % 2 == m]])
        per, _ = M.do_metric_reduction(sel, "mean_batch")
        got = [res2["hausdorff_distance_modality"][f"val_modality{m}/class{c}"] for c in range(1, C)]
        same(got, per.numpy(), rel=REL)
        assert f"val_modality{m}/avg" in res2["hausdorff_distance_modality"]
