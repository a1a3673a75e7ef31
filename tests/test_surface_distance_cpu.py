"""Average surface distance (MONAI 1.1.0 compute_average_surface_distance, restated in training/metrics.py) and the cumulative metric objects
of the evaluation script, on the CPU: the numpy restatement against the scipy one and against a brute-force oracle written here from the
rules alone, every quirk of those rules, and do_metric_reduction.  No GPU."""
import math

import numpy as np
import pytest
import torch

from mi_seg_amd.training import metrics as M


# ------------------------------------------------------------------------------------------ brute-force oracle
def _edge_coords(m, lo, hi):
    """edge voxels of mask m (3-D) inside the box [lo, hi]: a voxel of m with a neighbour, along an axis on which the box is thicker than one
    voxel, that lies outside the box or outside m"""
    out = []
    keep = [a for a in range(3) if hi[a] > lo[a]]
    for v in zip(*np.nonzero(m)):
        for a in keep:
            for s in (-1, 1):
                n = list(v)
                n[a] += s
                if n[a] < lo[a] or n[a] > hi[a] or not m[tuple(n)]:
                    out.append(v)
                    break
            else:
                continue
            break
    return np.array(out, dtype=np.float64).reshape(-1, 3)


def _one_way(a, b):
    if len(b) == 0:
        return [math.inf] * len(a)
    if len(a) == 0:
        return [math.inf] * len(b)
    d = np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))
    return list(d.min(axis=1))


def oracle_asd(pred, gt, symmetric):
    """pred, gt: bool [B, C, D, H, W] -> float64 [B, C] by pairwise nearest-edge search"""
    B, Cc = pred.shape[:2]
    out = np.empty((B, Cc))
    for b in range(B):
        for c in range(Cc):
            p, g = pred[b, c], gt[b, c]
            u = p | g
            if not u.any():
                out[b, c] = math.nan
                continue
            idx = np.nonzero(u)
            lo, hi = [int(i.min()) for i in idx], [int(i.max()) for i in idx]
            ep, eg = _edge_coords(p, lo, hi), _edge_coords(g, lo, hi)
            d = _one_way(ep, eg) + (_one_way(eg, ep) if symmetric else [])
            out[b, c] = math.nan if not d else float(np.mean(d))
    return out


def same(a, b, rel=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    assert np.array_equal(np.isinf(a), np.isinf(b)), (a, b)
    f = np.isfinite(a)
    assert np.all(np.abs(a[f] - b[f]) <= rel * np.maximum(np.abs(b[f]), 1e-300)), (a[f], b[f])


def onehot(cls, C):
    """class map [B, D, H, W] -> bool [B, C, D, H, W] (values outside [0, C) in no channel)"""
    return cls[:, None] == np.arange(C).reshape(1, C, 1, 1, 1)


def random_case(seed, shape, C, B=2):
    """blobs of a few classes over a background, the prediction a perturbed copy: structures of every size, some on the border"""
    rng = np.random.default_rng(seed)
    lab = np.zeros((B,) + shape, dtype=np.int64)
    zz, yy, xx = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    for b in range(B):
        for c in range(1, C):
            if rng.random() < 0.2:
                continue                    # a class absent from this sample
            ctr = [rng.integers(0, n) for n in shape]
            r = [max(1, rng.integers(1, max(2, n // 2))) for n in shape]
            e = sum(((g - c0) / rr) ** 2 for g, c0, rr in zip((zz, yy, xx), ctr, r)) <= 1
            lab[b][e] = c
    pred = lab.copy()
    flip = rng.random(pred.shape) < 0.08
    pred[flip] = rng.integers(0, C, size=int(flip.sum()))
    return pred, lab


def quirk_cases():
    """(name, pred bool [1, 1, D, H, W], gt bool, expected symmetric ASD or None)"""
    cases = []

    def new(shape=(3, 30, 30)):
        return np.zeros((1, 1) + shape, bool), np.zeros((1, 1) + shape, bool)

    p, g = new()
    p[0, 0, 1, 4:17, 4:17] = True
    g[0, 0, 1, 1:15, 5:14] = True
    cases.append(("slab", p, g, 1.9831400619750137))        # 0.600 if the squeeze were skipped
    p, g = new((1, 1, 12))
    p[..., 2:7] = True
    g[..., 4:10] = True
    cases.append(("line", p, g, None))
    p, g = new((5, 5, 5))
    p[0, 0, 2, 2, 2] = True
    cases.append(("single_voxel_pred_only", p, g, math.nan))
    p, g = new((5, 5, 5))
    p[0, 0, 2, 2, 2] = g[0, 0, 2, 2, 2] = True
    cases.append(("single_voxel_both", p, g, math.nan))
    p, g = new((6, 7, 8))
    p[0, 0, 1:4, 2:6, 3:7] = True
    cases.append(("gt_empty", p, g, math.inf))
    cases.append(("pred_empty", g.copy(), p.copy(), math.inf))
    cases.append(("both_empty", g.copy(), g.copy(), math.nan))
    p, g = new((6, 7, 8))
    p[0, 0, 0:6, 0:3, 0:8] = True                           # touches five faces of the volume
    g[0, 0, 0:4, 0:5, 2:8] = True
    cases.append(("border", p, g, None))
    return cases


# ------------------------------------------------------------------------------------------ tests
def test_line_edges_are_the_two_ends():
    m = np.ones(5, bool)
    assert (M._erode(m) ^ m).astype(int).tolist() == [1, 0, 0, 0, 1]


@pytest.mark.parametrize("name,pred,gt,expect", quirk_cases(), ids=[c[0] for c in quirk_cases()])
@pytest.mark.parametrize("symmetric", [True, False])
def test_quirks_numpy_vs_oracle(name, pred, gt, expect, symmetric):
    got = M.average_surface_distance_numpy(pred, gt, symmetric, use_scipy=False)
    same(got, oracle_asd(pred, gt, symmetric))
    if symmetric and expect is not None:
        same(got, [[expect]])


def test_one_way_empty_rules():
    """d(P -> G) alone: G's edges empty => inf whenever P has edges; P's edges empty but G's not => inf too"""
    cases = {c[0]: c for c in quirk_cases()}
    assert math.isinf(M.average_surface_distance_numpy(cases["gt_empty"][1], cases["gt_empty"][2], False, use_scipy=False)[0, 0])
    assert math.isinf(M.average_surface_distance_numpy(cases["pred_empty"][1], cases["pred_empty"][2], False, use_scipy=False)[0, 0])
    assert math.isnan(M.average_surface_distance_numpy(cases["both_empty"][1], cases["both_empty"][2], False, use_scipy=False)[0, 0])


@pytest.mark.parametrize("seed,shape,C", [(0, (7, 9, 11), 3), (1, (5, 1, 12), 4), (2, (9, 8, 6), 6), (3, (1, 1, 9), 2)])
@pytest.mark.parametrize("symmetric", [True, False])
def test_numpy_vs_oracle_random(seed, shape, C, symmetric):
    pred, lab = random_case(seed, shape, C)
    same(M.average_surface_distance_numpy(onehot(pred, C), onehot(lab, C), symmetric, use_scipy=False),
         oracle_asd(onehot(pred, C), onehot(lab, C), symmetric))


@pytest.mark.parametrize("seed,shape,C", [(4, (12, 13, 14), 4), (5, (17, 1, 23), 6), (6, (20, 16, 18), 3)])
@pytest.mark.parametrize("symmetric", [True, False])
def test_numpy_vs_scipy(seed, shape, C, symmetric):
    pytest.importorskip("scipy")
    pred, lab = random_case(seed, shape, C)
    a = M.average_surface_distance_numpy(onehot(pred, C), onehot(lab, C), symmetric, use_scipy=False)
    b = M.average_surface_distance_numpy(onehot(pred, C), onehot(lab, C), symmetric, use_scipy=True)
    same(a, b)
    for _, p, g, _ in quirk_cases():
        same(M.average_surface_distance_numpy(p, g, symmetric, use_scipy=False), M.average_surface_distance_numpy(p, g, symmetric, use_scipy=True))


def test_compute_average_surface_distance_background_and_metric():
    pred, lab = random_case(7, (8, 9, 10), 4)
    yp, y = torch.from_numpy(onehot(pred, 4)).float(), torch.from_numpy(onehot(lab, 4)).float()
    full = M.compute_average_surface_distance(yp, y, include_background=True, symmetric=True)
    assert full.dtype == torch.float64 and full.shape == (2, 4)
    same(full.numpy(), oracle_asd(onehot(pred, 4), onehot(lab, 4), True))
    same(M.compute_average_surface_distance(yp, y, include_background=False, symmetric=True).numpy(), full.numpy()[:, 1:])
    with pytest.raises(NotImplementedError):
        M.compute_average_surface_distance(yp, y, distance_metric="chessboard")


def test_from_logits_cpu_matches_onehot_path():
    pred, lab = random_case(8, (6, 7, 8), 5)
    logits = torch.randn(2, 5, 6, 7, 8)
    logits.scatter_(1, torch.from_numpy(pred)[:, None], 10.0)
    label = torch.from_numpy(lab)[:, None].to(torch.uint8)
    for inc in (True, False):
        a = M.surface_distance_from_logits(logits, label, 5, include_background=inc, symmetric=True)
        same(a.numpy(), oracle_asd(onehot(pred, 5), onehot(lab, 5), True)[:, 0 if inc else 1:])


def test_do_metric_reduction_nan_and_inf():
    nan, inf = math.nan, math.inf
    f = torch.tensor([[1.0, nan, 3.0, nan], [3.0, nan, inf, 2.0], [5.0, nan, 1.0, nan]], dtype=torch.float64)
    m, n = M.do_metric_reduction(f, "mean_batch")
    assert m.tolist()[0] == 3.0 and m.tolist()[1] == 0.0 and math.isinf(m.tolist()[2]) and m.tolist()[3] == 2.0
    assert n.tolist() == [3.0, 0.0, 3.0, 1.0]
    m, n = M.do_metric_reduction(f, "none")
    assert torch.equal(torch.isnan(m), torch.isnan(f)) and n.tolist() == (~torch.isnan(f)).float().tolist()
    fin = torch.tensor([[1.0, nan, 3.0], [2.0, 4.0, nan]], dtype=torch.float64)
    m, n = M.do_metric_reduction(fin, "mean")
    assert m.item() == pytest.approx((2.0 + 3.0) / 2) and n.item() == 2.0
    m, n = M.do_metric_reduction(fin, "sum")
    assert m.item() == 10.0 and n.item() == 4.0
    m, n = M.do_metric_reduction(fin, "sum_batch")
    assert m.tolist() == [3.0, 4.0, 3.0] and n.tolist() == [2.0, 1.0, 1.0]
    assert math.isinf(M.do_metric_reduction(f, "mean")[0].item())
    with pytest.raises(ValueError):
        M.do_metric_reduction(fin, "median")


def test_cumulative_metrics_aggregate():
    pred, lab = random_case(9, (6, 8, 7), 4, B=3)
    yp, y = torch.from_numpy(onehot(pred, 4)).float(), torch.from_numpy(onehot(lab, 4)).float()
    sd = M.SurfaceDistanceMetric(include_background=False, symmetric=True, reduction="mean_batch", get_not_nans=True)
    dm = M.DiceMetric(include_background=False, reduction="mean_batch", get_not_nans=True)
    b1 = sd(y_pred=yp[:2], y=y[:2])
    b2 = sd(y_pred=yp[2:], y=y[2:])
    assert b1.shape == (2, 3) and b2.shape == (1, 3)
    dm(y_pred=yp[:2], y=y[:2])
    dm(y_pred=yp[2:], y=y[2:])
    want = oracle_asd(onehot(pred, 4), onehot(lab, 4), True)[:, 1:]
    same(sd.get_buffer().numpy(), want)
    agg, nn = sd.aggregate()
    ref, refn = M.do_metric_reduction(torch.from_numpy(want), "mean_batch")
    same(agg.numpy(), ref.numpy())
    assert nn.tolist() == refn.tolist()
    assert sd.aggregate(reduction="none")[0].shape == (3, 3)
    d = M.dice_metric(yp, y)[:, 1:]
    dagg, dn = dm.aggregate()
    assert torch.allclose(dagg, M.do_metric_reduction(d, "mean_batch")[0], equal_nan=True)
    sd.reset()
    assert sd.get_buffer() is None
    c = M.Cumulative()
    c.extend(torch.ones(2, 3), torch.tensor([0, 1]))
    c.extend(torch.zeros(1, 3), torch.tensor([1]))
    v, mod = c.get_buffer()
    assert v.shape == (3, 3) and mod.tolist() == [0, 1, 1]
