"""GPU tests of the normalized surface Dice on the surface-distance kernels (csrc/surface.hip, miseg_surface_dice): the
kernel path against the oracle of test_surface_dice_cpu.py (the rule applied to brute-force lists) on every rule quirk and on small odd shapes
from logits with several groups of boxes, lines longer and shorter than a wave, every label dtype, a mid-size box against the scipy
restatement, the three-metric call against the existing entry points bit for bit, the clamp of a very large tolerance, the metric object on
device vs CPU tensors, the evaluation loop with all four metrics (plain and behind keep-largest / fill-holes), and the C ABI's argument
checks.  Every surface-Dice comparison is exact."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

from surface_common import (DEV, assert_results_match, assert_returns_match, bits_equal as _bits_equal, ops as _ops, swin_device_vs_replayed,
                            tied_logits as _tied_logits)
from test_hausdorff_cpu import oracle_lists
from test_surface_dice_cpu import QUIRKS, THRESHOLDS, case, class_taus, exact, nsd_from_lists
from test_surface_distance_cpu import onehot, random_case

pytestmark = pytest.mark.gpu


def _nsd(label, taus, inc, **kw):
    (got,) = _ops().surface_metrics(label, include_background=inc, want=("nsd",), class_thresholds=taus[0 if inc else 1:], **kw)
    assert got.dtype == torch.float64 and got.is_cuda
    return got.cpu().numpy()


@pytest.mark.parametrize("name", QUIRKS)
def test_kernel_quirks_vs_oracle(name):
    pred, gt, Cc, p, g, lists = case(name)
    pc = torch.from_numpy(pred.astype(np.int32)).to(DEV)
    gc = torch.from_numpy(gt.astype(np.uint8)).to(DEV)
    for shift in range(len(THRESHOLDS)):
        taus = class_taus(Cc, shift)
        want = nsd_from_lists(lists, (1, Cc), taus)
        for inc in (True, False):
            exact(_nsd(gc, taus, inc, pred=pc, num_classes=Cc), want[:, 0 if inc else 1:])


@pytest.mark.parametrize("name", ["random_b", "random_a", "random_c"])
def test_kernel_from_logits_vs_oracle(name):
    """tied logits; with the background and scattered flips every class's box is near the whole volume, so random_a ((17, 19, 23), C = 6,
    B = 2) runs several groups of boxes; random_c ((8, 33, 70)) has lines longer and shorter than a wave"""
    pred, lab, Cc, p, g, lists = case(name)
    logits = _tied_logits(pred, Cc, Cc).to(DEV)
    label = torch.from_numpy(lab)[:, None].to(torch.uint8).to(DEV)
    if name == "random_a":
        vols = [np.prod([i.max() - i.min() + 1 for i in np.nonzero(p[b, c] | g[b, c])]) for b in range(2) for c in range(Cc) if (p[b, c] | g[b, c]).any()]
        assert sum(vols) > 2 * 17 * 19 * 23                # more voxels of boxes than one group holds
    seen = set()
    for shift in range(len(THRESHOLDS)):
        taus = class_taus(Cc, shift)
        want = nsd_from_lists(lists, p.shape[:2], taus)
        seen.update(want[np.isfinite(want)].tolist())
        for inc in (True, False):
            exact(_nsd(label, taus, inc, logits=logits), want[:, 0 if inc else 1:])
    assert len(seen) > 3


def test_class_map_form_and_label_dtypes():
    pred, lab, Cc, p, g, lists = case("random_b")
    lab = lab.copy()
    lab[:, 0, 0, :3] = Cc                                    # labels outside [0, C) belong to no class
    pred = pred.copy()
    pred[:, 1, 1, :2] = -1                                   # and class-map values likewise
    taus = class_taus(Cc, 2)
    want = nsd_from_lists(oracle_lists(onehot(pred, Cc), onehot(lab, Cc)), p.shape[:2], taus)
    pc = torch.from_numpy(pred.astype(np.int32)).to(DEV)
    for dt in (torch.uint8, torch.int32, torch.int64, torch.float32):
        label = torch.from_numpy(lab)[:, None].to(dt).to(DEV)
        for inc in (True, False):
            exact(_nsd(label, taus, inc, pred=pc, num_classes=Cc), want[:, 0 if inc else 1:])
            exact(_nsd(label, taus, inc, pred=pc[:, None].long(), num_classes=Cc), want[:, 0 if inc else 1:])


def test_mid_size_box_vs_cpu_restatement():
    """96 x 112 x 80: lines longer than a wave on every axis, the background box the whole volume"""
    from mi_seg_amd.training import metrics as M
    pred, lab = random_case(21, (96, 112, 80), 4, B=1)
    logits = _tied_logits(pred, 4, 3).to(DEV)
    label = torch.from_numpy(lab)[:, None].to(torch.int64).to(DEV)
    taus = class_taus(4, 1)
    want = M.surface_dice_numpy(onehot(pred, 4), onehot(lab, 4), taus, use_scipy=True)
    assert np.isfinite(want).all() and len(set(want.reshape(-1).tolist())) == 4
    got = M.surface_dice_from_logits(logits, label, 4, taus, include_background=True)
    exact(got.cpu().numpy(), want)
    exact(M.surface_dice_from_logits(logits, label, 4, taus[1:], include_background=False).cpu().numpy(), want[:, 1:])


def test_three_metric_call_shares_the_passes_bit_for_bit():
    pred, lab, Cc, p, g, lists = case("random_a")
    logits = _tied_logits(pred, Cc, Cc).to(DEV)
    label = torch.from_numpy(lab)[:, None].to(torch.uint8).to(DEV)
    taus = class_taus(Cc, 3)
    for sym in (True, False):
        for inc in (True, False):
            t = taus[0 if inc else 1:]
            kw = dict(logits=logits, include_background=inc, symmetric=sym, percentile=95)
            asd, hd, nsd = _ops().surface_metrics(label, want=("asd", "hd", "nsd"), class_thresholds=t, **kw)
            assert _bits_equal(asd, _ops().surface_distance(label, logits=logits, include_background=inc, symmetric=sym))
            asd0, hd0 = _ops().surface_metrics(label, **kw)
            assert _bits_equal(asd, asd0) and _bits_equal(hd, hd0)
            (only,) = _ops().surface_metrics(label, want=("nsd",), class_thresholds=t, **kw)
            assert _bits_equal(nsd, only)
            exact(nsd.cpu().numpy(), nsd_from_lists(lists, p.shape[:2], taus)[:, 0 if inc else 1:])
            for order in itertools.permutations(("asd", "hd", "nsd")):
                got = dict(zip(order, _ops().surface_metrics(label, want=order, class_thresholds=t, **kw)))
                assert _bits_equal(got["asd"], asd) and _bits_equal(got["hd"], hd) and _bits_equal(got["nsd"], nsd)
            for pair in (("asd", "nsd"), ("nsd", "hd")):
                got = dict(zip(pair, _ops().surface_metrics(label, want=pair, class_thresholds=t, **kw)))
                assert all(_bits_equal(got[k], {"asd": asd, "hd": hd, "nsd": nsd}[k]) for k in pair)
    assert torch.isfinite(hd).any() and torch.isfinite(asd).any() and torch.isfinite(nsd).any()


@pytest.mark.parametrize("name", ["random_a", "gt_empty", "pred_empty", "both_empty", "slab"])
def test_very_large_tolerance_counts_every_real_distance(name):
    """a finite tolerance above every distance: 1.0 wherever both edge sets are non-empty, 0.0 where one is empty (the no-seed value of the
    distance passes lies above the clamped bound), NaN where both are"""
    pred, gt, Cc, p, g, lists = case(name)
    want = np.empty(p.shape[:2])
    for (b, c), (pg, gp) in lists.items():
        want[b, c] = math.nan if not pg and not gp else 0.0 if math.isinf(pg[0]) else 1.0
    if name == "random_a":
        assert (want == 1.0).any() and (want == 0.0).any()
    pc = torch.from_numpy(pred.astype(np.int32)).to(DEV)
    gc = torch.from_numpy(gt.astype(np.uint8)).to(DEV)
    for tau in (1e300, 1.7e308, 8192.0, 4096.0 * math.sqrt(3.0)):
        exact(_nsd(gc, [tau] * Cc, True, pred=pc, num_classes=Cc), want)


def test_onehot_metric_on_device_equals_the_cpu():
    from mi_seg_amd.training import metrics as M
    pred, lab = random_case(31, (20, 18, 22), 5, B=3)
    yp, y = torch.from_numpy(onehot(pred, 5)).float(), torch.from_numpy(onehot(lab, 5)).float()
    for inc in (True, False):
        taus = class_taus(5, 4)[0 if inc else 1:]
        out = {}
        for dev in ("cpu", DEV):
            nsd = M.SurfaceDiceMetric(taus, include_background=inc, reduction="mean_batch", get_not_nans=True)
            for i in range(3):
                nsd(y_pred=yp[i:i + 1].to(dev), y=y[i:i + 1].to(dev))
            out[dev] = (nsd.aggregate(), nsd.get_buffer())
            assert out[dev][1].device.type == torch.device(dev).type and out[dev][1].dtype == torch.float64
        exact(out[DEV][1].cpu().numpy(), out["cpu"][1].numpy())
        exact(out[DEV][0][0].cpu().numpy(), out["cpu"][0][0].numpy())
        assert torch.equal(out[DEV][0][1].cpu(), out["cpu"][0][1])
        assert len(set(out["cpu"][1][torch.isfinite(out["cpu"][1])].tolist())) > 3


def test_evaluate_end_to_end_with_all_four_metrics():
    """the evaluation loop over four volumes of both modalities with Dice, surface distance, Hausdorff distance and surface Dice: fused
    on-device metrics (ASD, HD and NSD of a batch from one call, the three disagreeing on the background) vs the one-hot chain on the replayed
    CPU logits; the surface-Dice parts exact"""
    from mi_seg_amd.training import metrics as M
    Cc = 6
    calls = []
    ops = _ops()
    real = ops.surface_metrics

    def counted(*a, **kw):
        calls.append(tuple(kw.get("want", ())))
        return real(*a, **kw)

    ops.surface_metrics = counted
    try:
        (ret_dev, res_dev), (ret_cpu, res_cpu) = swin_device_vs_replayed(Cc, lambda: dict(
            surface_distance=M.SurfaceDistanceMetric(include_background=True, symmetric=True, reduction="mean_batch", get_not_nans=True),
            hausdorff_distance=M.HausdorffDistanceMetric(include_background=False, percentile=95, reduction="mean_batch", get_not_nans=True),
            surface_dice=M.SurfaceDiceMetric(class_taus(Cc, 0)[1:], include_background=False, reduction="mean_batch", get_not_nans=True)))
    finally:
        ops.surface_metrics = real
    assert calls == [("asd", "hd", "nsd")] * 4             # ONE call per batch on the device, none for the replayed CPU logits
    assert res_dev.keys() == res_cpu.keys() == {"dice_modality", "dice_total", "surface_distance_modality", "surface_distance_total",
                                                "hausdorff_distance_modality", "hausdorff_distance_total", "surface_dice_modality",
                                                "surface_dice_total"}
    assert list(res_dev["surface_dice_total"]) == [f"val_total_surface_dice/class{c}" for c in range(1, Cc)]
    assert "val_modality1/avg" in res_dev["surface_dice_modality"]
    assert_results_match(res_dev, res_cpu)
    assert_returns_match(ret_dev, ret_cpu)


def test_evaluate_filtered_path_takes_the_metric():
    """evaluate.test(keep_largest=, fill_holes=, surface_dice=) on device logits (fused: the one filtered class map feeds ASD, HD and NSD in ONE
    call) against the same call on the replayed CPU logits (the one-hot chain with the transforms inside); the surface-Dice parts exact"""
    from mi_seg_amd.training import evaluate as E
    from mi_seg_amd.training import metrics as M
    from mi_seg_amd.training import postprocess as PP
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
    seen, calls = [], []
    ops = _ops()
    real = ops.surface_metrics

    def counted(*a, **kw):
        calls.append((tuple(kw.get("want", ())), kw.get("pred") is not None))
        return real(*a, **kw)

    def on_device(x, modalities=None):
        seen.append(model(x).detach())
        return seen[-1]

    def run(device, inferer):
        res = {}
        E.test(model, loader, device, M.DiceMetric(include_background=True, reduction="mean_batch", get_not_nans=True), E.AsDiscrete(to_onehot=Cc),
               E.AsDiscrete(argmax=True, to_onehot=Cc), model_inferer=inferer, amp=False,
               surface_distance=M.SurfaceDistanceMetric(include_background=False, symmetric=True, reduction="mean_batch", get_not_nans=True),
               hausdorff_distance=M.HausdorffDistanceMetric(include_background=False, percentile=95, reduction="mean_batch", get_not_nans=True),
               surface_dice=M.SurfaceDiceMetric(class_taus(Cc, 1), include_background=True, reduction="mean_batch", get_not_nans=True),
               results=res, keep_largest=PP.KeepLargestConnectedComponent(connectivity=1), fill_holes=PP.FillHoles())
        return res

    ops.surface_metrics = counted
    try:
        res_dev = run(DEV, on_device)
    finally:
        ops.surface_metrics = real
    assert calls == [(("asd", "hd", "nsd"), True)] * 2      # ONE call per batch, on the filtered class map
    replay = iter([s.cpu() for s in seen])
    res_cpu = run("cpu", lambda x, modalities=None: next(replay))
    assert res_dev.keys() == res_cpu.keys() and "surface_dice_total" in res_dev
    assert list(res_dev["surface_dice_total"]) == [f"val_total_surface_dice/class{c}" for c in range(Cc)]
    vals = list(res_dev["surface_dice_total"].values())
    assert len(set(vals)) == Cc and all(0.0 < v < 1.0 for v in vals)
    assert_results_match(res_dev, res_cpu)


def test_abi_rejects_bad_arguments():
    """every rejected call fails on the host side, before any launch"""
    from mi_seg_amd.hip import lib as L
    so = L.load()
    assert so.miseg_abi_version() == 16 and L.ABI_VERSION == 16
    assert so.miseg_abi_struct_size(b"miseg_surface_dice_params") == C.sizeof(L.SurfaceDice) > C.sizeof(L.SurfaceMetrics)
    for f, _ in L.SurfaceMetrics._fields_:                   # the fields of miseg_surface_metrics_params come first
        assert getattr(L.SurfaceDice, f).offset == getattr(L.SurfaceMetrics, f).offset
    logits = torch.zeros(1, 6, 4, 4, 4, device=DEV)
    label = torch.zeros(1, 4, 4, 4, dtype=torch.int32, device=DEV)
    out = [torch.empty(1, 6, dtype=torch.float64, device=DEV) for _ in range(3)]
    nbytes = so.miseg_surface_dice_workspace_bytes(1, 6, 4, 4, 4)
    assert nbytes > so.miseg_surface_metrics_workspace_bytes(1, 6, 4, 4, 4) > so.miseg_surface_distance_workspace_bytes(1, 6, 4, 4, 4)
    assert so.miseg_surface_dice_workspace_bytes(1, 6, 0, 4, 4) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    taus = (C.c_double * 6)(*[1.0] * 6)
    p = L.SurfaceDice(C.sizeof(L.SurfaceMetrics), logits.data_ptr(), None, label.data_ptr(), L.LABEL_I32, 1, 6, 4, 4, 4, 1, 1,
                      ws.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), 95.0, 0, out[2].data_ptr(), taus)
    assert so.miseg_surface_dice(C.byref(p), None) == -1 and b"struct_size" in so.miseg_last_error()
    p.struct_size = C.sizeof(L.SurfaceDice)
    assert so.miseg_surface_dice(C.byref(p), None) == 0
    p.thresholds = None
    assert so.miseg_surface_dice(C.byref(p), None) == -1 and b"thresholds" in so.miseg_last_error()
    for bad in (-1.0, -5e-324, math.nan, math.inf, -math.inf):
        p.thresholds = (C.c_double * 6)(1.0, 1.0, 1.0, bad, 1.0, 1.0)
        assert so.miseg_surface_dice(C.byref(p), None) == -1 and b"thresholds[3]" in so.miseg_last_error()
    p.thresholds = taus
    p.asd, p.hd, p.nsd = None, None, None
    assert so.miseg_surface_dice(C.byref(p), None) == -1      # no output at all
    p.nsd = out[2].data_ptr()
    assert so.miseg_surface_dice(C.byref(p), None) == 0       # the surface Dice alone
    p.C = 65
    assert so.miseg_surface_dice(C.byref(p), None) == -2
    p.C = 6
    p.D = 4097
    assert so.miseg_surface_dice(C.byref(p), None) == -2
    p.D = 4
    p.hd, p.percentile = out[1].data_ptr(), 101.0
    assert so.miseg_surface_dice(C.byref(p), None) == -1 and b"percentile" in so.miseg_last_error()
    x = logits.contiguous()
    with pytest.raises(ValueError):
        _ops().surface_metrics(label, logits=x, want=("nsd",))
    with pytest.raises(ValueError):
        _ops().surface_metrics(label, logits=x, want=("nsd",), class_thresholds=[1.0] * 5)
    with pytest.raises(ValueError):
        _ops().surface_metrics(label, logits=x, want=("nsd",), class_thresholds=[1.0] * 5 + [-1.0])
    with pytest.raises(ValueError, match="'asd', 'hd', 'nsd'"):
        _ops().surface_metrics(label, logits=x, want=("nsd", "dice"), class_thresholds=[1.0] * 6)
