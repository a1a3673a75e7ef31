"""GPU tests of the Hausdorff distance on the surface-distance kernels (csrc/surface.hip, miseg_surface_metrics): the
kernel path against the oracle of test_hausdorff_cpu.py on every rule quirk and on small odd shapes from logits, lists whose two ranks fall
in different coarse bins of the radix select, the combined ASD + HD call against the ASD entry point bit for bit, a box with lines longer
than a wave against the CPU restatement, the metric objects on device vs CPU tensors, the evaluation loop with all three metrics, and the
C ABI's argument checks."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from surface_common import (DEV, REL, assert_results_match, assert_returns_match, bits_equal as _bits_equal, ops as _ops, swin_device_vs_replayed,
                            tied_logits as _tied_logits)
from test_hausdorff_cpu import PERCENTILES, hd_from_lists, oracle_lists
from test_surface_distance_cpu import onehot, quirk_cases, random_case, same

pytestmark = pytest.mark.gpu


def _check_class_maps(pred, gt, Cc, percentiles=PERCENTILES):
    """class maps [B, D, H, W] through ops.surface_metrics(pred=) against the oracle, percentiles x directed x include_background"""
    lists = oracle_lists(onehot(pred, Cc), onehot(gt, Cc))
    pc = torch.from_numpy(pred.astype(np.int32)).to(DEV)
    gc = torch.from_numpy(gt.astype(np.uint8)).to(DEV)
    for pct in percentiles:
        for directed in (False, True):
            want = hd_from_lists(lists, (pred.shape[0], Cc), pct, directed)
            for inc in (True, False):
                (got,) = _ops().surface_metrics(gc, pred=pc, num_classes=Cc, include_background=inc, percentile=pct, directed=directed, want=("hd",))
                assert got.dtype == torch.float64 and got.is_cuda
                same(got.cpu().numpy(), want[:, 0 if inc else 1:], rel=REL)
    return lists


@pytest.mark.parametrize("name,pred,gt,expect", quirk_cases(), ids=[c[0] for c in quirk_cases()])
def test_kernel_quirks_vs_oracle(name, pred, gt, expect):
    _check_class_maps(pred[:, 0].astype(np.int64), gt[:, 0].astype(np.int64), 2)


@pytest.mark.parametrize("shape", [(17, 19, 23), (33, 1, 40)])
@pytest.mark.parametrize("C", [2, 6])
def test_kernel_from_logits_vs_oracle(shape, C):
    """the prediction's stray voxels make every class box nearly the whole volume: every box is a group of its own"""
    pred, lab = random_case(10 + C, shape, C)
    lab[:, 0, 0, :3] = C                                     # labels outside [0, C) belong to no class
    logits = _tied_logits(pred, C, C).to(DEV)
    lists = oracle_lists(onehot(pred, C), onehot(lab, C))
    want = {(pct, d): hd_from_lists(lists, (2, C), pct, d) for pct in PERCENTILES for d in (False, True)}
    assert any(np.isfinite(w).any() for w in want.values())
    for dt in (torch.uint8, torch.int32, torch.int64, torch.float32):
        label = torch.from_numpy(lab)[:, None].to(dt).to(DEV)
        for (pct, directed), w in want.items():
            for inc in (True, False):
                (got,) = _ops().surface_metrics(label, logits=logits, include_background=inc, percentile=pct, directed=directed, want=("hd",))
                same(got.cpu().numpy(), w[:, 0 if inc else 1:], rel=REL)


def _radix_volume():
    g = np.zeros((1, 4, 6, 260), dtype=np.int64)
    p = np.zeros_like(g)
    g[0, 1:3, 1:5, 0:4] = 1
    p[0, 1:3, 1:5, 1:5] = 1
    p[0, 1:3, 1:5, 252:256] = 1
    return p, g


@pytest.mark.parametrize("form", ["as_is", "mirrored", "transposed"])
def test_ranks_in_different_coarse_bins(form):
    """d(P -> G): half of P's edge voxels lie within one voxel of G, the other half 248 to 252 voxels away: ranks 31 and 32 of the 64 sorted
    squared distances are 1 and 249^2 = 62001, in coarse bins 0 and 7 of the 13-bit radix select"""
    p, g = _radix_volume()
    lists = oracle_lists(onehot(p, 2), onehot(g, 2))
    pg = sorted(int(round(d * d)) for d in lists[0, 1][0])
    assert len(pg) == 64 and pg[31] == 1 and pg[32] == 62001 and (pg[31] >> 13) != (pg[32] >> 13) and (pg[-1] >> 13) > 0
    assert hd_from_lists(lists, (1, 2), 50, True)[0, 1] == 125.0
    assert hd_from_lists(lists, (1, 2), 95, True)[0, 1] == 252.0
    if form == "mirrored":
        p, g = g, p
    elif form == "transposed":                    # the long axis along D: each pass sees it
        p, g = np.ascontiguousarray(p.transpose(0, 3, 2, 1)), np.ascontiguousarray(g.transpose(0, 3, 2, 1))
        assert p.shape == (1, 260, 6, 4)
    lists = _check_class_maps(p, g, 2)
    if form != "mirrored":
        pc, gc = torch.from_numpy(p.astype(np.int32)).to(DEV), torch.from_numpy(g.astype(np.uint8)).to(DEV)
        for pct, expect in ((50, 125.0), (95, 252.0)):
            (got,) = _ops().surface_metrics(gc, pred=pc, num_classes=2, include_background=False, percentile=pct, directed=True, want=("hd",))
            assert got.item() == expect


def test_combined_call_shares_the_passes_bit_for_bit():
    pred, lab = random_case(16, (17, 19, 23), 6)
    logits = _tied_logits(pred, 6, 6).to(DEV)
    label = torch.from_numpy(lab)[:, None].to(torch.uint8).to(DEV)
    for sym in (True, False):
        for inc in (True, False):
            kw = dict(logits=logits, include_background=inc, symmetric=sym)
            asd, hd = _ops().surface_metrics(label, percentile=95, **kw)
            assert _bits_equal(asd, _ops().surface_distance(label, **kw))
            asd2, hd2 = _ops().surface_metrics(label, percentile=95, **kw)
            assert _bits_equal(hd, hd2) and _bits_equal(asd, asd2)
            (only,) = _ops().surface_metrics(label, percentile=95, want=("hd",), **kw)
            assert _bits_equal(hd, only)
            (only_asd,) = _ops().surface_metrics(label, percentile=95, want=("asd",), **kw)
            assert _bits_equal(asd, only_asd)
            hd3, asd3 = _ops().surface_metrics(label, percentile=95, want=("hd", "asd"), **kw)
            assert _bits_equal(hd3, hd) and _bits_equal(asd3, asd)
    assert torch.isfinite(hd).any() and torch.isfinite(asd).any()


def test_mid_size_box_vs_cpu_restatement():
    """96 x 112 x 80: lines longer than a wave on every axis, the background box the whole volume"""
    from mi_seg_amd.training import metrics as M
    pred, lab = random_case(21, (96, 112, 80), 4, B=1)
    logits = _tied_logits(pred, 4, 3).to(DEV)
    label = torch.from_numpy(lab)[:, None].to(torch.int64).to(DEV)
    for pct in (95, None):
        asd, hd = M.surface_metrics_from_logits(logits, label, 4, include_background=True, symmetric=True, percentile=pct, directed=False)
        want = M.hausdorff_distance_numpy(onehot(pred, 4), onehot(lab, 4), pct, False, use_scipy=True)
        assert np.isfinite(want).all()
        same(hd.cpu().numpy(), want, rel=REL)
        assert torch.equal(hd, M.hausdorff_distance_from_logits(logits, label, 4, include_background=True, percentile=pct, directed=False))
    assert torch.equal(asd, M.surface_distance_from_logits(logits, label, 4, include_background=True, symmetric=True))


def test_onehot_metrics_on_device_equal_the_cpu():
    from mi_seg_amd.training import metrics as M
    pred, lab = random_case(31, (20, 18, 22), 5, B=3)
    yp, y = torch.from_numpy(onehot(pred, 5)).float(), torch.from_numpy(onehot(lab, 5)).float()
    for inc in (True, False):
        for pct, directed in ((None, False), (95, False), (50, True)):
            out = {}
            for dev in ("cpu", DEV):
                hd = M.HausdorffDistanceMetric(include_background=inc, percentile=pct, directed=directed, reduction="mean_batch", get_not_nans=True)
                for i in range(3):
                    hd(y_pred=yp[i:i + 1].to(dev), y=y[i:i + 1].to(dev))
                out[dev] = (hd.aggregate(), hd.get_buffer())
                assert out[dev][1].device.type == torch.device(dev).type and out[dev][1].dtype == torch.float64
            same(out[DEV][1].cpu().numpy(), out["cpu"][1].numpy(), rel=REL)
            same(out[DEV][0][0].cpu().numpy(), out["cpu"][0][0].numpy(), rel=REL)
            assert torch.equal(out[DEV][0][1].cpu(), out["cpu"][0][1])


def test_evaluate_end_to_end_with_all_three_metrics():
    """the evaluation loop over four volumes of both modalities with Dice, surface distance and Hausdorff distance: fused on-device metrics
    (ASD and HD of a batch from one call, the two disagreeing on the background) vs the one-hot chain on the replayed CPU logits"""
    from mi_seg_amd.training import metrics as M
    C = 6
    (ret_dev, res_dev), (ret_cpu, res_cpu) = swin_device_vs_replayed(C, lambda: dict(
        surface_distance=M.SurfaceDistanceMetric(include_background=True, symmetric=True, reduction="mean_batch", get_not_nans=True),
        hausdorff_distance=M.HausdorffDistanceMetric(include_background=False, percentile=95, reduction="mean_batch", get_not_nans=True)))
    assert res_dev.keys() == res_cpu.keys() == {"dice_modality", "dice_total", "surface_distance_modality", "surface_distance_total",
                                                "hausdorff_distance_modality", "hausdorff_distance_total"}
    assert list(res_dev["hausdorff_distance_total"]) == [f"val_total_hausdorff_distance/class{c}" for c in range(1, C)]
    assert "val_modality1/avg" in res_dev["hausdorff_distance_modality"]
    assert_results_match(res_dev, res_cpu)
    assert_returns_match(ret_dev, ret_cpu)


def test_abi_rejects_bad_arguments():
    """every rejected call fails on the host side, before any launch"""
    from mi_seg_amd.hip import lib as L
    so = L.load()
    assert so.miseg_abi_version() == 16 and L.ABI_VERSION == 16
    logits = torch.zeros(1, 65, 4, 4, 4, device=DEV)
    label = torch.zeros(1, 4, 4, 4, dtype=torch.int32, device=DEV)
    asd = torch.empty(1, 65, dtype=torch.float64, device=DEV)
    hd = torch.empty(1, 65, dtype=torch.float64, device=DEV)
    nbytes = so.miseg_surface_metrics_workspace_bytes(1, 65, 4, 4, 4)
    assert nbytes > so.miseg_surface_distance_workspace_bytes(1, 65, 4, 4, 4)
    assert so.miseg_surface_metrics_workspace_bytes(1, 6, 0, 4, 4) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    p = L.SurfaceMetrics(C.sizeof(L.SurfaceMetrics) - 8, logits.data_ptr(), None, label.data_ptr(), L.LABEL_I32, 1, 65, 4, 4, 4, 1, 1,
                         ws.data_ptr(), asd.data_ptr(), hd.data_ptr(), 95.0, 0)
    assert so.miseg_surface_metrics(C.byref(p), None) == -1 and b"struct_size" in so.miseg_last_error()
    p.struct_size = C.sizeof(L.SurfaceMetrics)
    assert so.miseg_surface_metrics(C.byref(p), None) == -2          # C = 65
    p.C = 6
    p.percentile = 101.0
    assert so.miseg_surface_metrics(C.byref(p), None) == -1 and b"percentile" in so.miseg_last_error()
    p.percentile = math.nan
    assert so.miseg_surface_metrics(C.byref(p), None) == -1
    p.percentile = 95.0
    p.asd, p.hd = None, None
    assert so.miseg_surface_metrics(C.byref(p), None) == -1          # neither output
    p.hd = hd.data_ptr()
    p.logits = None
    assert so.miseg_surface_metrics(C.byref(p), None) == -1          # neither logits nor a class map
    with pytest.raises(ValueError):
        _ops().surface_metrics(label, logits=logits[:, :6].contiguous(), percentile=100.5)
    with pytest.raises(ValueError):
        _ops().surface_metrics(label, logits=logits[:, :6].contiguous(), want=("hd", "dice"))
