"""GPU tests of the average surface distance kernels (csrc/surface.hip, reference test.py:145-151) and of the evaluation loop built on them
(training/evaluate.py, reference test.py:46-123): the kernel path against the brute-force oracle of test_surface_distance_cpu.py on small odd
shapes and every rule quirk, against the CPU restatement on a large box with the background class, run-to-run bit equality, the cumulative
metric objects on device vs CPU tensors, an end-to-end evaluation, and the C ABI's argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

from surface_common import DEV, REL, assert_results_match, assert_returns_match, ops as _ops, swin_device_vs_replayed, tied_logits as _tied_logits
from test_surface_distance_cpu import oracle_asd, onehot, quirk_cases, random_case, same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,pred,gt,expect", quirk_cases(), ids=[c[0] for c in quirk_cases()])
def test_kernel_quirks_vs_oracle(name, pred, gt, expect):
    pc = torch.from_numpy(pred[:, 0].astype(np.int32)).to(DEV)
    gc = torch.from_numpy(gt[:, 0].astype(np.uint8)).to(DEV)
    for sym in (True, False):
        want = oracle_asd(onehot(pred[:, 0].astype(np.int64), 2), onehot(gt[:, 0].astype(np.int64), 2), sym)
        for inc in (True, False):
            got = _ops().surface_distance(gc, pred=pc, num_classes=2, include_background=inc, symmetric=sym)
            assert got.dtype == torch.float64 and got.is_cuda
            same(got.cpu().numpy(), want[:, 0 if inc else 1:], rel=REL)
        if sym and expect is not None:
            same(want[:, 1:], [[expect]])


@pytest.mark.parametrize("shape", [(17, 19, 23), (33, 1, 40)])
@pytest.mark.parametrize("C", [2, 6, 14])
def test_kernel_from_logits_vs_oracle(shape, C):
    pred, lab = random_case(10 + C, shape, C)
    lab[:, 0, 0, :3] = C                                     # labels outside [0, C) belong to no class
    logits = _tied_logits(pred, C, C).to(DEV)
    lab_oh = onehot(lab, C)
    want = {sym: oracle_asd(onehot(pred, C), lab_oh, sym) for sym in (True, False)}
    for dt in (torch.uint8, torch.int32, torch.int64, torch.float32):
        label = torch.from_numpy(lab)[:, None].to(dt).to(DEV)
        for sym in (True, False):
            for inc in (True, False):
                got = _ops().surface_distance(label, logits=logits, include_background=inc, symmetric=sym)
                same(got.cpu().numpy(), want[sym][:, 0 if inc else 1:], rel=REL)
    again = _ops().surface_distance(label, logits=logits, include_background=True, symmetric=True)
    assert torch.equal(again, _ops().surface_distance(label, logits=logits, include_background=True, symmetric=True))


def test_large_box_with_background_vs_cpu_restatement():
    """160 x 192 x 128: lines of 128..192 voxels, the background box the whole volume"""
    from mi_seg_amd.training import metrics as M
    pred, lab = random_case(21, (160, 192, 128), 4, B=1)
    logits = _tied_logits(pred, 4, 3).to(DEV)
    label = torch.from_numpy(lab)[:, None].to(torch.int64).to(DEV)
    got = M.surface_distance_from_logits(logits, label, 4, include_background=True, symmetric=True)
    want = M.average_surface_distance_numpy(onehot(pred, 4), onehot(lab, 4), True)
    same(got.cpu().numpy(), want, rel=REL)
    assert np.isfinite(want).all()
    assert torch.equal(got, M.surface_distance_from_logits(logits, label, 4, include_background=True, symmetric=True))


def test_onehot_metrics_on_device_equal_the_cpu():
    from mi_seg_amd.training import metrics as M
    pred, lab = random_case(31, (20, 18, 22), 5, B=3)
    yp, y = torch.from_numpy(onehot(pred, 5)).float(), torch.from_numpy(onehot(lab, 5)).float()
    for inc in (True, False):
        out = {}
        for dev in ("cpu", DEV):
            sd = M.SurfaceDistanceMetric(include_background=inc, symmetric=True, reduction="mean_batch", get_not_nans=True)
            dm = M.DiceMetric(include_background=inc, reduction="mean_batch", get_not_nans=True)
            for i in range(3):
                sd(y_pred=yp[i:i + 1].to(dev), y=y[i:i + 1].to(dev))
                dm(y_pred=yp[i:i + 1].to(dev), y=y[i:i + 1].to(dev))
            out[dev] = (sd.aggregate(), dm.aggregate(), sd.get_buffer())
            assert out[dev][2].device.type == torch.device(dev).type
        same(out[DEV][2].cpu().numpy(), out["cpu"][2].numpy(), rel=REL)
        same(out[DEV][0][0].cpu().numpy(), out["cpu"][0][0].numpy(), rel=REL)
        assert torch.equal(out[DEV][0][1].cpu(), out["cpu"][0][1])
        assert torch.allclose(out[DEV][1][0].cpu(), out["cpu"][1][0], rtol=1e-6, equal_nan=True)


def test_evaluate_end_to_end_matches_the_loop_on_cpu_logits():
    """the reference's test() loop over four volumes of both modalities: fused on-device metrics vs the one-hot chain on the CPU logits"""
    from mi_seg_amd.training import metrics as M
    (ret_dev, res_dev), (ret_cpu, res_cpu) = swin_device_vs_replayed(6, lambda: dict(
        surface_distance=M.SurfaceDistanceMetric(include_background=True, symmetric=True, reduction="mean_batch", get_not_nans=True)))
    assert res_dev.keys() == res_cpu.keys() == {"dice_modality", "dice_total", "surface_distance_modality", "surface_distance_total"}
    assert "val_modality1/avg" in res_dev["surface_distance_modality"] and "val_modality0/avg" in res_dev["dice_modality"]
    assert_results_match(res_dev, res_cpu)
    assert_returns_match(ret_dev, ret_cpu)


def test_abi_rejects_bad_arguments():
    from mi_seg_amd.hip import lib as L
    so = L.load()
    logits = torch.zeros(1, 65, 4, 4, 4, device=DEV)
    label = torch.zeros(1, 4, 4, 4, dtype=torch.int32, device=DEV)
    asd = torch.empty(1, 65, dtype=torch.float64, device=DEV)
    ws = torch.empty(so.miseg_surface_distance_workspace_bytes(1, 65, 4, 4, 4), dtype=torch.uint8, device=DEV)
    p = L.SurfaceDistance(C.sizeof(L.SurfaceDistance) - 8, logits.data_ptr(), None, label.data_ptr(), L.LABEL_I32, 1, 65, 4, 4, 4, 1, 1,
                          ws.data_ptr(), asd.data_ptr())
    assert so.miseg_surface_distance(C.byref(p), None) == -1 and b"struct_size" in so.miseg_last_error()
    p.struct_size = C.sizeof(L.SurfaceDistance)
    assert so.miseg_surface_distance(C.byref(p), None) == -2
    p.C, p.logits = 6, None
    assert so.miseg_surface_distance(C.byref(p), None) == -1       # neither logits nor a class map
