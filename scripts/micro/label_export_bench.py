"""the prediction export (csrc/training.hip, miseg_label_export) at the MM-WHS CT size: a 512 x 512 x 363 uint16 label map in an oblique
LPS-like file grid from 8-class fp32 logits on the 180 x 180 x 164 resampled RAS grid plus a pad.  Times the kernel call (tables prebuilt,
as predict.py's inverse does once per volume) against the device-side composition of existing pieces (crop copy, torch.argmax, miseg_resample3d
nearest on int32, permute / flip copy, LUT index, cast) with device events after warm-up, median of several runs, and prints a bytes model
next to each."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import __graft_entry__ as ge

ge.load_package()
from mi_seg_amd.data.nifti import ras_orientation
from mi_seg_amd.data.preprocess import PredictionGeometry, resample
from mi_seg_amd.hip import ops
from mi_seg_amd.training.predict import label_lut

HBM_PEAK = 8.0e12            # MI355X HBM3E spec
C = 8
RUNS = 9


def geometry():
    # the file's X runs along -x (L), Y along -y (P) with a small in-plane rotation: the LPS-like scanner grid
    A = np.array([[-0.7 * 0.98, 0.7 * 0.17, 0.0, 120.0], [-0.7 * 0.17, -0.7 * 0.98, 0.0, 95.5], [0.0, 0.0, 0.45, -210.0], [0, 0, 0, 1.0]])
    order, flips = ras_orientation(A)
    file_shape = (512, 512, 363)
    ras = tuple(file_shape[a] for a in order)
    resampled = (180, 180, 164)
    pb, pa = (0, 0, 2), (0, 0, 2)
    return PredictionGeometry(file_shape, A, order, flips, ras, resampled, pb, pa)


def composition(logits, g, lut):
    cls = logits[(slice(None),) + tuple(slice(b, b + m) for b, m in zip(g.pad_before, g.resampled_shape))].contiguous()
    cls = cls.argmax(0).to(torch.int32)
    cls = resample(cls[None], g.ras_shape, "nearest")[0]
    flips = [k for k in range(3) if g.flips[k]]
    cls = cls.flip(flips) if flips else cls
    cls = cls.permute(*np.argsort(g.order).tolist()[::-1]).contiguous()       # [Z, Y, X]: the file's Fortran order
    return lut[cls.long()].to(torch.int16)


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def main():
    g = geometry()
    torch.manual_seed(0)
    logits = torch.randn((C,) + g.padded_shape, device="cuda")
    lut = label_lut(C).cuda()
    tables, axes = g.index_tables("cuda")
    out_vox = int(np.prod(g.file_shape))
    box = int(np.prod(g.resampled_shape))
    print(f"file {g.file_shape} order {g.order} flips {g.flips}; logits {C} x {g.padded_shape} fp32 ({logits.numel() * 4 / 1e6:.0f} MB)")
    # kernel: pass 1 reads the box's logits, writes the uint8 class map; pass 2 reads the class map (L2 / MALL-resident), writes uint16
    k_bytes = box * (C * 4 + 1) + box + out_vox * 2
    ms, lo, hi = timed(lambda: ops.label_export(logits, tables, axes, lut))
    print(f"miseg_label_export      {ms:8.3f} ms (median of {RUNS}; {lo:.3f}..{hi:.3f})  model {k_bytes / 1e9:5.3f} GB  "
          f"{k_bytes / ms / 1e9:6.3f} TB/s = {100 * k_bytes / ms / 1e9 / (HBM_PEAK / 1e12):5.1f} % of HBM peak")
    # composition: crop copy (r+w), argmax (r fp32, w int64), int32 cast (r int64, w int32), resample (r, w int32 full size), permute / flip
    # copy (r+w int32), LUT index (r int32 -> int64 index, gather, w int64), cast (r int64, w int16)
    c_bytes = (box * C * 4 * 2 + box * C * 4 + box * 8 + box * (8 + 4) + box * 4 + out_vox * 4 + out_vox * 4 * 2 + out_vox * (4 + 8)
               + out_vox * (8 + 8) + out_vox * (8 + 2))
    ms2, lo2, hi2 = timed(lambda: composition(logits, g, lut))
    print(f"device composition      {ms2:8.3f} ms (median of {RUNS}; {lo2:.3f}..{hi2:.3f})  model {c_bytes / 1e9:5.3f} GB  "
          f"{c_bytes / ms2 / 1e9:6.3f} TB/s")
    got = ops.label_export(logits, tables, axes, lut).view(torch.int16)
    want = composition(logits, g, lut)
    print("bit-identical:", bool(torch.equal(got, want)), f"  speed-up x{ms2 / ms:.1f}")


if __name__ == "__main__":
    main()
