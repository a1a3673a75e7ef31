"""the fill-holes filter (csrc/components.hip, miseg_fill_holes) at the prediction export's own workload: the 512 x 512 x
363 class map of 8 classes of bench_keep_largest.py (ellipsoid chambers plus 0.1 % speckle of random foreground classes - scattered wrong
voxels, most of them inside a chamber and so holes of it) with planted cavities: 3 x 3 x 3 cubes of background around random foreground voxels.
Times, with device events after warm-up (median of 5 runs): the whole call for all foreground labels; the call with no label applied (the
working map, the boxes and the output only) and with one label each, whose difference is that label's pass; the same call on a copy of the map
in which every label also has a voxel next to two opposite corners of the volume, so that every bounding box is the whole volume (what the
passes cost without the box confinement); miseg_keep_largest on the same map; and MONAI's scipy recipe on the host on a centre crop whose
size is printed (--host_crop, 0 skips it), whose result must equal the device's on that crop.  --host_full also runs the host recipe on the
whole map (about a minute on one core) and compares."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np
import torch
import __graft_entry__ as ge

ge.load_package()
from mi_seg_amd.hip import ops
from mi_seg_amd.training import postprocess as PP
from bench_keep_largest import C, SHAPE, heart_map

RUNS = 5


def planted(cls, cavities=4000, seed=1):
    """`cavities` cubes of 3 x 3 x 3 background voxels around random foreground voxels of the uint8 map [1, D, H, W]"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    centre = (torch.rand(cls.shape, device="cuda", generator=g) < cavities / cls.numel()) & (cls != 0)
    hole = centre
    for ax in (1, 2, 3):                                      # a centre's cube: one voxel to either side along every axis in turn
        grown = hole.clone()
        n = hole.shape[ax]
        grown.narrow(ax, 1, n - 1).logical_or_(hole.narrow(ax, 0, n - 1))
        grown.narrow(ax, 0, n - 1).logical_or_(hole.narrow(ax, 1, n - 1))
        hole = grown
    return torch.where(hole, torch.zeros_like(cls), cls).contiguous()


def whole_volume_boxes(cls):
    """the map with a voxel of every foreground label next to two opposite corners: every label's bounding box becomes the whole volume"""
    out = cls.clone()
    for c in range(1, C):
        out[0, 0, 0, c] = c
        out[0, -1, -1, -1 - c] = c
    return out


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
    ap = argparse.ArgumentParser()
    ap.add_argument("--host_crop", type=int, default=128, help="side of the centre crop the host recipe runs on (0: skip)")
    ap.add_argument("--host_full", action="store_true", help="also run the host recipe on the whole map and compare")
    ap.add_argument("--connectivity", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fill_holes: needs the HIP device (a CPU run times nothing)")
    conn = args.connectivity
    cls = planted(heart_map())
    fg = int((cls != 0).sum())
    print(f"class map {tuple(cls.shape[1:])} uint8, {C} classes, {fg} foreground voxels ({100 * fg / cls.numel():.2f} %), connectivity {conn}")
    out, stats = ops.fill_holes(pred=cls, num_classes=C, connectivity=conn, stats=True)
    print("voxels filled per label:", stats[0].tolist())
    ms, lo, hi = timed(lambda: ops.fill_holes(pred=cls, num_classes=C, connectivity=conn))
    print(f"miseg_fill_holes, labels 1..{C - 1}   {ms:8.3f} ms (median of {RUNS}; {lo:.3f}..{hi:.3f})")
    ms_s, lo_s, hi_s = timed(lambda: ops.fill_holes(pred=cls, num_classes=C, connectivity=conn, stats=True))
    print(f"  with statistics              {ms_s:8.3f} ms ({lo_s:.3f}..{hi_s:.3f})")
    ms_0, lo_0, hi_0 = timed(lambda: ops.fill_holes(pred=cls, num_classes=C, applied_labels=(), connectivity=conn))
    print(f"  no label applied             {ms_0:8.3f} ms ({lo_0:.3f}..{hi_0:.3f})  [working map, boxes, output]")
    for c in range(1, C):
        ms_c, lo_c, hi_c = timed(lambda: ops.fill_holes(pred=cls, num_classes=C, applied_labels=(c,), connectivity=conn))
        vox = int((cls == c).sum())
        print(f"  label {c} alone                {ms_c:8.3f} ms ({lo_c:.3f}..{hi_c:.3f})  pass = {ms_c - ms_0:6.3f} ms  [{vox} voxels of the label]")
    wide = whole_volume_boxes(cls)
    ms_w, lo_w, hi_w = timed(lambda: ops.fill_holes(pred=wide, num_classes=C, connectivity=conn))
    print(f"every box the whole volume     {ms_w:8.3f} ms ({lo_w:.3f}..{hi_w:.3f})  = {(ms_w - ms_0) / (C - 1):6.3f} ms per pass")
    ms_k, lo_k, hi_k = timed(lambda: ops.keep_largest_component(pred=cls, num_classes=C, connectivity=conn, independent=True))
    print(f"miseg_keep_largest, same map   {ms_k:8.3f} ms ({lo_k:.3f}..{hi_k:.3f})")
    ms_b, lo_b, hi_b = timed(lambda: ops.fill_holes(pred=ops.keep_largest_component(pred=cls, num_classes=C, connectivity=conn), num_classes=C, connectivity=conn))
    print(f"keep-largest, then fill-holes  {ms_b:8.3f} ms ({lo_b:.3f}..{hi_b:.3f})")
    if args.host_full:
        host = cls.cpu().numpy()
        t0 = time.perf_counter()
        want = PP.fill_holes_numpy(host, C, None, conn)
        t1 = time.perf_counter()
        print(f"host recipe on the whole map: {t1 - t0:8.1f} s (one core)  x{1e3 * (t1 - t0) / ms:.0f}; identical: {bool(np.array_equal(out.cpu().numpy(), want))}", flush=True)
    n = args.host_crop
    if n <= 0:
        return
    lo3 = [max((s - n) // 2, 0) for s in SHAPE]
    crop = cls[:, lo3[0]:lo3[0] + n, lo3[1]:lo3[1] + n, lo3[2]:lo3[2] + n].contiguous()
    host = crop.cpu().numpy()
    t0 = time.perf_counter()
    want = PP.fill_holes_numpy(host, C, None, conn)
    t1 = time.perf_counter()
    how = "scipy binary_dilation per label" if PP._ndimage() is not None else "numpy labelling per label"
    ms_d = timed(lambda: ops.fill_holes(pred=crop, num_classes=C, connectivity=conn))[0]
    got = ops.fill_holes(pred=crop, num_classes=C, connectivity=conn)
    print(f"host recipe on the centre crop {tuple(crop.shape[1:])}: {1e3 * (t1 - t0):8.0f} ms ({how}, one core); the device on that crop {ms_d:.3f} ms; "
          f"{int((want != host).sum())} voxels filled, identical: {bool(np.array_equal(got.cpu().numpy(), want))}")


if __name__ == "__main__":
    main()
