"""the keep-largest-connected-component filter (csrc/components.hip, miseg_keep_largest) at the prediction export's own
workload: a 512 x 512 x 363 class map of 8 classes, connectivity 3, every foreground class on its own.  The map is a synthetic heart-like
volume (data/synthetic.py's ellipsoids, built at a quarter of the size and enlarged) plus 0.1 % speckle of random foreground classes - the
stray islands the filter is there to remove.  Times the call with device events after warm-up (median of several runs) and prints, next to it,
the bytes a lean count of the six passes moves and the share of the HBM rate that implies, the time of miseg_label_export producing the same
volume (for scale), and the time of the host restatement (scipy.ndimage.label per class) on the same map, whose result must be identical.
--no_host skips the host restatement (tens of seconds on one core)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts", "micro"))
import numpy as np
import torch
import __graft_entry__ as ge

ge.load_package()
from mi_seg_amd.data.synthetic import synthetic_volume
from mi_seg_amd.hip import ops
from mi_seg_amd.training import postprocess as PP
from mi_seg_amd.training.predict import label_lut

HBM_PEAK = 8.0e12            # MI355X HBM3E spec
SHAPE = (512, 512, 363)
C = 8
RUNS = 9


def heart_map(shape=SHAPE, speckle=1e-3, seed=0):
    """uint8 [1, D, H, W] on the device: ellipsoid chambers + `speckle` of the voxels set to a random foreground class"""
    q = tuple((s + 3) // 4 for s in shape)
    _, label = synthetic_volume(q, seed, n_classes=C)
    cls = label[0, 0].to(torch.uint8)
    for ax in range(3):
        cls = cls.repeat_interleave(4, dim=ax)
    cls = cls[:shape[0], :shape[1], :shape[2]].contiguous().cuda()
    g = torch.Generator(device="cuda").manual_seed(seed)
    hit = torch.rand(shape, device="cuda", generator=g) < speckle
    noise = torch.randint(1, C, shape, device="cuda", generator=g, dtype=torch.uint8)
    return torch.where(hit, noise, cls)[None].contiguous()


def lean_bytes(cls):
    """what the six passes have to move: every pass reads the uint8 map; parent / size are touched at applied voxels only"""
    vox = cls.numel()
    applied = int((cls != 0).sum())
    per_voxel = 2 + 1 + 1 + 1 + 1 + 2             # classify r+w, local r, merge r, flatten r, select r, apply r+w (uint8 out)
    per_applied = 8 + 12 + 4 + 4                   # local: parent + size out; flatten: parent in / out + size in; select, apply: parent in
    return vox * per_voxel + applied * per_applied, applied


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
    ap.add_argument("--no_host", action="store_true", help="skip the host restatement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_keep_largest: needs the HIP device (a CPU run times nothing)")
    cls = heart_map()
    nbytes, applied = lean_bytes(cls)
    print(f"class map {tuple(cls.shape[1:])} uint8, {C} classes, {applied} foreground voxels ({100 * applied / cls.numel():.2f} %)")
    run = lambda: ops.keep_largest_component(pred=cls, num_classes=C, connectivity=3, independent=True)
    ms, lo, hi = timed(run)
    print(f"miseg_keep_largest      {ms:8.3f} ms (median of {RUNS}; {lo:.3f}..{hi:.3f})  lean model {nbytes / 1e9:5.3f} GB  "
          f"{nbytes / ms / 1e9:6.3f} TB/s = {100 * nbytes / ms / 1e9 / (HBM_PEAK / 1e12):5.1f} % of HBM peak")
    out, stats = ops.keep_largest_component(pred=cls, num_classes=C, connectivity=3, independent=True, stats=True)
    st = stats[0].cpu()
    print("components per class:", st[:, 2].tolist(), " voxels removed per class:", (st[:, 0] - st[:, 1]).tolist())
    ms_s, lo_s, hi_s = timed(lambda: ops.keep_largest_component(pred=cls, num_classes=C, connectivity=3, independent=True, stats=True))
    print(f"  with statistics       {ms_s:8.3f} ms ({lo_s:.3f}..{hi_s:.3f})")
    ms_j, lo_j, hi_j = timed(lambda: ops.keep_largest_component(pred=cls, num_classes=C, connectivity=3, independent=False))
    print(f"  joint mode            {ms_j:8.3f} ms ({lo_j:.3f}..{hi_j:.3f})")
    # for scale: the export of the same volume (label_export_bench.py's geometry: 8-class logits on the 180 x 180 x 168 grid -> 512 x 512 x 363)
    from label_export_bench import geometry
    g = geometry()
    logits = torch.randn((C,) + g.padded_shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    tables, axes = g.index_tables("cuda")
    lut = label_lut(C).cuda()
    ms_e, lo_e, hi_e = timed(lambda: ops.label_export(logits, tables, axes, lut))
    print(f"miseg_label_export      {ms_e:8.3f} ms ({lo_e:.3f}..{hi_e:.3f})  [{C} x {g.padded_shape} logits -> {g.file_shape} uint16]")
    if args.no_host:
        return
    host = cls.cpu().numpy()
    t0 = time.perf_counter()
    want = PP.keep_largest_numpy(host, C, None, True, 3)
    t1 = time.perf_counter()
    how = "scipy.ndimage.label per class" if PP._ndimage() is not None else "numpy labelling per class"
    print(f"host restatement        {1e3 * (t1 - t0):8.0f} ms ({how}, one core; without the device-to-host copy)  x{1e3 * (t1 - t0) / ms:.0f}")
    print("identical to the host restatement:", bool(np.array_equal(out.cpu().numpy(), want)))


if __name__ == "__main__":
    main()
