"""the weighted gather stitch (csrc/training.hip::stitch_weighted_kernel, MONAI mode="gaussian") against the constant stitch
(stitch_kernel) on the SAME resident buffer at the headline size: a 512 x 512 x 363 volume, 6 classes, 700 windows of 96^3 at overlap 0.5
(14.9 GB of fp32 window logits).  Both are timed in one process with device events after warm-up, alternating, median of 5, and reported
with the bytes model both share: every window value read once, every output value written once (the 3.5 MB map is cache traffic)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import __graft_entry__ as ge

ge.load_package()
from mi_seg_amd.hip import ops
from mi_seg_amd.training.inferer import _starts, importance_map

HBM_PEAK = 8.0e12            # MI355X HBM3E spec
SIZE, ROI, C, OVERLAP = (512, 512, 363), (96, 96, 96), 6, 0.5
RUNS, WARMUP = 5, 2


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    starts = tuple(_starts(s, r, OVERLAP) for s, r in zip(SIZE, ROI))
    n = len(starts[0]) * len(starts[1]) * len(starts[2])
    torch.manual_seed(0)
    win = torch.empty((n, C) + ROI, dtype=torch.float32, device="cuda").normal_()
    out = torch.empty((C,) + SIZE, dtype=torch.float32, device="cuda")
    wmap = importance_map(ROI, "gaussian", device="cuda")
    count = torch.empty(SIZE, dtype=torch.int16, device="cuda")
    ops.stitch_windows(win, out, starts, ROI, count=count)
    cover = torch.bincount(count.reshape(-1).long())
    nbytes = win.numel() * 4 + out.numel() * 4
    print(f"{n} windows of {ROI} x {C} classes = {win.numel() * 4 / 1e9:.2f} GB, output {out.numel() * 4 / 1e9:.2f} GB; "
          f"voxels covered by <= 8 windows: {100 * float(cover[:9].sum()) / count.numel():.1f} %, largest cover {int(count.max())}")
    legs = {"constant": lambda: ops.stitch_windows(win, out, starts, ROI), "gaussian": lambda: ops.stitch_windows(win, out, starts, ROI, weight=wmap)}
    times = {k: [] for k in legs}
    for it in range(WARMUP + RUNS):
        for k, fn in legs.items():
            t = once(fn)
            if it >= WARMUP:
                times[k].append(t)
    med = {}
    for k, ts in times.items():
        med[k] = sorted(ts)[len(ts) // 2]
        print(f"{k:9s} stitch {med[k]:8.3f} ms (median of {RUNS}; {min(ts):.3f}..{max(ts):.3f})  model {nbytes / 1e9:.2f} GB  "
              f"{nbytes / med[k] / 1e9:6.3f} TB/s = {100 * nbytes / med[k] / 1e9 / (HBM_PEAK / 1e12):5.1f} % of HBM peak")
    print(f"gaussian / constant: x{med['gaussian'] / med['constant']:.3f}")


if __name__ == "__main__":
    main()
