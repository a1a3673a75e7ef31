"""the device augmenter with Gaussian smoothing / sharpening behind the gather (csrc/gaussian.hip::miseg_gaussian_filter3d, DESIGN.md section
7.16) at the workload's size: patches of 96^3, one fp32 channel, patches_training_sample 1 and 2, out of a resident 256^3 volume.  Legs, all in
one process, timed with device events around REPS back-to-back calls after warm-up, alternating, median of RUNS:

  off       the augmenter with the options off: miseg_augment_crop alone, as it always was (the yardstick)
  smooth    + smooth on every sample at sigma 1.5 (radius 6): one filter call
  sharpen   + sharpen on every sample (sigma1 1.0, sigma2 0.5, alpha 20): two filter calls
  both      + both: three filter calls
  filter    one miseg_gaussian_filter3d call alone on the batch, at sigma 1.5 and at sigma 2.0 (radius 8)

The added cost of a leg is its time minus `off`'s."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import __graft_entry__ as ge

ge.load_package()
from mi_seg_amd.data.augment import GpuAugmenter, ResidentVolume, gaussian_filter

SIZE, ROI = (256, 256, 256), (96, 96, 96)
RUNS, WARMUP, REPS = 7, 2, 50


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def main():
    g = torch.Generator().manual_seed(0)
    vol = ResidentVolume(torch.rand((1,) + SIZE, generator=g).cuda(), torch.randint(0, 6, SIZE, generator=g).cuda())
    for n in (1, 2):
        aug = GpuAugmenter(ROI, patches_training_sample=n, seed=1)
        plain = [dict(origin=[16 * i, 32, 48], flip=[0, 1, 0], rot_k=i & 1, scale=0.05, shift=-0.02) for i in range(n)]
        smooth, sharpen = dict(smooth=(1.5, 1.5, 1.5)), dict(sharpen=((1.0, 1.0, 1.0), (0.5, 0.5, 0.5), 20.0))
        x = aug(vol, plain)["image"].clone()
        y = torch.empty_like(x)
        legs = {"off": lambda: aug(vol, plain),
                "smooth": lambda: aug(vol, [dict(p, **smooth) for p in plain]),
                "sharpen": lambda: aug(vol, [dict(p, **sharpen) for p in plain]),
                "both": lambda: aug(vol, [dict(p, **smooth, **sharpen) for p in plain]),
                "filter 1.5": lambda: gaussian_filter(x, (1.5, 1.5, 1.5), out=y),
                "filter 2.0": lambda: gaussian_filter(x, (2.0, 2.0, 2.0), out=y)}
        times = {k: [] for k in legs}
        for it in range(WARMUP + RUNS):
            for k, fn in legs.items():
                t = timed(fn)
                if it >= WARMUP:
                    times[k].append(t)
        med = {k: sorted(ts)[len(ts) // 2] for k, ts in times.items()}
        for k, ts in times.items():
            added = "" if k == "off" or k.startswith("filter") else f"  added {1e3 * (med[k] - med['off']):7.1f} us"
            print(f"n = {n}  {k:11s} {med[k] * 1e3:8.1f} us a call (median of {RUNS} x {REPS} calls; {min(ts) * 1e3:.1f}..{max(ts) * 1e3:.1f}){added}", flush=True)


if __name__ == "__main__":
    main()
