"""the fused average surface distance (csrc/surface.hip, miseg_surface_distance) at the bench.py --workload c5 volume size: a seeded synthetic
512 x 512 x 363 label of 6 classes (nested and overlapping ellipsoids, some cut by the volume border), the prediction a perturbed copy, fp32
logits.  Times the metric from logits with device events after warm-up (include_background True / False, symmetric), prints the bytes the
passes move (from the shapes and the class boxes), the share of HBM peak, and the CPU restatement's time on a cropped volume.
--combined [PERCENTILE] (default 95) also times the Hausdorff distance on the same kernels (miseg_surface_metrics): the
ASD + HD call, the HD-only call and their workspace next to the ASD call's; --dice [TOLERANCE] (default 2 voxels, every class) also times the
normalized surface Dice (miseg_surface_dice): ASD + HD + NSD in one call and the NSD alone, next to the ASD + HD call;
--no-cpu leaves out the CPU restatement."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import __graft_entry__ as ge

ge.load_package()
from mi_seg_amd.training import metrics as M

D, H, W, C = 363, 512, 512, 6
HBM_PEAK = 8.0e12            # MI355X HBM3E spec (6.29 TB/s measured with a float4 copy)


def ellipsoids(shape, specs, device):
    zz, yy, xx = (torch.arange(n, device=device, dtype=torch.float32) for n in shape)
    lab = torch.zeros(shape, dtype=torch.uint8, device=device)
    for c, ctr, r in specs:          # later ones paint over earlier ones: nested and overlapping structures
        e = ((zz.view(-1, 1, 1) - ctr[0]) / r[0]) ** 2 + ((yy.view(1, -1, 1) - ctr[1]) / r[1]) ** 2 + ((xx.view(1, 1, -1) - ctr[2]) / r[2]) ** 2 <= 1
        lab[e] = c
    return lab


def volume(device="cuda"):
    g = torch.Generator().manual_seed(0)
    specs = [(1, (180, 256, 256), (150, 220, 230)),        # the body: almost the whole volume
             (2, (120, 200, 180), (60, 80, 70)), (3, (250, 300, 330), (70, 90, 60)),
             (4, (190, 260, 250), (25, 30, 35)),           # nested inside 1, overlapping nothing else
             (5, (20, 480, 40), (60, 70, 80)),             # cut by three faces of the volume
             (2, (340, 60, 500), (40, 50, 30))]            # a second piece of class 2, on the border
    lab = ellipsoids((D, H, W), specs, device)
    jit = [(c, tuple(x + float(torch.randint(-4, 5, (1,), generator=g)) for x in ctr), tuple(x * (1 + 0.05 * float(torch.randn(1, generator=g))) for x in r))
           for c, ctr, r in specs]
    pred = ellipsoids((D, H, W), jit, device)
    flip = torch.rand((D, H, W), generator=g).to(device) < 0.002
    pred[flip] = torch.randint(0, C, (int(flip.sum()),), generator=g).to(device=device, dtype=torch.uint8)
    return pred, lab


def traffic(pred, lab, include_background):
    """bytes of one call: the classify pass over logits + label, then per (c, box) the W / H / D passes (both directions: int32 distances,
    packed stacks, edge bytes, class maps)"""
    S = D * H * W
    total = S * (C * 4 + 1 + 2)
    for c in range(0 if include_background else 1, C):
        u = (pred == c) | (lab == c)
        if not bool(u.any()):
            continue
        ext = []
        for ax in range(3):
            i = u.any(dim=tuple(d for d in range(3) if d != ax)).nonzero()
            ext.append(int(i.max() - i.min() + 1))
        vol = ext[0] * ext[1] * ext[2]
        total += vol * (2 + 1 + 2 * 4 * 3)        # W: class maps, edges, the two distance rows written twice and read once
        total += vol * 2 * 4 * 4                  # H: read, write, stack write + read
        total += vol * (2 * 4 * 3 + 2)            # D + gather: read, stack write + read, edge bytes
    return total


def median_ms(fn, warm=2, runs=5):
    for _ in range(warm):
        out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2], out


def combined(logits, label, pct):
    """ASD alone, ASD + HD in one call, HD alone: medians of 5, and the workspace of the two entry points"""
    from mi_seg_amd.hip import lib as L
    for inc in (True, False):
        kw = dict(include_background=inc, symmetric=True)
        asd_ms, asd = median_ms(lambda: M.surface_distance_from_logits(logits, label, C, **kw))
        both_ms, (asd2, hd) = median_ms(lambda: M.surface_metrics_from_logits(logits, label, C, percentile=pct, directed=False, **kw))
        hd_ms, _ = median_ms(lambda: M.hausdorff_distance_from_logits(logits, label, C, include_background=inc, percentile=pct))
        assert torch.equal(asd, asd2)
        print(f"include_background={inc!s:5}  ASD {asd_ms:7.2f} ms   ASD + HD{pct:g} in one call {both_ms:7.2f} ms (+{both_ms - asd_ms:5.2f})   "
              f"HD alone {hd_ms:7.2f} ms   ASD call + HD call {asd_ms + hd_ms:7.2f} ms   hd {[round(v, 3) for v in hd[0].tolist()]}")
    a, b = L.load().miseg_surface_distance_workspace_bytes(1, C, D, H, W), L.load().miseg_surface_metrics_workspace_bytes(1, C, D, H, W)
    print(f"workspace: ASD {a} bytes, ASD + HD {b} bytes (+{b - a} = {(b - a) // (2 * C)} per (class, direction))")


def dice(logits, label, pct, tau):
    """ASD + HD in one call, ASD + HD + NSD in one call, NSD alone: medians of 5, and the workspace of the three entry points"""
    from mi_seg_amd.hip import lib as L
    for inc in (True, False):
        kw = dict(include_background=inc, symmetric=True, percentile=pct, directed=False)
        taus = [tau] * (C - (0 if inc else 1))
        two_ms, (asd, hd) = median_ms(lambda: M.surface_metrics_from_logits(logits, label, C, **kw))
        three_ms, (asd2, hd2, nsd) = median_ms(lambda: M.surface_metrics_from_logits(logits, label, C, want=("asd", "hd", "nsd"), class_thresholds=taus, **kw))
        nsd_ms, nsd2 = median_ms(lambda: M.surface_dice_from_logits(logits, label, C, taus, include_background=inc))
        assert torch.equal(asd, asd2) and torch.equal(hd, hd2) and torch.equal(nsd, nsd2)
        print(f"include_background={inc!s:5}  ASD + HD{pct:g} {two_ms:7.2f} ms   ASD + HD{pct:g} + NSD in one call {three_ms:7.2f} ms (+{three_ms - two_ms:5.2f})   "
              f"NSD alone {nsd_ms:7.2f} ms   nsd(tau = {tau:g}) {[round(v, 4) for v in nsd[0].tolist()]}")
    a, b = L.load().miseg_surface_metrics_workspace_bytes(1, C, D, H, W), L.load().miseg_surface_dice_workspace_bytes(1, C, D, H, W)
    print(f"workspace: ASD + HD {a} bytes, ASD + HD + NSD {b} bytes (+{b - a})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dice", nargs="?", type=float, const=2.0, default=None, metavar="TOLERANCE")
    ap.add_argument("--combined", nargs="?", type=float, const=95.0, default=None, metavar="PERCENTILE")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    pred, lab = volume()
    logits = torch.nn.functional.one_hot(pred.long(), C).permute(3, 0, 1, 2).float()[None].contiguous()
    logits += 0.1 * torch.rand_like(logits)
    label = lab[None, None]
    for inc in (True, False):
        for _ in range(2):
            out = M.surface_distance_from_logits(logits, label, C, include_background=inc, symmetric=True)
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = M.surface_distance_from_logits(logits, label, C, include_background=inc, symmetric=True)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        ms = sorted(ts)[len(ts) // 2]
        nb = traffic(pred, lab, inc)
        print(f"include_background={inc!s:5}  {ms:8.2f} ms (median of 5)  {nb / 1e9:6.2f} GB  {nb / ms / 1e9:6.3f} TB/s = {100 * nb / ms / 1e9 / (HBM_PEAK / 1e12):5.1f} % "
              f"of HBM peak  asd {[round(v, 3) for v in out[0].tolist()]}")
    if args.combined is not None:
        combined(logits, label, args.combined)
    if args.dice is not None:
        dice(logits, label, args.combined if args.combined is not None else 95.0, args.dice)
    if args.no_cpu:
        return
    # the CPU restatement (scipy.ndimage when it imports: MONAI's recipe) on a crop, one thread
    crop = (slice(100, 228), slice(140, 268), slice(150, 246))
    p, g = pred[crop].cpu().numpy().astype(np.int64), lab[crop].cpu().numpy().astype(np.int64)
    cls = np.arange(C).reshape(1, C, 1, 1, 1)
    t0 = time.perf_counter()
    M.average_surface_distance_numpy(p[None, None] == cls, g[None, None] == cls, True)
    cpu = time.perf_counter() - t0
    n = p.size
    print(f"CPU restatement ({'scipy' if M._ndimage() is not None else 'numpy'}), include_background=True, crop {p.shape}: {cpu:.2f} s "
          f"({cpu / n * 1e9:.1f} ns per voxel; x{D * H * W / n:.0f} voxels for the whole volume)")


if __name__ == "__main__":
    main()
