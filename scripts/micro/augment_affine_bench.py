"""the device augmenter with rotation / zoom, gamma and noise (csrc/augment.hip::miseg_augment_affine) at the
headline size: n = 4 patches of 96^3 out of a resident 512 x 512 x 363 volume (one fp32 channel, int64 labels).  Four legs in one process,
timed with device events around REPS back-to-back calls after warm-up, alternating, median of RUNS:

  crop      miseg_augment_crop, the integer gather as it always was
  identity  miseg_augment_affine with identity matrices, no gamma, no noise (the same gather through the new entry point)
  full      miseg_augment_affine with rotation + zoom + translation, gamma and noise on every sample (two launches)
  torch     the same chain in torch on the device: one grid_sample per sample for the image (bilinear, border) and one for the label
            (nearest), amin / amax / pow, the scale and shift, randn noise

The bytes model is the output alone - every patch value written once: image 4 B + label 8 B a voxel (`full` writes the image twice and reads
it once more, which the model does not count); the gathered input is at most as much again and mostly cache traffic for the rotated reads."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import __graft_entry__ as ge

ge.load_package()
from mi_seg_amd.data.augment import GpuAugmenter, ResidentVolume, affine_matrix, augment_affine

SIZE, ROI, N = (512, 512, 363), (96, 96, 96), 4
RUNS, WARMUP, REPS = 7, 2, 20


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def torch_chain(vol, params, base):
    """the restatement a torch user would write: per sample a sampling grid in the volume's normalised coordinates, two grid_samples, the
    intensity chain; flips and the quarter turn are left out (they would only add passes)"""
    D, H, W = vol.label.shape
    size = torch.tensor([D - 1, H - 1, W - 1], dtype=torch.float32, device="cuda")
    image, label = vol.image[None], vol.label[None, None].float()
    imgs, labs = [], []
    for p in params:
        a = torch.from_numpy(p["affine"]).cuda()
        centre = torch.tensor([o + (r - 1) / 2 for o, r in zip(p["origin"], ROI)], dtype=torch.float32, device="cuda")
        s = base @ a[:, :3].T + (a[:, 3] + centre)                                  # [rd, rh, rw, 3] positions in the volume
        grid = (2 * s / size - 1).flip(-1)[None]                                     # (x, y, z) = (W, H, D)
        v = torch.nn.functional.grid_sample(image, grid, mode="bilinear", padding_mode="border", align_corners=True)[0]
        labs.append(torch.nn.functional.grid_sample(label, grid, mode="nearest", padding_mode="border", align_corners=True)[0].long())
        lo, hi = v.amin(), v.amax()
        v = ((v - lo) / (hi - lo + 1e-7)) ** p["gamma"] * (hi - lo) + lo
        v = v * (1 + p["scale"]) + p["shift"]
        imgs.append(v + (p["noise"][0] + p["noise"][1] * torch.randn_like(v)))
    return torch.stack(imgs), torch.stack(labs)


def main():
    g = torch.Generator().manual_seed(0)
    image = torch.rand((1,) + SIZE, generator=g).cuda()
    label = torch.randint(0, 6, SIZE, generator=g).cuda()
    vol = ResidentVolume(image, label)
    aug = GpuAugmenter(ROI, patches_training_sample=N, seed=1)
    rng = np.random.default_rng(0)
    plain = [dict(origin=[int(rng.integers(0, s - r + 1)) for s, r in zip(SIZE, ROI)], flip=[0, 0, 0], rot_k=0, scale=0.05, shift=-0.02) for _ in range(N)]
    full = [dict(p, affine=np.concatenate([affine_matrix(rng.uniform(-0.3, 0.3, 3), rng.uniform(0.8, 1.25, 3)), rng.uniform(-3, 3, (3, 1)).astype(np.float32)], 1),
                 gamma=float(rng.uniform(0.5, 2.0)), noise=(0.0, 0.05)) for p in plain]
    scratch = torch.zeros(64, dtype=torch.int32, device="cuda")
    out_i = torch.empty((N, 1) + ROI, dtype=torch.float32, device="cuda")
    out_l = torch.empty((N, 1) + ROI, dtype=torch.int64, device="cuda")
    zz, yy, xx = torch.meshgrid(*(torch.arange(r, dtype=torch.float32, device="cuda") - (r - 1) / 2 for r in ROI), indexing="ij")
    base = torch.stack([zz, yy, xx], -1)
    legs = {"crop": lambda: aug(vol, plain),
            "identity": lambda: augment_affine(image, label, ROI, plain, out_image=out_i, out_label=out_l),
            "full": lambda: augment_affine(image, label, ROI, full, seed=3, draw=5, minmax=scratch, out_image=out_i, out_label=out_l),
            "torch": lambda: torch_chain(vol, full, base)}
    a, b = aug(vol, plain), augment_affine(image, label, ROI, plain)
    assert torch.equal(a["image"], b[0]) and torch.equal(a["label"], b[1])           # the identity leg is the crop leg, bit for bit
    times = {k: [] for k in legs}
    for it in range(WARMUP + RUNS):
        for k, fn in legs.items():
            t = timed(fn)
            if it >= WARMUP:
                times[k].append(t)
    nbytes = N * ROI[0] * ROI[1] * ROI[2] * (4 + 8)
    med = {}
    for k, ts in times.items():
        med[k] = sorted(ts)[len(ts) // 2]
        print(f"{k:9s} {med[k] * 1e3:9.1f} us a call (median of {RUNS} x {REPS} calls; {min(ts) * 1e3:.1f}..{max(ts) * 1e3:.1f})  output {nbytes / 1e6:.1f} MB  "
              f"{nbytes / med[k] / 1e6:7.1f} GB/s")
    print(f"identity / crop x{med['identity'] / med['crop']:.3f}   full / crop x{med['full'] / med['crop']:.3f}   torch / full x{med['torch'] / med['full']:.2f}")
    assert int(scratch.abs().sum()) == 0


if __name__ == "__main__":
    main()
