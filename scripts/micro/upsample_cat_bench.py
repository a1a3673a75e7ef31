"""the C-UNet decoder step (csrc/elementwise.hip, miseg_upsample_cat / miseg_upsample_cat_bwd) at the four decoder levels of the published
model (feature_size 16 64 128 256 512, strides 1 2 2 2 1) on a 96^3 patch in bf16: the fused forward and backward against the torch
composition of reference unet_vanilla.py:162-169 (F.interpolate(mode="nearest") + torch.cat on NCDHW, backward by autograd).  Device
events after warm-up, median of several runs; the algorithmic bytes (each input read once, each output written once) over the median time
against the 6.3 TB/s the HBM achieves.  Checks that the forward outputs are identical and reports the largest backward difference.

--model adds one figure: eager forward + backward patches/s of the published C-UNet at B = 1, 96^3, bf16 (no optimiser step)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import torch.nn.functional as F
import __graft_entry__ as ge

ge.load_package()
from mi_seg_amd.hip import ops

HBM = 6.3e12                 # achievable MI355X HBM bandwidth (float4 copy)
RUNS = 15
# (fine side, skip channels, upsampled channels, factor) of up_path.3 .. up_path.0 at a 96^3 patch
LEVELS = [(96, 16, 64, 2), (48, 64, 128, 2), (24, 128, 256, 2), (12, 256, 512, 1)]


def timed(fn, runs=RUNS):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return sorted(ts)[len(ts) // 2]


def rate(nbytes, us):
    return f"{us:8.1f} us {nbytes / us / 1e3:7.0f} GB/s {100 * nbytes / us / 1e-6 / HBM:5.1f} %"


def level(side, cs, cu, f):
    torch.manual_seed(side)
    dt = torch.bfloat16
    c = side // f
    skip = torch.randn(1, side, side, side, cs, device="cuda").to(dt)             # channels-last, as the model holds them
    x = torch.randn(1, c, c, c, cu, device="cuda").to(dt)
    dcat = torch.randn(1, side, side, side, cs + cu, device="cuda").to(dt)
    skip_n = skip.permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)       # NCDHW, as the reference holds them
    x_n = x.permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
    dcat_n = dcat.permute(0, 4, 1, 2, 3).contiguous()
    es = 2
    fwd_bytes = es * (skip.numel() + x.numel() + dcat.numel())
    bwd_bytes = es * (side ** 3 * cu + x.numel())                               # right half of dcat read, dx written (skip: a view)

    def torch_fwd():
        return torch.cat((skip_n, F.interpolate(x_n, scale_factor=f, mode="nearest")), dim=1)

    out_t = torch_fwd()

    def torch_bwd():
        return torch.autograd.grad(out_t, (skip_n, x_n), dcat_n, retain_graph=True)

    right = dcat[..., cs:]
    t_ff = timed(lambda: ops.upsample_cat(skip, x, f))
    t_tf = timed(torch_fwd)
    t_fb = timed(lambda: ops.upsample_cat_bwd(right, f))
    t_tb = timed(torch_bwd)
    same = torch.equal(ops.upsample_cat(skip, x, f), out_t.detach().permute(0, 2, 3, 4, 1))
    dx_f = ops.upsample_cat_bwd(right, f).float()
    dx_t = torch_bwd()[1].permute(0, 2, 3, 4, 1).float()
    diff = float((dx_f - dx_t).abs().max())
    print(f"{side:3d}^3 Cs {cs:3d} Cu {cu:3d} f {f}: fwd {fwd_bytes / 1e6:6.1f} MB  fused {rate(fwd_bytes, t_ff)}  torch {rate(fwd_bytes, t_tf)}"
          f"  x{t_tf / t_ff:4.1f}  identical {same}")
    print(f"{'':24s}bwd {bwd_bytes / 1e6:6.1f} MB  fused {rate(bwd_bytes, t_fb)}  torch {rate(bwd_bytes, t_tb)}  x{t_tb / t_fb:4.1f}"
          f"  max |diff| {diff:.3g}")
    return t_ff + t_fb, t_tf + t_tb


def model_rate():
    from mi_seg_amd.networks.nets.unet_vanilla import UNetVanilla
    from mi_seg_amd.networks.norms.utils import parse_normalization
    from mi_seg_amd.utils.detfill import det_input, fill_module_
    m = UNetVanilla(3, 1, 8, channels=[16, 64, 128, 256, 512], strides=[1, 2, 2, 2, 1], num_res_units=3,
                    norm_down=parse_normalization("instance_cond", True, 4, 2), norm_up=parse_normalization("instance", True, 4, 2))
    fill_module_(m)
    m = m.cuda().set_compute_dtype(torch.bfloat16)
    x, cot = det_input(1, (1, 1, 96, 96, 96)).cuda(), det_input(2, (1, 8, 96, 96, 96)).cuda()

    def step():
        m.zero_grad(set_to_none=True)
        m(x, [0]).backward(cot)

    ms = timed(step, runs=7) / 1e3
    print(f"published C-UNet, B=1 96^3 bf16, eager forward + backward: {ms:.1f} ms = {1e3 / ms:.2f} patches/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", action="store_true")
    a = ap.parse_args()
    tf = tt = 0.0
    for lv in LEVELS:
        f_us, t_us = level(*lv)
        tf, tt = tf + f_us, tt + t_us
    print(f"four levels fwd + bwd: fused {tf:.1f} us, torch {tt:.1f} us")
    if a.model:
        model_rate()


if __name__ == "__main__":
    main()
