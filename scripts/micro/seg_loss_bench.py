"""the fused segmentation losses (csrc/training.hip, miseg_seg_loss_fwd / miseg_seg_loss_bwd: dice_focal, dice_ce, gdice_focal) and the Dice
metric pass (miseg_dice_metric, with and without the generalized Dice score) at the headline shape (B = 1, C = 6, 96^3, fp32 logits, int32
labels) and at the reference's out_channels = 8 MM-WHS shape.

Each (op, kind) is captured once as a hipGraph of REPS back-to-back calls, so a timed window holds REPS launches and no host time; the
windows of the kinds alternate round by round inside one process, device events around each replay, warm-up first, median over the rounds
(min and max are printed as the spread).  Bytes are algorithmic, from the shapes: the forward reads logits + labels, the backward reads them
again and writes dlogits, the metric reads logits + labels; TB/s is bytes over the median time (the HBM achieves 6.3 TB/s on a float4 copy,
and 21 MB of logits fit the 256 MB last-level cache, so a figure above that is cache bandwidth).

--kinds restricts the loss kinds and --no-score leaves the score out (a build without them can then be timed by the same script)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import __graft_entry__ as ge

ge.load_package()
from mi_seg_amd.hip import lib as L
from mi_seg_amd.hip import ops

REPS = 50          # calls inside one timed window
ROUNDS = 21
SHAPES = [("headline", 1, 6, 96), ("mm-whs", 1, 8, 96)]


def make_cfg(kind):
    if kind == "dice_focal":
        return ops.SegLossCfg(L.LOSS_DICE_FOCAL, False, True, 0.0, 1e-6)
    if kind == "dice_ce":
        return ops.SegLossCfg(L.LOSS_DICE_CE, False, True, 0.0, 1e-6, 0.0)
    return ops.SegLossCfg(L.LOSS_GDICE_FOCAL, False, False, 0.0, 1e-6, 2.0, 1.0, 1.0, L.GDICE_W_SQUARE)


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            fn()
    return g


def measure(graphs):
    """graphs: {name: CUDAGraph}; -> {name: (median, min, max) us per call}"""
    for g in graphs.values():
        for _ in range(3):
            g.replay()
    torch.cuda.synchronize()
    ts = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e3 / REPS)
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ts.items()}


def shape(name, B, C, side, kinds, score):
    g = torch.Generator().manual_seed(side + C)
    logits = (3.0 * torch.randn(B, C, side, side, side, generator=g)).cuda()
    labels = torch.randint(0, C, (B, 1, side, side, side), generator=g).to(torch.int32).cuda()
    gscale = torch.full((), 1.0, device="cuda")
    S = side ** 3
    read = 4 * B * S * (C + 1)
    nbytes = {"fwd": read, "bwd": read + 4 * B * S * C, "metric": read}
    graphs, keep = {}, []
    for kind in kinds:
        cfg = make_cfg(kind)
        _, sums = ops.seg_loss_fwd(logits, labels, cfg)
        keep.append(sums)
        graphs[f"{kind} fwd"] = capture(lambda cfg=cfg: ops.seg_loss_fwd(logits, labels, cfg))
        graphs[f"{kind} bwd"] = capture(lambda cfg=cfg, sums=sums: ops.seg_loss_bwd(logits, labels, cfg, sums, gscale))
    graphs["dice metric"] = capture(lambda: ops.dice_metric(logits, labels))
    if score:
        graphs["dice + score metric"] = capture(lambda: ops.dice_metric(logits, labels, gdice=(False, "square")))
    print(f"{name}: B {B} C {C} {side}^3 fp32 logits, int32 labels; {REPS} calls per window, {ROUNDS} rounds")
    for k, (med, lo, hi) in measure(graphs).items():
        nb = nbytes["metric" if "metric" in k else k.split()[-1]]
        print(f"  {k:22s} {med:7.2f} us (min {lo:7.2f} max {hi:7.2f})  {nb / 1e6:6.1f} MB  {nb / med / 1e6:5.2f} TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="dice_focal,dice_ce,gdice_focal")
    ap.add_argument("--no-score", action="store_true")
    a = ap.parse_args()
    print(torch.cuda.get_device_name(0))
    for s in SHAPES:
        shape(*s, kinds=a.kinds.split(","), score=not a.no_score)


if __name__ == "__main__":
    main()
