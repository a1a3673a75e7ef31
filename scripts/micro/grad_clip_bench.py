"""What gradient clipping and the non-finite guard cost in the captured training step: the headline C-Swin-UNETR step of bench.py's
secondary.c2_train_step_bf16 (refresh + forward + DiceFocal + backward + AdamW in one hipGraph, bf16, N = 1) in three arms

    off    everything off: the step as it was
    guard  skip_nonfinite: the two norm launches + the clipped kernels with the multiply off
    norm   gradient_clip_val: the two norm launches + the clipped kernels scaling every gradient

The arms share one model and one gradient arena (an optimiser and a set of graphs each), alternate in one process, and are timed with device
events around windows of --steps replays after --warmup; the figure of an arm is the median of its --windows windows.
Usage: python scripts/micro/grad_clip_bench.py [--windows 7] [--steps 20] [--warmup 5] [--clip 1.0] [--json out.json]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python scripts/micro/grad_clip_bench.py --windows 2` (a run of its own)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import __graft_entry__ as ge
ge.load_package()
import bench
from mi_seg_amd.runtime.arena import ParamArena
from mi_seg_amd.runtime.graph import GraphedTrainStep
from mi_seg_amd.training.losses import DiceFocalLoss
from mi_seg_amd.training.optim import ArenaOptimizer

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--clip", type=float, default=1.0, help="gradient_clip_val of the norm arm (Swin-UNETR recipes clip at 1)")
ap.add_argument("--json", type=str, default=None)
ap.add_argument("--arms", type=str, default="off,guard,norm", help="the order in which the arms are captured and timed")
a = ap.parse_args()

dtype = torch.bfloat16
model = bench.build_model(dtype, "c2")
params = [p for p in model.parameters() if p.requires_grad]
pool, mods = bench.synthetic_pool(16, 1000, "cuda")
labels = (pool * 6).floor().clamp_(0, 5).to(torch.int32)
arena = ParamArena(params, dtype)
crit = DiceFocalLoss(include_background=False, to_onehot_y=True, softmax=True, squared_pred=True, smooth_nr=0.0, smooth_dr=1e-6)
ARMS = {"off": {}, "guard": dict(skip_nonfinite=True), "norm": dict(gradient_clip_val=a.clip)}
ARMS = {n: ARMS[n] for n in a.arms.split(",")}
if sorted(ARMS) != ["guard", "norm", "off"]:
    raise SystemExit("--arms: a permutation of off,guard,norm")
steps = {}
for name, kw in ARMS.items():
    opt = ArenaOptimizer(arena, "adamw", lr=1e-4, weight_decay=1e-5, **kw)
    steps[name] = GraphedTrainStep(model, crit, opt, (1, 1, 96, 96, 96), (1, 1, 96, 96, 96), arena)
    for m_ in sorted(set(mods)):          # capture both graphs of the arm outside the timed region
        k = mods.index(m_)
        steps[name](pool[k:k + 1], labels[k:k + 1], [m_])
torch.cuda.synchronize()


def window(gts, first, n):
    for i in range(a.warmup):
        k = (first + i) % len(mods)
        gts(pool[k:k + 1], labels[k:k + 1], [mods[k]])
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(n):
        k = (first + a.warmup + i) % len(mods)
        loss = gts(pool[k:k + 1], labels[k:k + 1], [mods[k]])
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n, float(loss)


ms = {name: [] for name in ARMS}
for w in range(a.windows):
    for name in ARMS:                       # the arms alternate: drift of the device hits all of them alike
        t, loss = window(steps[name], w * 3, a.steps)
        if loss != loss:
            raise SystemExit(f"{name}: the loss is NaN")
        ms[name].append(t)
arena_bytes = arena.flat.numel() * 4
out = {"arena_bytes": arena_bytes, "parameters": len(params), "blocks": steps["norm"].opt._blocks, "steps_per_window": a.steps, "windows": a.windows,
       "ms_per_step": {n: {"median": statistics.median(v), "min": min(v), "max": max(v)} for n, v in ms.items()},
       "norm_arm": steps["norm"].opt.clip_stats(), "guard_arm": steps["guard"].opt.clip_stats()}
base = out["ms_per_step"]["off"]["median"]
for n in ("guard", "norm"):
    out["ms_per_step"][n]["over_off_us"] = 1000 * (out["ms_per_step"][n]["median"] - base)
    out["ms_per_step"][n]["over_off_percent"] = 100 * (out["ms_per_step"][n]["median"] / base - 1)
print(json.dumps(out), flush=True)
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
arena.detach()
