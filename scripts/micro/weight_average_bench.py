"""What weight averaging on the device costs, on the headline C-Swin-UNETR of bench.py's secondary.c2_train_step_bf16
(bf16, N = 1, one 96^3 patch per step):

    kernels  miseg_weight_average (an applying call with n > 0: reads the weights and the average, writes the average) and
             miseg_weight_swap (reads and writes both) over the model's whole arena, and - the yardstick, in the same process -
             miseg_grad_fold op 3 (acc = acc + g), which moves the same three arena-sized transfers as the averaging call
    step     GraphedTrainStep patches/s with averaging off, every step and every 4th step: the arms named in --arms share one model and
             one arena (an optimiser, an averager and a graph each).  In a captured step the weights the averaging launch reads were
             written by the launch just before it, which the kernels leg alone does not show.

The legs alternate in one process and are timed with device events around windows of --steps calls after --warmup; a figure is the median of
its --windows windows, printed with their range.  --root names another checkout of this project (the parent commit, built) to measure
instead of this one: only its `off` arm exists, built WITHOUT the argument, so `--arms off --no-kernels --root <parent>` against `--arms off`
is the step before and after (run the two alternately, a process each: two versions of the package do not share one).
Usage: python scripts/micro/weight_average_bench.py [--windows 7] [--steps 20] [--warmup 5] [--arms off,every1,every4] [--no-kernels] [--root DIR] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--arms", type=str, default="off,every1,every4", help="off | every<count>, comma separated: the order in which the arms are captured and timed ('' = none)")
ap.add_argument("--no-kernels", action="store_true", help="skip the kernels leg")
ap.add_argument("--root", type=str, default=None, help="the checkout to measure (default: the one this script lies in)")
ap.add_argument("--json", type=str, default=None)
a = ap.parse_args()

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.abspath(a.root) if a.root else HERE
sys.path.insert(0, ROOT)
import torch
import __graft_entry__ as ge
ge.load_package()
import bench
from mi_seg_amd.runtime.arena import ParamArena
from mi_seg_amd.runtime.graph import GraphedTrainStep
from mi_seg_amd.training.losses import DiceFocalLoss
from mi_seg_amd.training.optim import ArenaOptimizer

arms = [s for s in a.arms.split(",") if s]
dtype = torch.bfloat16
model = bench.build_model(dtype, "c2")
params = [p for p in model.parameters() if p.requires_grad]
pool, mods = bench.synthetic_pool(16, 1000, "cuda")
labels = (pool * 6).floor().clamp_(0, 5).to(torch.int32)
arena = ParamArena(params, dtype)
crit = DiceFocalLoss(include_background=False, to_onehot_y=True, softmax=True, squared_pred=True, smooth_nr=0.0, smooth_dr=1e-6)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def timed(fn, n):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n


out = {"root": ROOT, "arena_bytes": arena.flat.numel() * 4, "parameters": len(params), "steps_per_window": a.steps, "windows": a.windows,
       "lib": os.environ.get("MISEG_HIP_LIB") or "in-tree"}

# ---------------------------------------------------------------------------------------------------------------- the steps
steps, averagers = {}, {}
for arm in arms:
    opt = ArenaOptimizer(arena, "adamw", lr=1e-4, weight_decay=1e-5)
    kw = {}
    if arm != "off":
        from mi_seg_amd.training.optim import WeightAverager
        averagers[arm] = WeightAverager(opt, "ema", decay=0.999, every=int(arm[len("every"):]))
        kw = dict(weight_averager=averagers[arm])
    steps[arm] = GraphedTrainStep(model, crit, opt, (1, 1, 96, 96, 96), (1, 1, 96, 96, 96), arena, **kw)
    for m_ in sorted(set(mods)):          # capture every graph of the arm outside the timed region
        i = mods.index(m_)
        steps[arm](pool[i:i + 1], labels[i:i + 1], [m_])
torch.cuda.synchronize()


def window(gts, first, n):
    loss = None
    for i in range(a.warmup):
        j = (first + i) % len(mods)
        gts(pool[j:j + 1], labels[j:j + 1], [mods[j]])
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(n):
        j = (first + a.warmup + i) % len(mods)
        loss = gts(pool[j:j + 1], labels[j:j + 1], [mods[j]])
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n, float(loss)


ms = {arm: [] for arm in arms}
for w in range(a.windows):
    for arm in arms:                        # the arms alternate: drift of the device hits all of them alike
        t, loss = window(steps[arm], w * 3, a.steps)
        if loss != loss:
            raise SystemExit(f"{arm}: the loss is NaN")
        ms[arm].append(t)
out["ms_per_patch"] = {arm: spread(v) for arm, v in ms.items()}
out["patches_per_s"] = {arm: spread([1000.0 / t for t in v]) for arm, v in ms.items()}
out["averaged"] = {arm: av.stats() for arm, av in averagers.items()}

# ---------------------------------------------------------------------------------------------------------------- the kernels alone
if not a.no_kernels:
    from mi_seg_amd.hip import lib as L
    from mi_seg_amd.hip import ops
    from mi_seg_amd.training.optim import GradAccumulator, WeightAverager
    opt = ArenaOptimizer(arena, "adamw", lr=1e-4, weight_decay=1e-5)
    n, flat = len(arena.params), arena.flat
    av = WeightAverager(opt, "ema", decay=0.999)
    av.prepare()
    av.update()                              # the first update copies: every timed call below has n > 0, reads both sides and writes avg
    acc = GradAccumulator(opt, 4)
    acc.prepare()
    acc.acc.normal_()
    flat.normal_()
    codes = torch.full((n,), L.FOLD_USED | L.FOLD_EARLIER, dtype=torch.int32, device=flat.device)
    fold = L.GradFold(C.sizeof(L.GradFold), opt._table.data_ptr(), n, opt._blocks, flat.data_ptr(), acc.acc.data_ptr(), codes.data_ptr(), flat.numel(), acc.scale)
    legs = {"weight_average": av.update, "grad_fold_op3": lambda: ops._call("miseg_grad_fold", fold), "weight_swap": lambda: (av.swap(), av.swap())}
    t = {name: [] for name in legs}
    for w in range(a.windows):
        for name, fn in legs.items():       # the legs alternate
            timed(fn, a.warmup)
            t[name].append(timed(fn, a.steps) / (2 if name == "weight_swap" else 1))
    # bytes the arithmetic needs: the average and the fold read two buffers and write one, the swap reads two and writes two
    moved = {"weight_average": 3, "grad_fold_op3": 3, "weight_swap": 4}
    out["kernels_us"] = {name: dict(spread([1000 * x for x in v]), tb_per_s=moved[name] * flat.numel() * 4 / (statistics.median(v) * 1e-3) / 1e12)
                         for name, v in t.items()}
    out["average_over_fold"] = statistics.median(t["weight_average"]) / statistics.median(t["grad_fold_op3"])
    out["swap_over_fold"] = statistics.median(t["weight_swap"]) / statistics.median(t["grad_fold_op3"])
    assert av.stats()["apply"] == 1 and av.stats()["first"] == 0
    arena.refresh_weights()                  # (an even number of swaps: the weights are back; the copies follow the version the swaps bumped)

print(json.dumps(out), flush=True)
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
arena.detach()
