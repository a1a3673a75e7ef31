"""What gradient accumulation over micro-batches costs and buys, on the headline C-Swin-UNETR of bench.py's
secondary.c2_train_step_bf16 (bf16, N = 1, one 96^3 patch per micro-batch):

    fold   miseg_grad_fold over the model's whole gradient arena against the torch composition of the same arithmetic:
             add    acc = acc + g (op 3 everywhere)                    against  acc.add_(flat)
             close  arena = (acc + g) * fl(1/k) (op 7 everywhere)     against  torch.mul(acc + flat, s, out=flat)
    step   GraphedTrainStep patches/s (one patch = one micro-batch = one call) with accumulate_grad_batches = 1, 2, 4: the arms named in
           --arms share one model and one arena (an optimiser and a set of graphs each)

The legs alternate in one process and are timed with device events around windows of --steps calls after --warmup; a figure is the median of
its --windows windows, printed with their range.  --root names another checkout of this project (the parent commit, built) to measure
instead of this one: its k1 arm is built WITHOUT the argument, so `--arms k1 --root <parent>` against `--arms k1` is the step before and
after (run the two alternately, a process each: two versions of the package do not share one).
Usage: python scripts/micro/grad_accum_bench.py [--windows 7] [--steps 20] [--warmup 5] [--arms k1,k2,k4] [--no-fold] [--root DIR] [--json out.json]"""
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
ap.add_argument("--arms", type=str, default="k1,k2,k4", help="k<count>, comma separated: the order in which the arms are captured and timed ('' = none)")
ap.add_argument("--no-fold", action="store_true", help="skip the fold-against-torch leg")
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

counts = [int(s[1:]) for s in a.arms.split(",") if s]
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


out = {"root": ROOT, "arena_bytes": arena.flat.numel() * 4, "parameters": len(params), "steps_per_window": a.steps, "windows": a.windows}

# ---------------------------------------------------------------------------------------------------------------- the steps
steps = {}
for k in counts:
    opt = ArenaOptimizer(arena, "adamw", lr=1e-4, weight_decay=1e-5)
    kw = {} if k == 1 else dict(accumulate_grad_batches=k)
    steps[k] = GraphedTrainStep(model, crit, opt, (1, 1, 96, 96, 96), (1, 1, 96, 96, 96), arena, **kw)
    for m_ in sorted(set(mods)):          # capture every graph of the arm outside the timed region: whole windows of each modality alone
        i = mods.index(m_)
        for _ in range(k):
            steps[k](pool[i:i + 1], labels[i:i + 1], [m_])
torch.cuda.synchronize()


def window(gts, first, n):
    """n calls after a warm-up.  With --steps a multiple of every arm's count, any n calls in a row hold n / k closing ones, wherever the
    arm's accumulation window happens to stand when the timing starts."""
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


ms = {k: [] for k in counts}
for w in range(a.windows):
    for k in counts:                        # the arms alternate: drift of the device hits all of them alike
        t, loss = window(steps[k], w * 3, a.steps)
        if loss != loss:
            raise SystemExit(f"k{k}: the loss is NaN")
        ms[k].append(t)
out["lib"] = os.environ.get("MISEG_HIP_LIB") or "in-tree"
out["ms_per_patch"] = {f"k{k}": spread(v) for k, v in ms.items()}
out["patches_per_s"] = {f"k{k}": spread([1000.0 / t for t in v]) for k, v in ms.items()}
out["graphs"] = {f"k{k}": len(steps[k].graphs) for k in counts}

# ---------------------------------------------------------------------------------------------------------------- the fold alone
if not a.no_fold:
    from mi_seg_amd.hip import lib as L
    from mi_seg_amd.hip import ops
    from mi_seg_amd.training.optim import GradAccumulator
    opt = ArenaOptimizer(arena, "adamw", lr=1e-4, weight_decay=1e-5)
    acc = GradAccumulator(opt, 4)
    acc.prepare()
    n = len(arena.params)
    flat = arena.flat
    s = torch.tensor(acc.scale, dtype=torch.float32, device=flat.device)

    def fold_with(code):
        codes = torch.full((n,), code, dtype=torch.int32, device=flat.device)          # (a tensor per leg: the launch reads it when it runs)
        p = L.GradFold(C.sizeof(L.GradFold), opt._table.data_ptr(), n, opt._blocks, flat.data_ptr(), acc.acc.data_ptr(), codes.data_ptr(), flat.numel(), acc.scale)
        return lambda: (codes, ops._call("miseg_grad_fold", p))

    legs = {"add": (fold_with(L.FOLD_USED | L.FOLD_EARLIER), lambda: acc.acc.add_(flat)),
            "close": (fold_with(L.FOLD_USED | L.FOLD_EARLIER | L.FOLD_CLOSE), lambda: torch.mul(acc.acc + flat, s, out=flat))}
    res = {}
    for name, (hip, ref) in legs.items():
        t = {"hip": [], "torch": []}
        for w in range(a.windows):
            for leg, fn in (("hip", hip), ("torch", ref)):
                flat.normal_()
                acc.acc.normal_()          # (a closing fold scales the arena in place: fresh values keep every window alike)
                timed(fn, a.warmup)
                t[leg].append(timed(fn, a.steps))
        # bytes the arithmetic needs: add reads two buffers and writes one, close the same
        res[name] = {leg: dict(spread([1000 * x for x in v]), tb_per_s=3 * flat.numel() * 4 / (statistics.median(v) * 1e-3) / 1e12) for leg, v in t.items()}
    out["fold_us"] = res
    # the two agree bit for bit on every parameter's slot (the composition rounds the sum and the product on their own, like the kernel; it
    # also writes the padding between slots, which the kernel leaves alone)
    flat.normal_()
    acc.acc.normal_()
    want = (acc.acc + flat) * s
    legs["close"][0]()
    out["fold_equals_torch_bits"] = all(bool(torch.equal(v.view(torch.int32), want[o:o + v.numel()].view(v.shape).view(torch.int32)))
                                        for v, o in zip(arena.views, arena._offs))

print(json.dumps(out), flush=True)
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
arena.detach()
