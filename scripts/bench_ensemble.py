"""the ensemble fold (csrc/ensemble.hip, miseg_ensemble_accumulate) at the prediction export's own workload: the stitched
logits of a 512 x 512 x 363 volume with 8 classes, fp32 [1, 8, 363, 512, 512] = 3.05 GB.  For each of the three kinds, with device events after
warm-up (median of 5 runs): one accumulate call that adds a member predicted on the fully mirrored volume (flip along D, H and W; reads src,
reads and writes acc: 3 x the tensor), the same call as the first member (2 x the tensor), and the torch composition it replaces on the same
tensors - torch.flip, the term (nothing | softmax | argmax + one_hot), mul by the weight, add into the accumulator.  Prints ms and GB/s of
the algorithmic bytes (the kernel's 2 or 3 tensors; the torch passes move more than that, which is the point), and checks the two results
against each other (kinds mean_logits and vote to the bit).  --shape D H W / --classes C run another size."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import __graft_entry__ as ge

ge.load_package()
from mi_seg_amd.hip import ops

RUNS = 5
FLIP = (True, True, True)
WEIGHT = 0.75


def timed(fn):
    for _ in range(2):
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


def torch_fold(src, acc, kind, first):
    """the glue this kernel replaces: every line is a pass over the tensor"""
    x = torch.flip(src, (2, 3, 4))
    if kind == "mean_prob":
        x = torch.softmax(x, dim=1)
    elif kind == "vote":
        x = torch.nn.functional.one_hot(x.argmax(1), src.shape[1]).permute(0, 4, 1, 2, 3).float()
    if kind != "vote":
        x = x * WEIGHT
    if first:
        acc.copy_(x)
    else:
        acc.add_(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(363, 512, 512), help="D H W")
    ap.add_argument("--classes", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble: needs the HIP device (a CPU run times nothing)")
    shape = (1, args.classes) + tuple(args.shape)
    g = torch.Generator(device="cuda").manual_seed(0)
    src = torch.randn(shape, device="cuda", generator=g) * 3
    acc = torch.randn(shape, device="cuda", generator=g)
    keep = acc.clone()
    nbytes = src.numel() * 4
    print(f"logits {tuple(shape)} fp32, {nbytes / 1e9:.2f} GB a tensor ({nbytes} bytes: {'above' if nbytes > 2 ** 31 else 'below'} 2^31), flip {FLIP}, weight {WEIGHT}")
    for kind in ("mean_logits", "mean_prob", "vote"):
        for first in (False, True):
            moved = (2 if first else 3) * nbytes
            ms, lo, hi = timed(lambda: ops.ensemble_accumulate(src, acc, flip=FLIP, kind=kind, weight=WEIGHT, first=first))
            ms_t, lo_t, hi_t = timed(lambda: torch_fold(src, acc, kind, first))
            print(f"{kind:11s} {'first' if first else 'add  '}  kernel {ms:8.3f} ms ({lo:.3f}..{hi:.3f}) {moved / ms / 1e6:7.1f} GB/s   "
                  f"torch composition {ms_t:8.3f} ms ({lo_t:.3f}..{hi_t:.3f}) {moved / ms_t / 1e6:7.1f} GB/s   x{ms_t / ms:.2f}", flush=True)
        # one fold from the same accumulator both ways
        acc.copy_(keep)
        ops.ensemble_accumulate(src, acc, flip=FLIP, kind=kind, weight=WEIGHT)
        got = acc.clone()
        acc.copy_(keep)
        torch_fold(src, acc, kind, False)
        diff = float((got - acc).abs().max())
        print(f"{kind:11s} kernel against the torch composition: largest difference {diff:.3e}" + ("" if kind == "mean_prob" else f", identical: {torch.equal(got, acc)}"), flush=True)
        del got
        acc.copy_(keep)


if __name__ == "__main__":
    main()
