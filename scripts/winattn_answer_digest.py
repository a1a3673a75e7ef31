"""what the two question entry points of the attention launches (miseg_winattn_on_matrix_cores / miseg_winattn_bwd_on_matrix_cores) answer over
the seeded sweep of tests/winattn_cases.py, reduced to a digest over the parameter sets THIS tree's plan accepts - for comparing two builds of
the library (the params structs are the same in both; an older build needs no plan symbol).  Also counts the refused sets the library under
test still answers 1 for, by the plan's refusal message.  CPU only.
Usage: python scripts/winattn_answer_digest.py [--lib path/to/libmiseg_hip.so] [--count N] [--seed S]"""
import argparse
import collections
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as ge
ge.load_package()
from mi_seg_amd.hip import lib as L
import winattn_cases as G

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=L.LIB_PATH)
ap.add_argument("--count", type=int, default=120000)
ap.add_argument("--seed", type=int, default=20261021)
args = ap.parse_args()
so = C.CDLL(args.lib)      # opened bare: an older build has neither this tree's source digest nor all of its symbols
for q in G.QUESTIONS:
    getattr(so, q).restype, getattr(so, q).argtypes = C.c_int, [C.c_void_p]
t0 = time.time()
digest, n = G.sweep(L.load(), so, L, args.count, args.seed)
print(f"{args.lib}\nseed {args.seed} count {args.count} in {time.time() - t0:.1f} s: accepted (fwd, bwd) {n['accepted']}, answered 1 among them {n['yes']}, sha256 {digest}")
classes = collections.Counter()
for d, msg, _ in n["refused_yes"]:
    classes[("fwd", "bwd")[d], next((c for c in G.REFUSED_CLASSES if c in msg), "UNLISTED: " + msg)] += 1
print(f"refused (fwd, bwd) {n['refused']}; answered 1 although refused: {len(n['refused_yes'])}")
for k, v in sorted(classes.items()):
    print(f"  {k[0]} {v:6d}  {k[1]}")
