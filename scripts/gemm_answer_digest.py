"""what the seven question entry points of miseg_gemm (fuses_stat / _anorm / _bstat / _scatter, tn_fuses_colsum, tn_splits, workspace_bytes)
answer over the seeded sweep of tests/gemm_cases.py, reduced to a digest - for comparing two builds of the library (miseg_gemm_params is
the same in both).  CPU only.  Usage: python scripts/gemm_answer_digest.py [--lib path/to/libmiseg_hip.so] [--count N] [--seed S]"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as ge
ge.load_package()
from mi_seg_amd.hip import lib as L
import gemm_cases as G

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=L.LIB_PATH)
ap.add_argument("--count", type=int, default=200000)
ap.add_argument("--seed", type=int, default=20261020)
args = ap.parse_args()
so = C.CDLL(args.lib)      # opened bare: an older build has neither this tree's source digest nor all of its symbols
for q in G.QUESTIONS:
    getattr(so, q).restype = C.c_size_t if q.endswith("bytes") else C.c_int
    getattr(so, q).argtypes = [C.POINTER(L.Gemm)]
t0 = time.time()
digest, asked, yes = G.sweep(so, L, args.count, args.seed)
print(f"{args.lib}\nseed {args.seed} count {args.count}: {asked} parameter sets in {time.time() - t0:.1f} s, sha256 {digest}\nanswered non-zero: {yes}")
