"""which GEMM problems of one C-Swin-UNETR step land in which kernel: miseg_gemm_plan is asked for every miseg_gemm call of the step"""
import os, sys, collections
import ctypes as C
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import __graft_entry__ as ge
ge.load_package()
import bench
from mi_seg_amd.hip import ops, lib as L
KERNELS = {getattr(L, n): n[5:].lower() for n in dir(L) if n.startswith("GEMM_NT_") or n.startswith("GEMM_TN_")}
model = bench.build_model(torch.bfloat16)
x = torch.randn(1, 1, 96, 96, 96, device="cuda"); cot = torch.randn(1, 6, 96, 96, 96, device="cuda")
seen = collections.Counter()
orig = ops._call
def spy(name, p, prof=None, extra=()):
    if name == "miseg_gemm":
        pl = L.GemmPlan()
        L.check(L.load().miseg_gemm_plan(C.byref(p), C.byref(pl)), "gemm_plan")
        form = {L.GEMM_NT_SMALL: f"<{pl.mtw},{pl.ntw},gelu {pl.gelu},stat {pl.stat},anorm {pl.anorm}>",
                L.GEMM_NT_STREAM: f"<{pl.k16},gelu {pl.gelu},{pl.nch},stat {pl.stat},scat {pl.scat},anorm {pl.anorm}>", L.GEMM_NT_GENERIC: f"<{pl.nt}>",
                L.GEMM_TN_STREAM: f"{pl.wm}x{pl.wn} waves"}.get(pl.kernel, "")
        seen[(KERNELS[pl.kernel], p.M, p.N, p.K, form, f"{pl.grid_x}x{pl.grid_y}x{pl.grid_z}", pl.lds_bytes)] += 1
    return orig(name, p, prof=prof, extra=extra)
ops._call = spy
ops.begin_step()
model(x, [0]).backward(cot)
torch.cuda.synchronize()
for (k, M, N, K, form, grid, lds), n in sorted(seen.items(), key=lambda kv: (kv[0][0], -kv[0][1], kv[0][2], kv[0][3])):
    print(f"{k:14s} M {M:7d} N {N:5d} K {K:6d}  grid {grid:12s} lds {lds:6d}  {form}  x{n}")
