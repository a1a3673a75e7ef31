"""launches every row of tests/gemm_cases.py that is not refused once (twice with --reps 2) through miseg_gemm, on real buffers laid out as the
row says (offsets, row strides, optional views), and writes per row a sha256 of everything the launch wrote, plus the output itself where it
is small - for a kernel trace of the table (rocprofv3 --kernel-trace -- python scripts/gemm_table.py) and for comparing two builds of the
library bit for bit.  Uses miseg_gemm and miseg_gemm_workspace_bytes only.  Usage: python scripts/gemm_table.py OUT.pt [--reps N]"""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
import __graft_entry__ as ge
ge.load_package()
from mi_seg_amd.hip import lib as L, ops
import gemm_cases as G

out_path = sys.argv[1]
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 1
so = L.load()
DT = {0: torch.float32, 1: torch.bfloat16}
gen = torch.Generator().manual_seed(7)


def view(rows, cols, ld, dtype, off_bytes, fill=None):
    """a [rows][cols] view with row stride ld, `off_bytes` past a 256-byte aligned base; returns (storage, pointer, the view)"""
    es = torch.empty(0, dtype=dtype).element_size()
    pad = off_bytes // es
    n = pad + (rows - 1) * ld + cols
    t = (torch.randn(n, generator=gen) if fill is None else torch.full((n,), float(fill))).to("cuda").to(dtype)
    return t, t.data_ptr() + off_bytes, t[pad:].as_strided((rows, cols), (ld, 1))


def launch(kw):
    p = G.params(L, **kw)
    M, N, K, tn = p.M, p.N, p.K, p.ta
    dt, odt = DT[p.dtype], DT[p.out_dtype]
    keep, outs = [], []
    a = view(K if tn else M, M if tn else K, p.lda, dt, p.A - G.A)
    b = view(K if tn else N, N if tn else K, p.ldb, dt, p.B - G.A)
    rows_c, cols_c = (8 * M, p.scat_cout) if p.scat_cout else (M, N)
    c = view(rows_c, cols_c, p.ldc if not p.scat_cout else p.scat_cout, odt, p.C - G.A, fill=0.0)
    if p.scat_cout:
        p.ldc = p.scat_cout
    p.A, p.B, p.C = a[1], b[1], c[1]
    keep += [a, b, c]
    outs.append(c[0])
    if p.bias:
        bias = torch.randn(N, generator=gen).cuda()
        keep.append(bias)
        p.bias = bias.data_ptr()
    if p.res:
        r = view(M, N, p.ldres, odt, p.res - G.A)
        keep.append(r)
        p.res = r[1]
    if p.aux:
        x = view(M, N, p.ldaux, odt, p.aux - G.A)
        keep.append(x)
        p.aux = x[1]
        if p.epi_mode == 1:
            outs.append(x[0])
    if p.an.stat:
        st = ops.instnorm_stats(a[2].reshape(1, M, K) if a[2].is_contiguous() else a[2].contiguous().reshape(1, M, K), 1, M)
        keep.append(st)
        p.an.stat, p.an.eps = st.data_ptr(), 1e-5
    if p.an_out:
        x = view(M, K, p.ld_an_out, dt, p.an_out - G.A, fill=0.0)
        keep.append(x)
        p.an_out = x[1]
        outs.append(x[0])
    if p.bs_x:
        x = view(M, N, p.ld_bs_x, odt, p.bs_x - G.A)
        st = ops.instnorm_stats(x[2].contiguous().reshape(1, M, N), 1, M)
        keep += [x, st]
        p.bs_x, p.bs_stat, p.bs_eps = x[1], st.data_ptr(), 1e-5
    if p.stat:
        st = torch.zeros(so.miseg_instnorm_stat_bytes(1, N) // 8, dtype=torch.float64, device="cuda")
        keep.append(st)
        p.stat = st.data_ptr()
        outs.append(st)
    if p.tn_colsum:
        cs = torch.zeros(M, device="cuda")
        keep.append(cs)
        p.tn_colsum = cs.data_ptr()
        outs.append(cs)
    wsb = so.miseg_gemm_workspace_bytes(C.byref(p))
    p.workspace = None
    if wsb:
        ws = torch.empty(wsb // 4, device="cuda")
        keep.append(ws)
        p.workspace = ws.data_ptr()
        if p.defer_reduce:
            outs.append(ws)
    torch.cuda.synchronize()
    L.check(so.miseg_gemm(C.byref(p), None), "miseg_gemm")
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in outs:
        h.update(t.view(torch.uint8).cpu().numpy().tobytes())
    small = c[0].float().cpu() if c[0].numel() <= (1 << 18) else None
    return h.hexdigest(), small


result = {}
for rep in range(reps):
    for id_, kw, expect in G.ROWS:
        if expect.get("rc", 0) != 0:
            continue
        gen.manual_seed(7)      # the same operands in every repeat
        sha, small = launch(kw)
        result.setdefault(id_, []).append((sha, small))
torch.save(result, out_path)
print(len(result), "rows launched", reps, "time(s) ->", out_path)
