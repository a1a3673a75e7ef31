"""launches every launchable row of tests/instnorm_cases.py once through its entry point, on real operands laid out as the row says
(tests/layouts.py), and writes per row every output of the call: a sha256 of the outputs the kernels STORE (y, dx, dres, dxa, dxb, the x of
the slab forward, the statistics of the one-launch forward), and the values of the outputs that meet in atomics (streaming statistics,
dgamma / dbeta, r1dw) - for comparing two builds of the library: the first bit for bit, the second against the spread between two runs of
one build (scripts/instnorm_table.py A.pt; ... B.pt; --compare A.pt B.pt).  Forward statistics and the sums miseg_instnorm_bwd_apply expects
are computed with torch into replica 0, so that no input of a row depends on the order of atomics.  Uses the entry points only, no plan.
Usage: python scripts/instnorm_table.py OUT.pt [--skip-long] | --compare A.pt B.pt"""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch


def compare(pa, pb):
    a, b = torch.load(pa, weights_only=False), torch.load(pb, weights_only=False)
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    differ, worst = [], 0.0
    for rid in sorted(a):
        for name, (kind, va) in a[rid].items():
            vb = b[rid][name][1]
            if kind == "stored":
                if va != vb:
                    differ.append(f"{rid}:{name}")
            else:
                d = float(((va - vb).abs() / (1e-30 + torch.maximum(va.abs(), vb.abs()).max())).max())
                worst = max(worst, d)
    print(f"{len(a)} rows; stored outputs that differ: {len(differ)} {differ[:8]}; atomic outputs: worst difference {worst:.3e} of the output's largest magnitude")


if len(sys.argv) < 2 or (sys.argv[1] == "--compare" and len(sys.argv) != 4):
    sys.exit("usage: python scripts/instnorm_table.py OUT.pt [--skip-long] | --compare A.pt B.pt")
if sys.argv[1] == "--compare":
    compare(sys.argv[2], sys.argv[3])
    sys.exit(0)

import __graft_entry__ as ge
ge.load_package()
from mi_seg_amd.hip import lib as L
import instnorm_cases as IC
from layouts import place_in, place_out

so = L.load()
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
DEV = "cuda"
EPS = 1e-5
keep = []


def ref(t):
    keep.append(t)      # alive until the launch has finished
    return t.data_ptr(), (t.stride(-2) if t.dim() > 1 else 0)


def replica0(sums, B, Cc):
    st = torch.zeros(so.miseg_instnorm_stat_bytes(B, Cc) // 8, dtype=torch.float64, device=DEV).view(-1, B, Cc, 2)
    st[0] = sums
    return st


def moments(x):
    xd = x.double()
    return torch.stack([xd.sum(1), xd.square().sum(1)], -1)


def launch(r):
    e, dt, B, S, Cc, o = r["entry"], DT[r["dtype"]], r["B"], r["S"], r["C"], r["opts"]
    g = torch.Generator().manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)      # noqa: E731
    lay = lambda k: r["lay"].get(k, "contig")      # noqa: E731
    inp = lambda k: place_in(rnd(B, S, Cc).to(dt), lay(k))      # noqa: E731
    outp = lambda k: place_out((B, S, Cc), dt, lay(k))      # noqa: E731
    ops, stored, atomic = {}, {}, {}
    del keep[:]
    r1 = bool(o.get("rank1"))
    zstat = lambda: replica0(0.0, B, Cc)      # noqa: E731
    if r1:
        r1x, r1w = rnd(B * S, 1).to(dt), rnd(Cc).to(dt)
        prod = (r1x.float() * r1w.float()[None, :]).to(dt).view(B, S, Cc)      # what the kernels form: round(r1x * r1w)
        ops["r1x"], ops["r1w"] = (r1x.data_ptr(), 1), ref(r1w)
    if e == "stats":
        x, st = inp("x"), zstat()
        ops.update(x=ref(x), stat=ref(st))
        atomic["stat"] = st
    elif e in ("apply", "fwd", "fwd_slabs"):
        x = outp("x") if e == "fwd_slabs" else inp("x")
        xv = x.view if e == "fwd_slabs" else x
        y = outp("y")
        st = zstat() if e != "apply" else replica0(moments(xv), B, Cc)
        ops.update(x=ref(xv), y=ref(y.view), stat=ref(st))
        if o.get("res"):
            ops["res"] = ref(inp("res"))
        if r1:
            rs = replica0(moments(prod), B, Cc)
            ops["res_stat"] = ref(rs)
        stored["y"] = y.buf
        if e == "fwd_slabs":
            stored["x"] = x.buf
        if e != "apply":
            (stored if S <= so.miseg_instnorm_fused_max_rows() else atomic)["stat"] = st
    elif e in ("bwd", "bwd_apply", "bwd_slabs", "bwd_reduce"):
        x = inp("x")
        st, dst = replica0(moments(x), B, Cc), zstat()
        ops.update(x=ref(x), stat=ref(st), dstat=ref(dst))
        if e != "bwd_slabs":
            dy = inp("dy")
            ops["dy"] = ref(dy)
        if e == "bwd_apply":
            xd = x.double()
            xh = (xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + EPS)
            dst[0] = torch.stack([dy.double().sum(1), (dy.double() * xh).sum(1)], -1)
        if e == "bwd_reduce":
            atomic["dstat"] = dst
        else:
            dx = outp("dx")
            ops["dx"] = ref(dx.view)
            stored["dx"] = dx.buf
            for k in ("y", "gadd"):
                if o.get(k):
                    ops[k] = ref(inp(k))
            if o.get("dres"):
                dres = outp("dres")
                ops["dres"] = ref(dres.view)
                stored["dres"] = dres.buf
    else:
        dy, xa = inp("dy"), inp("xa")
        dxa = outp("dxa")
        sa = replica0(moments(xa), B, Cc)
        ops.update(dy=ref(dy), xa=ref(xa), dxa=ref(dxa.view), stat_a=ref(sa), dstat_a=ref(zstat()), dstat_b=ref(zstat()))
        stored["dxa"] = dxa.buf
        if r1:
            ops["stat_b"] = ref(replica0(moments(prod), B, Cc))
            dw = torch.zeros(Cc, device=DEV)
            ops["r1dw"] = ref(dw)
            atomic["r1dw"] = dw
        else:
            xb, dxb = inp("xb"), outp("dxb")
            ops.update(xb=ref(xb), dxb=ref(dxb.view), stat_b=ref(replica0(moments(xb), B, Cc)))
            stored["dxb"] = dxb.buf
            if o.get("y"):
                ops["y"] = ref(inp("y"))
    p, extra = IC.params(r, L, ops)
    # one style with affine rows and gradients, so that dgamma / dbeta are written
    aff = {"apply": ("gamma", "beta"), "fwd": ("gamma", "beta"), "fwd_slabs": ("gamma", "beta"), "bwd": ("gamma", "beta", "dgamma", "dbeta"),
           "bwd_apply": ("gamma", "dgamma", "dbeta"), "bwd_slabs": ("gamma", "beta", "dgamma", "dbeta"),
           "pair": ("gamma_a", "beta_a", "gamma_b", "beta_b", "dgamma_a", "dbeta_a", "dgamma_b", "dbeta_b")}.get(e, ())
    for f in aff:
        t = torch.zeros(Cc, device=DEV) if f.startswith("d") else rnd(Cc) * 0.2 + 1
        getattr(p, f)[0] = t.data_ptr()
        keep.append(t)
        if f.startswith("d"):
            atomic[f] = t
    if e.endswith("_slabs"):
        n, stride = o["nslabs"], B * S * Cc + o["gap"]
        ws = torch.full((n * stride + 4,), float("nan"), device=DEV)
        off = o.get("slabs_off", 0) // 4
        for k in range(n):
            ws[off + k * stride:off + k * stride + B * S * Cc] = rnd(B * S * Cc) * 0.8
        extra = (C.c_void_p(ws.data_ptr() + 4 * off),) + tuple(extra[1:])
    torch.cuda.synchronize()
    L.check(getattr(so, IC.ENTRY_FN[e])(C.byref(p), *extra, None), r["id"])
    torch.cuda.synchronize()
    out = {k: ("stored", hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()) for k, t in stored.items()}
    out.update({k: ("atomic", t.double().cpu().clone()) for k, t in atomic.items()})
    return out


result = {}
for r in IC.ROWS:
    if not r["launch"] or ("--skip-long" in sys.argv and r["S"] > (1 << 20)):
        continue
    result[r["id"]] = launch(r)
torch.save(result, sys.argv[1])
print(len(result), "rows launched ->", sys.argv[1])
