"""The launch-form table of the fused MLP (csrc/mlp.hip: mlp_fwd_kernel<STAT, ANORM, CC>, mlp_bwd_kernel<BSTAT, CC>), its grid arithmetic, its
float64 reference and its exact-integer case.  No GPU needed to import: tests/test_mlp_ref_cpu.py pins the table on the host,
tests/test_hip_mlp_forms.py launches every row.

A row is (id, keywords); the id spells the form.  Keywords: dir "fwd" / "bwd", C, M; forward: stat, an = number of styles of a folded norm
(0: none), style = the selected one, an_out, gamma_null / beta_null (the selected style's row is NULL), res, b1, b2 (default: given);
backward: bstat, dx, b1; walkers = the waves that take a second tile (default 0: none); lay = {operand: layout} for the row views x, res,
y, an_out, dy, dz, h, dx, bs_x - a name of tests/layouts.py ("contig", "slice", "off8") or (element offset, row stride) for the rows that
give every operand a stride of its own; tails / ints = 1."""
import math
import os
import re

import torch

WAVES = 8      # MLP_FWD_WAVES, MLP_BWD_WAVES
CAP = {48: 512, 96: 256}      # workgroups: two 63 KB workgroups per CU at C = 48, one 155 KB workgroup per CU at C = 96
WALK_M = {48: 65589, 96: 32805}      # rows of the `-walk` rows: above 16 * 8 * CAP[C], a last tile of 5
WALKERS = {48: 4, 96: 3}             # ... and the waves that take a second tile there (worked out by hand: 4100 - 4096, 2051 - 2048 tiles)
EPS = 1e-5
TOL = 5e-3      # the bar of test_fused_mlp_forward_and_backward and of the folded-norm tests (tests/test_hip_kernels.py)
VIEWS = {"fwd": ("x", "res", "y", "an_out"), "bwd": ("x", "dy", "dz", "h", "dx", "bs_x")}


def cdiv(a, b):
    return -(-a // b)


# ---- the launchers' grid expressions (miseg_mlp_fwd / miseg_mlp_bwd)
def mtiles(M):
    return cdiv(M, 16)


def blocks(M, C):
    return min(cdiv(mtiles(M), WAVES), CAP[C])


def walkers(M, C):
    """waves that take a second tile: tile = blockIdx.x * 8 + wave, then += 8 * gridDim.x"""
    return max(0, mtiles(M) - WAVES * blocks(M, C))


def last_tile_rows(M):
    return M - 16 * (mtiles(M) - 1)


def form(kw):
    """the instantiation a row launches: ("fwd", STAT, ANORM, CC) / ("bwd", BSTAT, CC)"""
    if kw["dir"] == "fwd":
        return ("fwd", bool(kw.get("stat")), bool(kw.get("an")), kw["C"])
    return ("bwd", bool(kw.get("bstat")), kw["C"])


def launcher_forms():
    """the instantiations the two launchers of mlp.hip name: the template arguments at the MLP_FWD_LAUNCH / MLP_BWD_LAUNCH sites"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mi-seg_amd", "csrc", "mlp.hip")).read()
    tf = {"true": True, "false": False}
    ccs = [int(c) for c in re.findall(r"MLP_FWD_LAUNCH_C\(ST, AN, (\d+)\)", src)]
    fwd = {("fwd", tf[s], tf[a], c) for s, a in re.findall(r"MLP_FWD_LAUNCH\((true|false), (true|false)\)", src) for c in ccs}
    bwd = {("bwd", tf[b], int(c)) for b, c in re.findall(r"MLP_BWD_LAUNCH\((true|false), (\d+)\)", src)}
    return fwd | bwd


def view_cols(kw):
    """name -> columns of every row view the row's launch passes"""
    C = kw["C"]
    if kw["dir"] == "fwd":
        d = {"x": C, "y": C}
        if kw.get("res", 1):
            d["res"] = C
        if kw.get("an") and kw.get("an_out", 1):
            d["an_out"] = C
        return d
    d = {"x": C, "dy": C, "dz": 4 * C, "h": 4 * C}
    if kw.get("dx", 1):
        d["dx"] = C
    if kw.get("bstat"):
        d["bs_x"] = C
    return d


def layout(c, lay):
    """(element offset of the view's first column, row stride) of a bf16 row view of c columns: what tests/layouts.py::Slot builds for a name"""
    if isinstance(lay, tuple):
        return lay
    cp = cdiv(c, 8) * 8
    return {"contig": (0, c), "slice": (8, cp + 24), "off8": (4, cp + 16), "ldodd": (0, cp + 9), "off4": (2, cp + 16), "off2": (1, cp + 16)}[lay]


def params(L, kw, at):
    """the miseg_mlp_params of a row.  at: name -> (address, row stride) of the row views, name -> address of w1, w2, w2t, w1t, b1, b2, stat,
    an_stat, bs_stat, bs_dstat (ops.NormRef.fill writes styles, gamma and beta behind this)"""
    import ctypes
    C = kw["C"]
    p = L.Mlp()
    p.struct_size, p.M, p.C, p.HID, p.dtype = ctypes.sizeof(L.Mlp), kw["M"], C, kw.get("HID", 4 * C), kw.get("dtype", 1)
    p.x, p.ldx = at["x"]
    p.w1 = at["w1"]
    if kw.get("b1", 1):
        p.b1 = at["b1"]
    if kw["dir"] == "fwd":
        p.w2 = at["w2"]
        if kw.get("b2", 1):
            p.b2 = at["b2"]
        if kw.get("res", 1):
            p.res, p.ldres = at["res"]
        p.y, p.ldy = at["y"]
        if kw.get("stat"):
            p.stat = at["stat"]
        if kw.get("an"):
            p.an.stat, p.an.num_styles, p.an.eps = at["an_stat"], kw["an"], EPS
            if kw.get("an_out", 1):
                p.an_out, p.ld_an_out = at["an_out"]
        return p
    p.dy, p.lddy = at["dy"]
    p.w2t, p.w1t = at["w2t"], at["w1t"]
    (p.dz, p.lddz), (p.h, p.ldh) = at["dz"], at["h"]
    if kw.get("dx", 1):
        p.dx, p.lddx = at["dx"]
    if kw.get("bstat"):
        (p.bs_x, p.ld_bs_x), p.bs_stat, p.bs_eps, p.bs_dstat = at["bs_x"], at["bs_stat"], EPS, at["bs_dstat"]
    return p


# ---- the float64 reference
def gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z * 0.7071067811865476))


def gelu_grad(z):
    return 0.5 * (1.0 + torch.erf(z * 0.7071067811865476)) + z * torch.exp(-0.5 * z * z) * 0.3989422804014327


def norm_ref(x, gamma=None, beta=None, eps=EPS):
    """the folded norm over all rows as one sample: fma(x, sc, sh) in float64 (the caller rounds), sc = rstd gamma, sh = beta - mean sc"""
    xd = x.double()
    mean, var = xd.mean(0, keepdim=True), xd.var(0, unbiased=False, keepdim=True)
    sc = (var + eps).rsqrt() * (gamma.double() if gamma is not None else 1.0)
    sh = (beta.double() if beta is not None else 0.0) - mean * sc
    return xd * sc + sh


def reference(x, w1, b1, w2, b2=None, res=None, dy=None):
    """float64 on the very operands the kernel got: z = x W1^T + b1, h = gelu(z), y = bf16(h) W2^T + b2 + res, dz = (dy W2) gelu'(z)
    (dx is formed by the caller from the STORED dz: dz W1).  Returns a dict; y / dz before their rounding to bf16."""
    z = x.double() @ w1.double().t()
    if b1 is not None:
        z = z + b1.double()
    h = gelu(z)
    r = {"z": z, "h": h}
    if w2 is not None:
        y = h.to(torch.bfloat16).double() @ w2.double().t()
        if b2 is not None:
            y = y + b2.double()
        if res is not None:
            y = y + res.double()
        r["y"] = y
        if dy is not None:
            r["dh"] = dy.double() @ w2.double()
            r["dz"] = r["dh"] * gelu_grad(z)
    return r


# ---- the exact-integer case: every value an integer that bf16 holds, gelu the identity, every fp32 sum below 2^24
def int_case(M, C, seed=5):
    """x in {0, 1}, w1, w2 in {-1, 0, 1}, dy in {-2 .. 2}, res in {-3 .. 3}, drawn asymmetrically; b1[j] = 128 + j % 32, b2[c] = c - 20"""
    g = torch.Generator().manual_seed(seed + C)
    H = 4 * C

    def draw(shape, values, probs):
        idx = torch.multinomial(torch.tensor(probs), math.prod(shape), replacement=True, generator=g)
        return torch.tensor(values, dtype=torch.float32)[idx].reshape(shape)

    return dict(x=draw((M, C), [0, 1], [0.6, 0.4]).to(torch.bfloat16), w1=draw((H, C), [-1, 0, 1], [0.5, 0.3, 0.2]).to(torch.bfloat16),
                w2=draw((C, H), [-1, 0, 1], [0.2, 0.3, 0.5]).to(torch.bfloat16), dy=draw((M, C), [-2, -1, 0, 1, 2], [0.3, 0.25, 0.2, 0.15, 0.1]).to(torch.bfloat16),
                res=draw((M, C), [-3, -2, -1, 0, 1, 2, 3], [0.05, 0.1, 0.15, 0.2, 0.2, 0.2, 0.1]).to(torch.bfloat16),
                b1=128.0 + (torch.arange(H) % 32).float(), b2=torch.arange(C).float() - 20.0)


def assert_int_ranges(r, w1):
    """the conditions under which the kernel must match `r` = reference(...) of an int_case bit for bit; returns the float64 dx (or None)"""
    z = r["z"]
    assert bool((z == z.round()).all()) and 32 <= float(z.min()) and float(z.max()) <= 255      # exp(-z^2 / 2) <= exp(-512) = 0 in fp32
    assert torch.equal(r["h"], z) and torch.equal(gelu_grad(z), torch.ones_like(z))      # ... and in float64: gelu(z) = z, gelu'(z) = 1
    assert float(r["y"].abs().max()) < 2 ** 24
    if "dz" not in r:
        return None
    assert torch.equal(r["dz"], r["dh"]) and float(r["dz"].abs().max()) < 256      # (every h and dz: an integer bf16 holds)
    dx = r["dz"] @ w1.double()
    assert float(dx.abs().max()) < 2 ** 24
    return dx


# ---- the rows
ROWS = []


def _row(id_, dir_, C, M, **kw):
    ROWS.append((id_, dict(dir=dir_, C=C, M=M, **kw)))


FWD_FORMS = {"plain": {}, "stat": dict(stat=1), "anorm": dict(an=1), "anorm-stat": dict(an=1, stat=1)}
for _C in (48, 96):
    _W = WALK_M[_C]
    for _n, _k in FWD_FORMS.items():      # the four forms, all tiles full and a last tile of 5 rows
        _row(f"fwd-c{_C}-{_n}-m4096", "fwd", _C, 4096, **_k)
        _row(f"fwd-c{_C}-{_n}-m4101", "fwd", _C, 4101, **_k)
    _row(f"fwd-c{_C}-stat-walk-m{_W}", "fwd", _C, _W, stat=1, walkers=WALKERS[_C])
    _row(f"fwd-c{_C}-anorm-stat-walk-m{_W}", "fwd", _C, _W, an=1, stat=1, walkers=WALKERS[_C])      # the prefetched tile is normalised in the loop
    # options, each at 4101 rows
    _row(f"fwd-c{_C}-stat-nores-m4101", "fwd", _C, 4101, stat=1, res=0)
    _row(f"fwd-c{_C}-plain-nob1-m4101", "fwd", _C, 4101, b1=0)
    _row(f"fwd-c{_C}-plain-nob2-m4101", "fwd", _C, 4101, b2=0)
    _row(f"fwd-c{_C}-stat-nob1-nob2-m4101", "fwd", _C, 4101, stat=1, b1=0, b2=0)
    _row(f"fwd-c{_C}-anorm-noanout-m4101", "fwd", _C, 4101, an=1, an_out=0)
    for _s in range(4):
        _row(f"fwd-c{_C}-anorm-styles4-sel{_s}-m4101", "fwd", _C, 4101, an=4, style=_s, stat=_s & 1)
    _row(f"fwd-c{_C}-anorm-styles4-sel2-nogamma-m4101", "fwd", _C, 4101, an=4, style=2, gamma_null=1)
    _row(f"fwd-c{_C}-anorm-styles4-sel1-nobeta-m4101", "fwd", _C, 4101, an=4, style=1, beta_null=1)
    for _n, _k in (("plain", {}), ("bstat", dict(bstat=1))):
        for _M in (4096, 4101):
            _row(f"bwd-c{_C}-{_n}-m{_M}", "bwd", _C, _M, **_k)
        _row(f"bwd-c{_C}-{_n}-walk-m{_W}", "bwd", _C, _W, walkers=WALKERS[_C], **_k)
    _row(f"bwd-c{_C}-plain-nodx-m4101", "bwd", _C, 4101, dx=0)
    _row(f"bwd-c{_C}-bstat-nob1-m4101", "bwd", _C, 4101, bstat=1, b1=0)
    # layouts: every row view as an aligned slice and 8 bytes into a 16-byte unit, the others contiguous
    for _l in ("slice", "off8"):
        for _o in ("x", "res", "y", "an_out"):
            _row(f"fwd-c{_C}-anorm-stat-{_o}-{_l}-m4101", "fwd", _C, 4101, an=1, stat=1, lay={_o: _l})
        for _o in ("x", "dy", "dz", "h", "dx", "bs_x"):
            _row(f"bwd-c{_C}-bstat-{_o}-{_l}-m4101", "bwd", _C, 4101, bstat=1, lay={_o: _l})
    # every operand in a layout and with a row stride of its own: a stride applied to the wrong operand reads NaN or writes a sentinel
    _row(f"fwd-c{_C}-anorm-stat-mixed-m4101", "fwd", _C, 4101, an=1, stat=1,
         lay={"x": (4, _C + 8), "res": (8, _C + 16), "y": (4, _C + 24), "an_out": (8, _C + 32)})
    _row(f"bwd-c{_C}-bstat-mixed-m4101", "bwd", _C, 4101, bstat=1,
         lay={"x": (4, _C + 8), "dy": (8, _C + 16), "dz": (4, 4 * _C + 8), "h": (8, 4 * _C + 16), "dx": (4, _C + 24), "bs_x": (8, _C + 32)})
    # GELU tails (z spans about +-12: exp(-z^2 / 2) underflows, the cdf saturates) and exact integers
    _row(f"fwd-c{_C}-stat-tails-m4101", "fwd", _C, 4101, stat=1, tails=1)
    _row(f"bwd-c{_C}-plain-tails-m4101", "bwd", _C, 4101, tails=1)
    _row(f"fwd-c{_C}-plain-ints-m4101", "fwd", _C, 4101, ints=1)
    _row(f"bwd-c{_C}-plain-ints-m4101", "bwd", _C, 4101, ints=1)


# ---- refusals (tests/test_hip_mlp_forms.py): (id, entry point, what to change in a valid 4096-row, 48-channel launch, the error's text)
FUSED_EDGES = [(4095, 48, 192, 1, 0), (4096, 48, 192, 1, 1), (4096, 96, 384, 1, 1), (4096, 32, 128, 1, 0), (4096, 64, 256, 1, 0), (4096, 192, 768, 1, 0),
               (4096, 48, 176, 1, 0), (4096, 48, 208, 1, 0), (4096, 96, 368, 1, 0), (4096, 96, 400, 1, 0), (4096, 48, 192, 0, 0), (4096, 96, 384, 0, 0)]
REFUSALS = []
for _d, _ops in (("fwd", ("x", "y", "res", "an_out")), ("bwd", ("x", "dy", "dz", "h", "dx", "bs_x"))):
    for _o in _ops:
        for _l in ("ldodd", "off4", "off2"):
            REFUSALS.append((f"{_d}-{_o}-{_l}", _d, ("lay", _o, _l)))
        REFUSALS.append((f"{_d}-ld{_o}-below-width", _d, ("short", _o)))      # ldres, lddy, lddz, ldh, lddx, ld_bs_x: new with this table
    for _w in (("w1", "w2") if _d == "fwd" else ("w1", "w2t", "w1t")):
        REFUSALS.append((f"{_d}-{_w}-off8", _d, ("woff", _w)))
    REFUSALS.append((f"{_d}-struct-size", _d, ("struct",)))
REFUSALS += [("fwd-num-styles-0", "fwd", ("styles", 0)), ("fwd-num-styles-5", "fwd", ("styles", 5)), ("bwd-bstat-without-dx", "bwd", ("nodx",))]
for _e in FUSED_EDGES:
    if not _e[4]:
        REFUSALS += [(f"{_d}-unsupported-m{_e[0]}-c{_e[1]}-hid{_e[2]}-{'bf16' if _e[3] else 'f32'}", _d, ("shape",) + _e[:4]) for _d in ("fwd", "bwd")]
