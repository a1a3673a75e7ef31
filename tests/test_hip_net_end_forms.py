"""Launch forms and operand layouts of the kernels at the two ends of every network (csrc/net_end.hip): the stem convolution
(miseg_conv3_thin_fwd / _wgrad), the patch embedding (miseg_patch_embed_fwd / _bwd), the output head (miseg_head_fwd / _bwd) and the public
im2col3 / col2im3 (csrc/elementwise.hip).

The rows are tests/net_end_cases.py, the table tests/test_net_end_plan_cpu.py pins on the host-only plans: every row goes through
`ops._call` with its ctypes struct (leading dimensions and bases chosen freely), and BEFORE the launch the plan of these very params must
name the kernel, the partial-sum route, the passes and the wrapping loop the row is there for.  Form -> rows: the row ids carry the form
(`stem_fwd-mfma-*`, `-brick-*`, `-generic-*`; `stem_wgrad-mfma-*` ...; `patch_bwd-team-*`, `-generic-*`; `head_fwd-tile-*`, `-scalar-*`;
`head_bwd-dx<form>-dw<form>-*`, `head_bwd-scalar-*` = scalar dx with the generic dw), `*-wrap-*` are the rows whose loop goes round.

Operands: channels-last ones come from tests/layouts.py (inputs in NaN-filled buffers, outputs in sentinel-filled ones whose every element
outside the view must survive); the NCDHW fp32 image sits in a NaN-filled allocation with more than one depth slab of NaN before and behind it
(a halo read outside the volume poisons the result); the head's NCDHW y / dy sit in sentinel- / NaN-filled allocations; with B = 2 the samples
differ; dw and dbias start from random values inside sentinel guards and `after - before` is judged (the contract is +=); rows with a NULL
dbias / bias / dx / dw / workspace check that nothing else moved.  References are float64 F.conv3d, torch.nn.grad.conv3d_weight /
conv3d_input and plain sums on the very inputs the kernel got; tests/parity.py judges pooled and per element at the tolerances
tests/test_hip_kernels.py uses for these calls (fp32 2e-4, bf16 2e-2, the head's dbias 1e-4).  Where an honest bf16 result exceeds the
per-element bound the `local_tol` rule of DESIGN.md section 3 applies (max(tol, 2 x the local error of torch's own bf16 composition against the
same float64 reference), computed here, only then, and reported in the error table).  Every forward, both data gradients and the weight
gradients on the partial-sum route run twice and must repeat bit for bit; the atomic routes are judged by parity only.

NOT launched: the 64-bit item forms of patch_embed_fwd_kernel and head_bwd_dx_team_kernel (2^29 .. 2^31 items); the plan test pins their choice.

Measured on an MI355X, worst over the rows, pooled / per element (the last test of the file prints this table; no row needed the local_tol rule):
  stem forward y        fp32 1.7e-7 / 7.5e-7    bf16 3.0e-3 / 1.5e-2  (bar 2e-4 / 2e-2; the matrix-core form rounds image and weights to bf16)
  stem dw               fp32 4.3e-7 / 1.3e-6    bf16 1.7e-3 / 7.4e-3
  patch embed y         fp32 1.1e-7 / 2.7e-7    bf16 2.1e-3 / 2.9e-3
  patch embed dw        fp32 5.5e-7 / 2.0e-6    bf16 4.9e-7 / 1.2e-6  (fp32 sums of the bf16 gradients the reference also got)
  patch embed dbias     fp32 5.8e-7 / 7.9e-7    bf16 5.8e-8 / 6.6e-8
  head y                fp32 1.8e-7 / 5.2e-7    bf16 1.8e-7 / 5.7e-7  (fp32 output of bf16 activations)
  head dx               fp32 7.3e-8 / 2.1e-7    bf16 1.8e-3 / 3.2e-3
  head dw               fp32 1.5e-6 / 2.7e-6    bf16 1.9e-3 / 8.6e-3  (the matrix-core form rounds dy to bf16)
  head dbias (bar 1e-4) fp32 6.0e-6 / 3.0e-6    bf16 5.0e-7 / 3.7e-7
  col2im3               fp32 7.3e-8 / 1.7e-7    bf16 1.7e-3 / 2.6e-3;  im2col3 exact
No row exposed a defect: no wrong number, no overwritten sentinel, no NaN read.  Wall time of the file: 9 s for its 206 cases (the slowest case,
1.1 s, is the first launch of a process).

That the file can fail - each mutation built from a copy outside the repository and run once; all give wrong numbers from in-bounds
accesses only.  Red rows of this file / `test_conv3_thin_and_head_and_patch_embed` of tests/test_hip_kernels.py:
  1. the stem kernels' `brick += gridDim.x` loops ended after their first brick: the five stem `*-wrap-*` rows (mfma and brick forward, mfma
     and both brick weight gradients) / old test GREEN;
  2. the stem forward's edge guard as `ww < W - 1`: all 18 `stem_fwd-mfma-*` and `stem_fwd-brick-*` rows / old test red;
  3. the patch-embed team kernel's `ci == 0` on dbias dropped: the atomic-route team rows with Cin > 1 and a dbias
     (`patch_bwd-team-cout48-cin4-f32`, `-cout24-cin4-bf16`, `-team-b2-slice-*`) / old test GREEN;
  4. the head team weight gradient's second pass not launched: the seven team rows with Cout 9 / 16 (`-48to9-*`, `-48to16-*`,
     `-s210-48to9`, `-s210-48to16`, `-96to9-slices`, both `no-dbias`) / old test GREEN;
  5. both partial-sum reduces started at block 1: the three `stem_wgrad-mfma-*` rows on the partial route and the six
     `patch_bwd-team-*partial*` rows / old test red;
  6. the head tile kernels' `b = v0 / S` taken as 0: `head_fwd-tile-b2-s210-*` and the five B = 2 rows of the tile dx / matrix-core dw
     kernels (`-b2-s512`, `-dx-slice`, `-96to6`, `-48to16`, `mfma-no-dx-no-dbias`) / old test red."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import net_end_cases as NE
from layouts import SENT, _bits, assert_untouched, place_in, place_out
from parity import assert_parity, local_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {"f32": 2e-4, "bf16": 2e-2}
HEAD_DBIAS_TOL = 1e-4
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
GUARD = 64             # fp32 sentinel elements before and behind dw / dbias / the head's NCDHW output (a multiple of 4: the view stays 16-byte aligned)
WORST = {}             # (op, dtype, quantity) -> [pooled, local, local_tol rule used]


def _ops():
    from mi_seg_amd.hip import ops
    return ops


def _L():
    from mi_seg_amd.hip import lib
    return lib


def rnd(*shape, dtype=torch.float32, seed=0, scale=1.0):
    big = 1
    for v in shape:
        big *= v
    if big > 1 << 20:          # the loop-wrapping shapes: drawn on the device
        g = torch.Generator(device=DEV).manual_seed(seed + 7 * sum(shape))
        return (torch.randn(*shape, generator=g, device=DEV) * scale).to(dtype)
    g = torch.Generator().manual_seed(seed + 7 * sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


def image(B, Cin, D, H, W, seed):
    """the NCDHW fp32 network input inside a NaN-filled allocation: two depth slabs (and a row, and a voxel) of NaN before and behind"""
    n = B * Cin * D * H * W
    pad = -(-(2 * H * W + W + 1) // 4) * 4
    buf = torch.full((pad + n + pad,), float("nan"), device=DEV)
    x = buf[pad:pad + n].view(B, Cin, D, H, W)
    x.copy_(rnd(B, Cin, D, H, W, seed=seed))
    if B == 2:
        assert not torch.equal(x[0], x[1])
    return x


class Guarded:
    """a contiguous fp32 tensor between two runs of GUARD sentinels"""

    def __init__(self, values=None, shape=None, fill=SENT):
        shape = tuple(values.shape) if values is not None else tuple(shape)
        n = 1
        for v in shape:
            n *= v
        self.buf = torch.full((GUARD + n + GUARD,), SENT, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        self.t.copy_(values) if values is not None else self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0

    def check(self, what):
        g = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]])
        assert bool((g == SENT).all()), f"{what}: a sentinel beside the buffer was overwritten"


def nan_wrapped(values):
    """an NCDHW fp32 input (the head's dy) with NaN before and behind"""
    n = values.numel()
    buf = torch.full((GUARD + n + GUARD,), float("nan"), device=DEV)
    t = buf[GUARD:GUARD + n].view(values.shape)
    t.copy_(values)
    return t


def addr(t):
    return int(t.data_ptr()) if t is not None else 0


def _note(r, quantity, pooled, loc, rule):
    w = WORST.setdefault((r["op"], r["dt"], quantity), [0.0, 0.0, 0])
    w[0], w[1], w[2] = max(w[0], pooled), max(w[1], loc), w[2] + int(rule)


def parity(r, quantity, got, ref, tol, compose=None):
    """assert_parity at `tol`; a bf16 result beyond the per-element bound is judged by the local_tol rule: at most twice the
    local error of torch's own bf16 composition `compose()` against the same reference - never below tol, and the pooled check keeps tol"""
    what = f"{r['id']} {quantity}"
    try:
        pooled, loc = assert_parity(got, ref, tol, what)
        rule = False
    except AssertionError:
        if compose is None or r["dt"] != "bf16":
            raise
        lt = max(tol, 2 * local_err(compose().double(), ref)[0])
        pooled, loc = assert_parity(got, ref, tol, what, local_tol=lt)
        rule = True
    print(f"PARITY {what}: pooled {pooled:.3e} local {loc:.3e}{' (local_tol rule)' if rule else ''}")
    _note(r, quantity, pooled, loc, rule)


def same_bits(a, b, what):
    assert torch.equal(_bits(a.contiguous()), _bits(b.contiguous())), f"{what}: two runs of a launch with a fixed order of summation differ"


def check_layout(r, view, c, lay):
    off, ld = NE.layout(c, r["dt"], lay)
    assert view.stride(-2) == ld and (view.data_ptr() % 16 == 0) == (lay != "off8"), (r["id"], view.stride(), ld)


def launch(r, a):
    """plan first (it must name the form the row is there for), then the call itself, on the same params"""
    L, ops = _L(), _ops()
    prm = NE.params(r, L, a)
    rc, pl = NE.plan(r, L, prm)
    NE.check_plan(r, L, rc, pl)
    ops._call(NE.CALL_FN[r["op"]], prm)
    return pl


def rows_of(op):
    return [r for r in NE.ROWS if r["op"] == op]


def _ids(r):
    return r["id"]


# ---------------------------------------------------------------------------------------------------------------- stem
@pytest.mark.parametrize("r", rows_of("stem_fwd"), ids=_ids)
def test_stem_forward(r):
    B, Cin, Cout, (D, H, W), dt = r["B"], r["Cin"], r["Cout"], r["dims"], TD[r["dt"]]
    x, w = image(B, Cin, D, H, W, seed=51), rnd(Cout, Cin, 3, 3, 3, seed=52) / 5
    outs = []
    for _ in range(2):
        y = place_out((B, D, H, W, Cout), dt, r["lay"])
        check_layout(r, y.view, Cout, r["lay"])
        launch(r, {"x": addr(x), "y": addr(y.view), "w": addr(w)})
        assert_untouched(y, r["id"])
        outs.append(y.view)
    same_bits(outs[0], outs[1], r["id"])
    ref = F.conv3d(x.double(), w.double(), padding=1)
    parity(r, "y", outs[0].permute(0, 4, 1, 2, 3), ref, TOL[r["dt"]], lambda: F.conv3d(x.bfloat16(), w.bfloat16(), padding=1))


@pytest.mark.parametrize("r", rows_of("stem_wgrad"), ids=_ids)
def test_stem_weight_gradient(r):
    L = _L()
    B, Cin, Cout, (D, H, W), dt = r["B"], r["Cin"], r["Cout"], r["dims"], TD[r["dt"]]
    x = image(B, Cin, D, H, W, seed=53)
    dy = place_in(rnd(B, D, H, W, Cout, dtype=dt, seed=54), r["lay"])
    check_layout(r, dy, Cout, r["lay"])
    base = rnd(Cout, Cin, 3, 3, 3, seed=55)
    nb = L.load().miseg_conv3_thin_wgrad_workspace_bytes(C.byref(NE.params(r, L, NE.standins(r))))
    assert (nb > 0) == (r["k"] == "NE_STEM_WGRAD_MFMA")
    outs = []
    for _ in range(2):
        dw = Guarded(base)
        ws = Guarded(shape=(max(nb // 4, 4),), fill=float("nan")) if r["ws"] else None
        pl = launch(r, {"x": addr(x), "dy": addr(dy), "dw": addr(dw.t), "ws": addr(ws.t) if ws else 0})
        dw.check(r["id"])
        if ws:
            ws.check(r["id"] + " workspace")
        outs.append(dw.t)
    if pl.partial:
        same_bits(outs[0], outs[1], r["id"])
    dyd = dy.double().permute(0, 4, 1, 2, 3)
    ref = torch.nn.grad.conv3d_weight(x.double(), base.shape, dyd, padding=1)
    parity(r, "dw", outs[0] - base, ref, TOL[r["dt"]],
           lambda: torch.nn.grad.conv3d_weight(x.bfloat16(), base.shape, dy.permute(0, 4, 1, 2, 3).contiguous(), padding=1))


# ---------------------------------------------------------------------------------------------------------------- patch embedding
@pytest.mark.parametrize("r", rows_of("patch_fwd"), ids=_ids)
def test_patch_embed_forward(r):
    B, Cin, Cout, (D, H, W), dt = r["B"], r["Cin"], r["Cout"], r["dims"], TD[r["dt"]]
    x, w = image(B, Cin, D, H, W, seed=56), rnd(Cout, Cin, 2, 2, 2, seed=57) / 3
    bias = rnd(Cout, seed=58) if r["bias"] else None
    outs = []
    for _ in range(2):
        y = place_out((B, D // 2, H // 2, W // 2, Cout), dt, r["lay"])
        check_layout(r, y.view, Cout, r["lay"])
        launch(r, {"x": addr(x), "y": addr(y.view), "w": addr(w), "bias": addr(bias)})
        assert_untouched(y, r["id"])
        outs.append(y.view)
    same_bits(outs[0], outs[1], r["id"])
    ref = F.conv3d(x.double(), w.double(), bias.double() if r["bias"] else None, stride=2)
    parity(r, "y", outs[0].permute(0, 4, 1, 2, 3), ref, TOL[r["dt"]],
           lambda: F.conv3d(x.bfloat16(), w.bfloat16(), bias.bfloat16() if r["bias"] else None, stride=2))


@pytest.mark.parametrize("r", rows_of("patch_bwd"), ids=_ids)
def test_patch_embed_backward(r):
    L = _L()
    B, Cin, Cout, (D, H, W), dt = r["B"], r["Cin"], r["Cout"], r["dims"], TD[r["dt"]]
    x = image(B, Cin, D, H, W, seed=59)
    dy = place_in(rnd(B, D // 2, H // 2, W // 2, Cout, dtype=dt, seed=60), r["lay"])
    check_layout(r, dy, Cout, r["lay"])
    base_w, base_b = rnd(Cout, Cin, 2, 2, 2, seed=61), rnd(Cout, seed=62)
    nb = L.load().miseg_patch_embed_bwd_workspace_bytes(C.byref(NE.params(r, L, NE.standins(r))))
    assert nb == 256 * Cin * 9 * Cout * 4
    outs = []
    for _ in range(2):
        dw, db = Guarded(base_w), Guarded(base_b)
        ws = Guarded(shape=(nb // 4,), fill=float("nan")) if r["ws"] else None
        pl = launch(r, {"x": addr(x), "dy": addr(dy), "dw": addr(dw.t), "dbias": addr(db.t) if r["dbias"] else 0, "ws": addr(ws.t) if ws else 0})
        for g, what in ((dw, "dw"), (db, "dbias"), (ws, "workspace")):
            if g is not None:
                g.check(f"{r['id']} {what}")
        outs.append((dw.t, db.t))
    if pl.partial:
        same_bits(outs[0][0], outs[1][0], r["id"] + " dw")
        same_bits(outs[0][1], outs[1][1], r["id"] + " dbias")
    dyd = dy.double().permute(0, 4, 1, 2, 3)
    parity(r, "dw", outs[0][0] - base_w, torch.nn.grad.conv3d_weight(x.double(), base_w.shape, dyd, stride=2), TOL[r["dt"]],
           lambda: torch.nn.grad.conv3d_weight(x.bfloat16(), base_w.shape, dy.permute(0, 4, 1, 2, 3).contiguous(), stride=2))
    if r["dbias"]:
        parity(r, "dbias", outs[0][1] - base_b, dy.double().sum((0, 1, 2, 3)), TOL[r["dt"]], lambda: dy.sum((0, 1, 2, 3)))
    else:
        assert torch.equal(outs[0][1], base_b), f"{r['id']}: dbias is NULL, the buffer beside dw changed"


# ---------------------------------------------------------------------------------------------------------------- head
def _head_operands(r, seed):
    B, Cin, Cout, (D, H, W), dt = r["B"], r["Cin"], r["Cout"], r["dims"], TD[r["dt"]]
    xv = rnd(B, D, H, W, Cin, dtype=dt, seed=seed)
    if B == 2:
        assert not torch.equal(xv[0], xv[1])
    x = place_in(xv, r["lay"])
    check_layout(r, x, Cin, r["lay"])
    return x, rnd(Cout, Cin, 1, 1, 1, seed=seed + 1) / 7


@pytest.mark.parametrize("r", rows_of("head_fwd"), ids=_ids)
def test_head_forward(r):
    B, Cout, (D, H, W) = r["B"], r["Cout"], r["dims"]
    x, w = _head_operands(r, 63)
    bias = rnd(Cout, seed=65) if r["bias"] else None
    outs = []
    for _ in range(2):
        y = Guarded(shape=(B, Cout, D, H, W), fill=float("nan"))
        launch(r, {"x": addr(x), "y": addr(y.t), "w": addr(w), "bias": addr(bias)})
        y.check(r["id"])
        outs.append(y.t)
    same_bits(outs[0], outs[1], r["id"])
    xd = x.double().permute(0, 4, 1, 2, 3)
    ref = F.conv3d(xd, w.double(), bias.double() if r["bias"] else None)
    # the head's output is fp32 whatever the activations' dtype: torch's own composition is the fp32 convolution of the same bf16 activations
    parity(r, "y", outs[0], ref, TOL[r["dt"]], lambda: F.conv3d(x.float().permute(0, 4, 1, 2, 3), w, bias))


@pytest.mark.parametrize("r", rows_of("head_bwd"), ids=_ids)
def test_head_backward(r):
    B, Cin, Cout, (D, H, W), dt = r["B"], r["Cin"], r["Cout"], r["dims"], TD[r["dt"]]
    x, w = _head_operands(r, 66)
    gv = rnd(B, Cout, D, H, W, seed=68)
    if B == 2:
        assert not torch.equal(gv[0], gv[1])
    dy = nan_wrapped(gv)
    base_w, base_b = rnd(Cout, Cin, 1, 1, 1, seed=69), rnd(Cout, seed=70)
    outs = []
    for _ in range(2):
        dx = place_out((B, D, H, W, Cin), dt, r["lay_dx"]) if r["dx"] else None
        if dx is not None:
            check_layout(r, dx.view, Cin, r["lay_dx"])
        dw, db = Guarded(base_w), Guarded(base_b)
        launch(r, {"x": addr(x), "dy": addr(dy), "dx": addr(dx.view) if dx is not None else 0, "w": addr(w), "dw": addr(dw.t) if r["dw"] else 0,
                   "dbias": addr(db.t) if r["dbias"] else 0})
        if dx is not None:
            assert_untouched(dx, r["id"] + " dx")
        dw.check(r["id"] + " dw")
        db.check(r["id"] + " dbias")
        outs.append((dx.view if dx is not None else None, dw.t, db.t))
    if r["dx"]:
        same_bits(outs[0][0], outs[1][0], r["id"] + " dx")
        ref = torch.nn.grad.conv3d_input((B, Cin, D, H, W), w.double(), dy.double())
        parity(r, "dx", outs[0][0].permute(0, 4, 1, 2, 3), ref, TOL[r["dt"]], lambda: torch.nn.grad.conv3d_input((B, Cin, D, H, W), w, dy).to(dt))
    if r["dw"]:
        xd = x.double().permute(0, 4, 1, 2, 3)
        parity(r, "dw", outs[0][1] - base_w, torch.nn.grad.conv3d_weight(xd, base_w.shape, dy.double()), TOL[r["dt"]],
               lambda: torch.nn.grad.conv3d_weight(x.permute(0, 4, 1, 2, 3).contiguous(), base_w.shape, dy.to(dt)))
    else:
        assert torch.equal(outs[0][1], base_w), f"{r['id']}: dw is NULL, the buffer changed"
    if r["dbias"]:
        parity(r, "dbias", outs[0][2] - base_b, dy.double().sum((0, 2, 3, 4)), HEAD_DBIAS_TOL)
    else:
        assert torch.equal(outs[0][2], base_b), f"{r['id']}: dbias is NULL, the buffer beside dw changed"


# ---------------------------------------------------------------------------------------------------------------- im2col3 / col2im3
IM2COL = [(dt, c, grid, B, ls, ld) for dt in ("f32", "bf16") for (c, grid, B, ls, ld) in [
    (8, (2, 3, 5), 2, "contig", "contig"), (6, (2, 3, 5), 2, "contig", "contig"), (8, (1, 1, 1), 1, "contig", "contig"), (6, (1, 1, 1), 2, "contig", "contig"),
    (8, (2, 3, 5), 1, "slice", "contig"), (8, (2, 3, 5), 1, "contig", "slice"), (8, (2, 3, 5), 2, "ldodd", "contig"), (8, (2, 3, 5), 2, "contig", "ldodd"),
    (8, (2, 3, 5), 1, "off8", "slice"), (6, (2, 3, 5), 1, "slice", "ldodd")]]


def _taps(xp, D, H, W):
    return torch.cat([xp[:, a:a + D, b:b + H, c:c + W, :] for a in range(3) for b in range(3) for c in range(3)], -1)


@pytest.mark.parametrize("case", IM2COL, ids=lambda c: f"{c[0]}-C{c[1]}-{'x'.join(map(str, c[2]))}-B{c[3]}-{c[4]}-{c[5]}")
def test_im2col3_and_col2im3(case):
    L, ops = _L(), _ops()
    dtn, Cc, (D, H, W), B, ls, ld = case
    dt = TD[dtn]
    xv = rnd(B, D, H, W, Cc, dtype=dt, seed=71)
    x = place_in(xv, ls)
    cols = []
    for _ in range(2):
        col = place_out((B, D, H, W, 27 * Cc), dt, ld)
        ops._call("miseg_im2col3", L.Im2col3(addr(x), x.stride(-2), addr(col.view), col.view.stride(-2), B, D, H, W, Cc, L.BF16 if dtn == "bf16" else L.F32))
        assert_untouched(col, "im2col3")
        cols.append(col.view)
    assert torch.equal(cols[0], _taps(F.pad(xv, (0, 0, 1, 1, 1, 1, 1, 1)), D, H, W)) and torch.equal(cols[0], cols[1])      # pure data movement: exact
    # the adjoint: col (27 C channels, layout ls) -> [B, D, H, W, C] (layout ld)
    cv = rnd(B, D, H, W, 27 * Cc, dtype=dt, seed=72)
    cin = place_in(cv, ls)
    backs = []
    for _ in range(2):
        back = place_out((B, D, H, W, Cc), dt, ld)
        ops._call("miseg_col2im3", L.Im2col3(addr(cin), cin.stride(-2), addr(back.view), back.view.stride(-2), B, D, H, W, Cc, L.BF16 if dtn == "bf16" else L.F32))
        assert_untouched(back, "col2im3")
        backs.append(back.view)
    same_bits(backs[0], backs[1], "col2im3")
    xr = torch.zeros(B, D, H, W, Cc, dtype=torch.float64, device=DEV, requires_grad=True)
    _taps(F.pad(xr, (0, 0, 1, 1, 1, 1, 1, 1)), D, H, W).backward(cv.double())
    r = {"id": f"col2im3-{dtn}", "op": "col2im3", "dt": dtn}
    parity(r, "dst", backs[0], xr.grad, TOL[dtn])


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refused_problems_return_their_code_before_any_launch():
    """the output buffer keeps its sentinel: nothing was launched"""
    L = _L()
    lib = L.load()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = image(1, 4, 8, 8, 8, seed=73)
    big = lambda n: torch.full((n,), SENT, device=DEV)      # noqa: E731
    out, w, dy = big(1 << 16), rnd(1 << 15, seed=74), rnd(1 << 14, seed=75)
    BADARG, UNSUPPORTED = -1, -2
    a = addr
    cases = [
        ("miseg_patch_embed_fwd", L.PatchEmbed(a(x), a(out), 24, a(w), a(w), 1, 1, 8, 7, 8, 24, L.F32), BADARG),                  # an odd grid side
        ("miseg_patch_embed_fwd", L.PatchEmbed(a(x), a(out), 24, a(w), a(w), 1, 1, 8, 8, 5, 24, L.BF16), BADARG),
        ("miseg_patch_embed_fwd", L.PatchEmbed(a(x), a(out), 376, a(w), a(w), 1, 4, 8, 8, 8, 376, L.F32), UNSUPPORTED),            # Cin * 8 * Cout > 12000
        ("miseg_patch_embed_fwd", L.PatchEmbed(a(x), a(out), 24, 0, a(w), 1, 1, 8, 8, 8, 24, L.F32), BADARG),                       # w NULL
        ("miseg_patch_embed_bwd", L.PatchEmbedBwd(a(x), a(dy), 64, a(out), a(out) + 65536, 1, 4, 8, 8, 8, 64, L.F32, 0), UNSUPPORTED),
        ("miseg_patch_embed_bwd", L.PatchEmbedBwd(0, a(dy), 24, a(out), a(out) + 65536, 1, 1, 8, 8, 8, 24, L.F32, 0), BADARG),
        ("miseg_conv3_thin_fwd", L.Conv3Thin(a(x), a(out), 8, a(w), 1, 5, 8, 8, 8, 8, L.F32), UNSUPPORTED),                          # Cin 5
        ("miseg_conv3_thin_fwd", L.Conv3Thin(a(x), a(out), 140, a(w), 1, 4, 4, 4, 4, 140, L.F32), UNSUPPORTED),                      # Cin * 27 * Cout > 15000
        ("miseg_conv3_thin_fwd", L.Conv3Thin(0, a(out), 8, a(w), 1, 1, 8, 8, 8, 8, L.F32), BADARG),
        ("miseg_conv3_thin_wgrad", L.Conv3ThinWgrad(a(x), a(dy), 8, a(out), 1, 5, 8, 8, 8, 8, L.F32, 0), UNSUPPORTED),
        ("miseg_conv3_thin_wgrad", L.Conv3ThinWgrad(a(x), a(dy), 72, a(out), 1, 1, 4, 4, 4, 72, L.F32, 0), UNSUPPORTED),             # Cout > 64
        ("miseg_conv3_thin_wgrad", L.Conv3ThinWgrad(a(x), 0, 8, a(out), 1, 1, 8, 8, 8, 8, L.F32, 0), BADARG),
        ("miseg_head_fwd", L.Head(a(w), 48, a(out), a(w), a(w), 1, 64, 48, 17, L.F32), UNSUPPORTED),                                 # Cout 17
        ("miseg_head_fwd", L.Head(a(w), 520, a(out), a(w), a(w), 1, 8, 520, 16, L.F32), UNSUPPORTED),                                # Cin * Cout > 8192
        ("miseg_head_fwd", L.Head(0, 48, a(out), a(w), a(w), 1, 64, 48, 6, L.F32), BADARG),
        ("miseg_head_bwd", L.HeadBwd(a(w), 48, a(dy), a(out), 48, a(w), a(out) + 65536, a(out) + 131072, 1, 64, 48, 17, L.F32), UNSUPPORTED),
        ("miseg_head_bwd", L.HeadBwd(a(w), 64, a(dy), a(out), 64, a(w), a(out) + 65536, a(out) + 131072, 1, 64, 64, 16, L.F32), UNSUPPORTED),
        ("miseg_head_bwd", L.HeadBwd(a(w), 48, 0, a(out), 48, a(w), a(out) + 65536, a(out) + 131072, 1, 64, 48, 6, L.F32), BADARG),
        ("miseg_head_bwd", L.HeadBwd(a(w), 48, a(dy), a(out), 48, a(w), a(out) + 65536, a(out) + 131072, 1, 64, 48, 6, 5), BADARG),  # unknown dtype
    ]
    for fn, prm, code in cases:
        pl = L.HeadBwdPlan() if fn == "miseg_head_bwd" else L.NetEndLaunch()
        assert getattr(lib, fn + "_plan")(C.byref(prm), C.byref(pl)) == code, (fn, lib.miseg_last_error())
        assert getattr(lib, fn)(C.byref(prm), s) == code, (fn, lib.miseg_last_error())
    torch.cuda.synchronize()
    assert bool((out == SENT).all()), "a refused call wrote to its output"


def test_zz_report_the_worst_errors():
    """prints the error table of this run (pytest -s): op, dtype, quantity, worst pooled and per-element error, rows judged by the local_tol rule"""
    for (op, dt, q), (pooled, loc, rule) in sorted(WORST.items()):
        bar = HEAD_DBIAS_TOL if (op == "head_bwd" and q == "dbias") else TOL[dt]
        print(f"WORST {op:10s} {dt:4s} {q:5s} pooled {pooled:.2e} local {loc:.2e} bar {bar:.0e} local_tol-rule rows {rule}")
        assert pooled < bar
