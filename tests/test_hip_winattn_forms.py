"""Geometry, launch forms, options and layouts of the attention kernels (csrc/attention.hip, csrc/attention_global.hip): the query-lane
kernels (any head_dim, both dtypes), the bf16 head_dim-16 matrix-core pair (forward with 8 or 11 waves, with or without shift mask and
dropout; backward with or without mask, table gradient and dropout; vector or scalar operand loads) and the bf16 head_dim-64 global pair
(eight tile counts).  Every case stands against the float64 reference of tests/winattn_ref.py on the same fp32 or bf16-rounded inputs
(pinned on the CPU by tests/test_winattn_ref_cpu.py, which also shows that the inputs leave a model of the matrix-core rounding points
below half of every bar on `out`), pooled and per element (parity.assert_parity); forward and backward run twice and `out`, `lse`, `dqkv`
must repeat bit for bit (`dtable` and `dqkv_bias` end in float atomics across workgroups: parity only); before each launch the library's plan
(miseg_winattn_fwd_plan / _bwd_plan) must equal, field for field, the hand-derived row of tests/winattn_cases.py for that call - kernel
family, template arguments, vec, grid, threads, LDS, units - and miseg_winattn_on_matrix_cores / miseg_winattn_bwd_on_matrix_cores must
answer as that plan; `out`, `lse`, `dqkv` start NaN-filled (a skipped row stays NaN) or, as
views, inside sentinel-filled buffers that must survive outside the view.

form -> case (winattn_ref.GEOMETRY unless said)
  forward matrix cores <MASK, waves, DROP>
    <0, 11, 0>  7x7x4 / 4x7x7 unshifted, n = 32 / 64 / 320 / 352, 1 and 9 units       <0, 11, 1>  options 6x6x6, p = 0.25
    <1, 11, 0>  per-axis shifts, n = 48 / 64, 27 and 192 units                        <1, 11, 1>  options 10x9x8, p = 0.25
    <1,  8, 0>  270 units (production form), 256 units at n = 64                      <1,  8, 1>  270 units, p = 0.25
    <0,  8, 0>  test_unshifted_grids_at_the_wave_boundary (16^3 in windows of 4^3, 4 heads = 256 units), <0, 8, 1> the same with p = 0.25
  backward matrix cores <MASK, DT, DROP>: test_options walks mask (10x9x8 shifted / 6x6x6) x table gradient x dropout = all eight;
    no tail tile n = 32 / 48 / 64 / 320 / 352; the tail tile in a wave's slot 0 (n = 8: wave 0, n = 27: wave 1), 1 (n = 216: wave 5), 2 (n = 343: wave 5)
  scalar-load forms (vec = false): test_layouts off8 / ldodd on qkv, out, dout
  cross-kernel pairs: test_layouts out-ldodd (query-lane forward, matrix-core backward), qkv-ldodd and dqkv-ldodd (matrix-core forward,
    query-lane backward), n = 352 with a 15^3 table (the same, by the table's size); each pair also with dropout
  query-lane kernels: every fp32 case; bf16 at n = 360 / 384 (384 threads); head_dim 8 / 12 / 32 / 64 and bf16 16 without a table
    (test_head_dims); head_dim 4 and 16: tests/test_hip_kernels.py and every fp32 head_dim-16 case here
  global kernels NP / 16: 2 (n = 1, 2), 6 (n = 80), 10 (n = 150), 12 (n = 180) here; 2, 4, 8, 14, 16 in tests/test_hip_kernels.py;
    n = 288 > GA_MAXN and the layout declines fall to the query-lane head_dim-64 kernels (test_global_*)
  att_unit with a remainder: 9, 27, 270 units (1, 256, 192 without)
  refusals, all returned by the host before any launch: test_refusals_return_before_any_launch

Tolerances are those of the existing tests of the same calls: out 2e-4 (fp32) / 2e-2 (bf16), gradients 2e-4 / 4e-2, dqkv_bias twice that,
the per-element bound of bf16 dqkv max(tol, 2 x the local error of torch's own bf16 composition) (winattn_ref.dqkv_local_tol, DESIGN.md
section 3).  No pooled bar was raised.  lse: max |lse - float64 lse| <= 2 x the yardstick of the kernel family that ran, computed on the
same inputs (winattn_ref.lse_yardstick: torch's fp32 logsumexp for the fp32 kernels and the bf16 query-lane kernels, the rounding model for
the bf16 matrix-core kernels).

Measured on the card, worst over the file, fp32 / bf16 (pooled; local): out 3.8e-7 / 2.5e-3; 1.6e-6 / 9.7e-3 - dqkv 1.5e-6 / 4.1e-3;
2.2e-5 / 3.4e-2 (the bf16 figure at table amplitude 4; bar 4e-2, so no case took the yardstick route) - dtable 1.3e-6 / 4.4e-3; 2.7e-5 /
2.1e-2 - dqkv_bias 6.6e-7 / 1.2e-3; 1.2e-6 / 2.5e-3.  lse, kernel against its yardstick (worst ratio of the two over the cases): fp32
query-lane kernels 2e-7 .. 9.8e-6 against 2e-7 .. 1.0e-5 (1.5); bf16 query-lane kernels <= 8.7e-7 against <= 9.2e-7 (1.2); bf16 matrix-core
kernels 1e-4 .. 1.9e-3 against the same figures of the rounding model (1.0).  The first run of this file found the query-lane forward at
1.6 .. 3.2 times its yardstick (fp32, table amplitude 4: 2.59e-6 against 1.00e-6; bf16 without a table: 2.63e-6 against 8.2e-7): it summed
the softmax denominator one key at a time in fp32.  The log-sum-exp now takes the denominator from a second sum in double
(csrc/attention.hip, winattn_fwd_kernel); `out` keeps the fp32 sum, and with it its bits.

Mutations, each built from a scratch copy and run once against this file and the attention tests of tests/test_hip_kernels.py (which stay
green under every one): the last unit of att_unit's remainder form mapped away -> the 9 / 12 / 27 / 270-unit cases; the forward's full-tile
count taken as ntiles - 1 also for n % 32 == 0 -> every such case; lse in log2 units in the matrix-core forward and backward alike -> every
lse value and the cross-kernel pairs; one axis' region label cut at another axis' shift -> the (0, 3, 3) shift.  Dropping the `g.sd ?` guard
of token_info changes nothing observable: without a shift on an axis the label is constant inside every window."""
import ctypes as C
import functools

import pytest
import torch

import winattn_cases as G
import winattn_ref as W
from layouts import SENT, assert_untouched, place_in
from parity import assert_parity

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
S = W.Spec


def _ops():
    from mi_seg_amd.hip import ops
    return ops


def _L():
    from mi_seg_amd.hip import lib
    return lib


def _name(dt):
    return {F32: "fp32", BF: "bf16"}[dt]


def _id(v):
    return _name(v) if isinstance(v, torch.dtype) else str(v)


@functools.lru_cache(maxsize=1)
def _key():
    """a dropout key of this file's own (seed, call-site id, device step counter): drawing from ops.DROP would shift the masks of later tests"""
    return (0x5EED0FA77E, 11, torch.zeros(1, dtype=torch.int64, device=DEV))


@functools.lru_cache(maxsize=4)
def _case(spec, dtype):
    return W.Case(spec, dtype, device=DEV)


@functools.lru_cache(maxsize=4)
def _ref(spec, dtype, drop_p):
    """the float64 reference of a case (with the mask miseg_dropout draws for this file's key), computed once on the device and shared;
    ["yard"]: the lse yardsticks of both kernel families, ["dqkv_tol"]: the per-element bound of dqkv"""
    ops = _ops()
    c = _case(spec, dtype)
    mask = None
    if drop_p:
        n = spec.n
        mask = ops.dropout_apply(torch.ones(spec.windows * spec.heads * n, n, device=DEV), drop_p, _key()).view(spec.windows, spec.heads, n, n)
        kept = float((mask != 0).float().mean())
        assert abs(kept - (1 - drop_p)) < 0.02 + 2.0 / n, kept
    r = c.reference(drop_mask=mask)
    args = (c.qkv, c.qb, c.table, spec.heads, spec.ws, spec.ss, spec.tw, spec.scale, r["lse"])
    r["yard"] = {0: W.lse_yardstick("fp32", *args), 1: W.lse_yardstick("mfma", *args) if dtype == BF else None}
    tol = W.TOL[dtype] * (2 if dtype == BF else 1)
    r["dqkv_tol"] = W.dqkv_local_tol(tol, c.qkv, c.qb, c.table, c.dout, spec.heads, spec.ws, spec.ss, spec.scale, r["dqkv"], drop_mask=mask, tw=spec.tw)
    return r


_CODE = {F32: G.F32, BF: G.BF16}


def _forms(spec, dtype, drop_p=0.0, lay=None, want_dtable=True, want_dqb=True):
    """(forward, backward) launch forms of a call - G.ql(hd4, waves) / G.win(waves, vec) / G.glob(tiles, grid_x) - from the hand-derived table of
    tests/winattn_cases.py (pinned on the CPU by tests/test_winattn_plan_cpu.py)"""
    return G.find(spec, _CODE[dtype], drop_p, lay, want_dtable, want_dqb)


def _expected(spec, dtype):
    """(forward, backward) on the matrix cores for contiguous operands: the table's rows"""
    return tuple(int(f[0] != "ql") for f in _forms(spec, dtype))


def _assert_plan(pl, spec, dtype, form, bwd, drop_p, want_dtable, what):
    want = G.expected(spec, _CODE[dtype], form, bwd, drop_p, want_dtable)
    got = {k: getattr(pl, k) for k in want}
    assert got == want, f"{what}: the {'backward' if bwd else 'forward'} plan {got} is not the table's {want}"


def _in(t, lay):
    return t if lay in (None, "contig") else place_in(t, lay)


def _report(what, dtype, name, pooled, loc, bound=None):
    print(f"WINATTN {_name(dtype)} {name} pooled {pooled:.3e} local {loc:.3e}" + (f" bound {bound:.3e}" if bound is not None else "") + f" | {what}")


def run(spec, dtype, drop_p=0.0, lay=None, expect=None, want_dtable=True, want_dqb=True):
    """forward and backward of one case, each twice: kernel choice, parity of out / lse / dqkv / dtable / dqkv_bias with float64, bit-identical
    reruns, nothing written outside a view.  lay: {"qkv" | "out" | "dout" | "dqkv": layout}.  Returns the first run's dqkv (contiguous copy)."""
    ops, L = _ops(), _L()
    lib = L.load()
    lay = lay or {}
    c, ref = _case(spec, dtype), _ref(spec, dtype, drop_p)
    what = f"{spec} {_name(dtype)} p={drop_p} {lay or ''}"
    form_f, form_b = _forms(spec, dtype, drop_p, lay, want_dtable, want_dqb)
    exp_f, exp_b = int(form_f[0] != "ql"), int(form_b[0] != "ql")
    assert expect is None or tuple(expect) == (exp_f, exp_b), f"{what}: the test expects {expect} on the matrix cores, the table {form_f} / {form_b}"
    drop = (drop_p, _key()) if drop_p else None
    qkv, dout = _in(c.qkv, lay.get("qkv")), _in(c.dout, lay.get("dout"))
    tol = W.TOL[dtype]
    gtol = tol * (2 if dtype == BF else 1)

    def forward():
        out = W.new_output(c.dout.shape, dtype, lay.get("out", "contig"))
        lse = torch.full((spec.windows, spec.heads, spec.n), float("nan"), device=DEV)
        prm = W.fwd_params(ops, spec, qkv, out.view, c.qb, c.table, lse, drop)
        pl = ops.winattn_fwd_plan(prm)
        _assert_plan(pl, spec, dtype, form_f, 0, drop_p, want_dtable, what)
        assert lib.miseg_winattn_on_matrix_cores(C.byref(prm)) == exp_f == int(pl.kernel != L.WINATTN_QUERY_LANE), f"{what}: forward kernel choice"
        L.check(lib.miseg_winattn_fwd(C.byref(prm), ops._stream()), "winattn_fwd")
        return out, lse, pl

    out, lse, plan_f = forward()
    pooled, loc = assert_parity(out.view, ref["out"], tol, f"{what}: out against float64")
    _report(what, dtype, "out", pooled, loc)
    assert bool(torch.isfinite(lse).all()), f"{what}: {int((~torch.isfinite(lse)).sum())} lse rows were never written"
    lerr, yard = float((lse.double() - ref["lse"]).abs().max()), ref["yard"][int(plan_f.kernel != L.WINATTN_QUERY_LANE)]      # of the kernel family the plan names
    print(f"WINATTN {_name(dtype)} lse{'-mc' if exp_f else '-ql'} err {lerr:.3e} yardstick {yard:.3e} | {what}")
    assert lerr <= 2 * yard, f"{what}: lse off by {lerr:.3e}, allowed 2 x {yard:.3e} (the {'rounding model' if exp_f else 'fp32 logsumexp'})"
    assert_untouched(out, f"{what}: out")
    out2, lse2, _ = forward()
    assert torch.equal(out.view, out2.view) and torch.equal(lse, lse2), f"{what}: the forward does not repeat bit for bit"

    def backward():
        dqkv = W.new_output(c.qkv.shape, dtype, lay.get("dqkv", "contig"))
        dtab = torch.zeros_like(c.table) if (want_dtable and c.table is not None) else None
        dqb = torch.zeros_like(c.qb) if (want_dqb and c.qb is not None) else None
        prm = W.bwd_params(ops, L, spec, qkv, out.view, c.qb, c.table, lse, dout, dqkv.view, dqb, dtab, drop)
        pl = ops.winattn_bwd_plan(prm)
        _assert_plan(pl, spec, dtype, form_b, 1, drop_p, want_dtable, what)
        assert lib.miseg_winattn_bwd_on_matrix_cores(C.byref(prm)) == exp_b == int(pl.kernel != L.WINATTN_QUERY_LANE), f"{what}: backward kernel choice"
        L.check(lib.miseg_winattn_bwd(C.byref(prm), ops._stream()), "winattn_bwd")
        return dqkv, dtab, dqb

    dqkv, dtab, dqb = backward()
    Cc = spec.C
    # the thirds separately: a lost dk must not hide in the pooled norm of the whole.  One key: the softmax is the constant 1, dq = dk = 0
    # identically, and a relative metric of those thirds has no scale - dqkv as a whole then (the scale of dv)
    thirds = [("d" + nm, slice(i * Cc, (i + 1) * Cc)) for i, nm in enumerate("qkv")] if spec.n > 1 else [("dqkv", slice(None))]
    for nm, sl in thirds:
        pooled, loc = assert_parity(dqkv.view[..., sl], ref["dqkv"][..., sl], gtol, f"{what}: {nm} against float64", local_tol=ref["dqkv_tol"])
        _report(what, dtype, nm, pooled, loc, ref["dqkv_tol"])
    if dtab is not None:
        _report(what, dtype, "dtable", *assert_parity(dtab, ref["dtable"], gtol, f"{what}: dtable against float64"))
    if dqb is not None:
        if spec.padded:
            _report(what, dtype, "dqkv_bias", *assert_parity(dqb, ref["dqb"], 2 * gtol, f"{what}: dqkv_bias against float64"))
        else:
            assert float(dqb.abs().max()) == 0.0, f"{what}: dqkv_bias of a grid without padding"
    assert_untouched(dqkv, f"{what}: dqkv")
    dqkv2, _, _ = backward()
    assert torch.equal(dqkv.view, dqkv2.view), f"{what}: the backward does not repeat bit for bit"
    return dqkv.view.contiguous()


# ----------------------------------------------------------------------------------------------------------------- a. geometry
@pytest.mark.parametrize("spec,dtype", [(s, dt) for s, dts in W.GEOMETRY for dt in dts], ids=_id)
def test_geometry(spec, dtype):
    run(spec, dtype)


def test_capacity_edges_pick_the_kernels_the_table_and_the_token_count_allow():
    """n = 352 with a 15^3 table: the forward keeps the matrix cores (its table slot is sized by the launch), the backward's two fixed slots
    of 2200 words do not hold it; above 352 tokens both passes are the query-lane kernels' (384 threads)"""
    by = {s.dims: s for s, _ in W.GEOMETRY}
    assert _expected(by[(11, 8, 4)], BF) == (1, 0) and by[(11, 8, 4)].n == 352
    assert _expected(by[(6, 8, 8)], BF) == (0, 0) and by[(6, 8, 8)].n == 384
    assert _expected(by[(6, 6, 10)], BF) == (0, 0) and by[(6, 6, 10)].n == 360
    assert _expected(W.PRODUCTION, BF) == (1, 1) and W.PRODUCTION.windows * W.PRODUCTION.heads == 270
    assert _forms(by[(11, 8, 4)], BF) == (G.win(11), G.ql(4, 6)) and _forms(by[(6, 8, 8)], BF) == _forms(by[(6, 6, 10)], BF) == (G.ql(4, 6), G.ql(4, 6))


def test_the_production_form_with_dropout():
    """270 units of 343 tokens (the 8-wave forward, a wave owning two query tiles; a remainder in the unit mapping), padded, masked, p = 0.25"""
    spec = W.PRODUCTION
    assert _forms(spec, BF, 0.25) == (G.win(8), G.win(8)) and any(spec.ss) and spec.windows * spec.heads == 270      # forward <1, 8, 1>
    run(spec, BF, drop_p=0.25)


@pytest.mark.parametrize("drop_p", [0.0, 0.25])
def test_unshifted_grids_at_the_wave_boundary(drop_p):
    """256 units without a shift mask: the 8-wave forward's unmasked instantiations"""
    spec = S((16, 16, 16), (4, 4, 4), (0, 0, 0), 4, 64, B=1)
    assert spec.windows * spec.heads == 256 and not any(spec.ss)
    assert _forms(spec, BF, drop_p) == (G.win(8), G.win(8))      # forward <mask 0, waves 8, drop>
    run(spec, BF, drop_p=drop_p)


# ----------------------------------------------------------------------------------------------------------------- b. options
@pytest.mark.parametrize("dtype", [F32, BF], ids=_id)
@pytest.mark.parametrize("drop_p", [0.0, 0.25])
@pytest.mark.parametrize("spec", W.OPTION_SPECS, ids=str)
def test_options(spec, drop_p, dtype):
    """dropout x table gradient {wanted, None} x dqkv_bias {given, None}: every combination against float64, and dqkv the same bits whether or
    not the parameter gradients are asked for (bf16: mask x DT x DROP are the eight backward instantiations of the matrix-core kernel)"""
    full = run(spec, dtype, drop_p=drop_p)
    for want_dtable, want_dqb in ((False, True), (True, False), (False, False)):
        # bf16: <mask, table gradient, 8, dropout> - run() holds each launch's plan to it; fp32: the query lanes
        assert _forms(spec, dtype, drop_p, None, want_dtable, want_dqb) == ((G.win(11), G.win(8)) if dtype == BF else (G.ql(4, G._w(spec.n)),) * 2)
        got = run(spec, dtype, drop_p=drop_p, want_dtable=want_dtable, want_dqb=want_dqb)
        assert torch.equal(full, got), f"dqkv differs with dtable {'given' if want_dtable else 'None'}, dqkv_bias {'given' if want_dqb else 'None'}"


# ----------------------------------------------------------------------------------------------------------------- c. head dims
@pytest.mark.parametrize("spec,dtype", [(s, dt) for s, dts in W.HEAD_DIMS for dt in dts], ids=_id)
def test_head_dims_on_the_query_lane_kernels(spec, dtype):
    assert _expected(spec, dtype) == (0, 0) and _forms(spec, dtype)[0] == _forms(spec, dtype)[1] == G.ql(spec.hd // 4, G._w(spec.n))
    run(spec, dtype)


# ----------------------------------------------------------------------------------------------------------------- d. layouts
# expected (forward, backward) on the matrix cores, bf16 head_dim 16, by operand and layout (fp32: the query-lane kernels throughout):
#   slice: aligned, ld % 8 == 0 - nothing changes;  off8: 8-byte aligned - the matrix cores with scalar loads;
#   ldodd: ld % 4 != 0 - `out` sends the forward to the query lanes (8-byte stores), `qkv` / `dqkv` the backward (8-byte loads / stores),
#   `dout` is only ever read through the staging loads (scalar then)
_LAYOUT_CHOICE = {("out", "ldodd"): (0, 1), ("qkv", "ldodd"): (1, 0), ("dqkv", "ldodd"): (1, 0)}


@pytest.mark.parametrize("dtype", [F32, BF], ids=_id)
@pytest.mark.parametrize("layout", ["slice", "off8", "ldodd"])
@pytest.mark.parametrize("operand", ["qkv", "out", "dout", "dqkv"])
def test_layouts(operand, layout, dtype):
    expect = _LAYOUT_CHOICE.get((operand, layout), (1, 1)) if dtype == BF else (0, 0)
    if dtype == BF and layout == "off8":      # the scalar-load forms: vec = 0 wherever the operand passes through the staging loads
        assert _forms(W.LAYOUT_SPEC, BF, lay={operand: layout}) == {"qkv": (G.win(11, 0), G.win(8, 0)), "out": (G.win(11, 1), G.win(8, 0)),
                                                                    "dout": (G.win(11, 1), G.win(8, 0)), "dqkv": (G.win(11, 1), G.win(8, 1))}[operand]
    run(W.LAYOUT_SPEC, dtype, lay={operand: layout}, expect=expect)


@pytest.mark.parametrize("operand", ["qkv", "out", "dqkv"])
def test_cross_kernel_pairs_draw_the_same_dropout_mask(operand):
    """a query-lane forward with a matrix-core backward and the reverse: the log-sum-exp crosses in natural-log units, and both kernels
    re-create the mask of the same key"""
    expect = _LAYOUT_CHOICE[(operand, "ldodd")]
    assert sum(expect) == 1
    forms = _forms(W.LAYOUT_SPEC, BF, 0.25, {operand: "ldodd"})
    assert sorted(f[0] for f in forms) == ["ql", "win"] and (forms[0][0] == "win") == bool(expect[0])      # one direction query-lane, the other matrix-core
    run(W.LAYOUT_SPEC, BF, drop_p=0.25, lay={operand: "ldodd"}, expect=expect)


# ----------------------------------------------------------------------------------------------------------------- e. global kernels
@pytest.mark.parametrize("drop_p", [0.0, 0.1])
@pytest.mark.parametrize("spec", W.GLOBAL, ids=str)
def test_global_head_dim_64_tile_counts(spec, drop_p):
    assert _expected(spec, BF) == (1, 1) and (spec.n + 31) // 32 * 2 in (2, 6, 10, 12)
    tiles, gx = (spec.n + 31) // 32 * 2, -(-spec.n // 64)
    assert _forms(spec, BF, drop_p) == (G.glob(tiles, gx), G.glob(tiles, 2 * gx))
    run(spec, BF, drop_p=drop_p)


@pytest.mark.parametrize("drop_p", [0.0, 0.1])
def test_global_above_the_token_limit_falls_to_the_query_lanes(drop_p):
    assert W.GLOBAL_ABOVE.n == 288 and _expected(W.GLOBAL_ABOVE, BF) == (0, 0)      # GA_MAXN = 256
    assert _forms(W.GLOBAL_ABOVE, BF, drop_p) == (G.ql(16, 5), G.ql(16, 5))
    run(W.GLOBAL_ABOVE, BF, drop_p=drop_p)


@pytest.mark.parametrize("operand,layout,expect,drop_p", [("qkv", "ldodd", (0, 0), 0.0), ("dout", "off8", (1, 0), 0.0), ("dout", "off8", (1, 0), 0.1),
                                                           ("dqkv", "ldodd", (1, 0), 0.0), ("dqkv", "ldodd", (1, 0), 0.1)])
def test_global_declines_by_layout(operand, layout, expect, drop_p):
    """qkv must be 16-byte aligned with ld % 8 == 0 for either global kernel; dO (16-byte loads) and dqkv (8-byte stores) only bind the
    backward, which then runs on the query lanes behind a global forward"""
    forms = _forms(W.GLOBAL_LAYOUT, BF, drop_p, {operand: layout})
    assert forms == tuple(G.glob(6, 2 * (1 + i)) if e else G.ql(16, 2) for i, e in enumerate(expect))      # a decline: the head_dim-64 query-lane kernel
    run(W.GLOBAL_LAYOUT, BF, drop_p=drop_p, lay={operand: layout}, expect=expect)


# ----------------------------------------------------------------------------------------------------------------- f. refusals
def test_refusals_return_before_any_launch():
    """every call returns MISEG_E_BADARG (-1) or MISEG_E_UNSUPPORTED (-2) from the plan - its geometry checks, the drop_p check, the
    dbias_table guard, the LDS bound or the head_dim set - in front of the launch, and the sentinel-filled outputs keep every element; the
    plan entry point returns the same code and message and names no kernel, and the question entry point answers 0.  All buffers are valid
    and sized for the call."""
    ops, L = _ops(), _L()
    lib = L.load()
    BADARG, UNSUPPORTED = -1, -2

    def attempt(spec, dtype, rc, match, drop=None, table_tw=None, dtable_without_table=False, bwd_only=False):
        B, (D, H, Wd), Cc = spec.B, spec.dims, spec.C
        nw = B * -(-D // spec.ws[0]) * -(-H // spec.ws[1]) * -(-Wd // spec.ws[2])
        qkv = torch.ones(B, D, H, Wd, 3 * Cc, dtype=dtype, device=DEV)
        dout = torch.ones(B, D, H, Wd, Cc, dtype=dtype, device=DEV)
        qb = torch.zeros(3 * Cc, device=DEV)
        tw = table_tw or spec.tw
        table = torch.zeros((2 * max(tw, 7) - 1) ** 3, spec.heads, device=DEV) if spec.table else None
        outs = [torch.full((B, D, H, Wd, Cc), SENT, dtype=dtype, device=DEV), torch.full((nw, spec.heads, spec.n), SENT, device=DEV),
                torch.full((B, D, H, Wd, 3 * Cc), SENT, dtype=dtype, device=DEV), torch.full((3 * Cc,), SENT, device=DEV),
                torch.full(((2 * max(tw, 7) - 1) ** 3, spec.heads), SENT, device=DEV)]
        out, lse, dqkv, dqb, dtab = outs
        f = ops.winattn_params(qkv, out, qb, table, lse, spec.heads, spec.ws, spec.ss, tw, spec.scale, drop)
        b = L.WinattnBwd(f, ops._ptr(dout), Cc, ops._ptr(dqkv), 3 * Cc, ops._ptr(dqb), ops._ptr(dtab if (spec.table or dtable_without_table) else None))
        calls = [("fwd", lib.miseg_winattn_fwd, lib.miseg_winattn_fwd_plan, lib.miseg_winattn_on_matrix_cores, f),
                 ("bwd", lib.miseg_winattn_bwd, lib.miseg_winattn_bwd_plan, lib.miseg_winattn_bwd_on_matrix_cores, b)][1 if bwd_only else 0:]
        for name, fn, plan_fn, asks, prm in calls:
            assert fn(C.byref(prm), ops._stream()) == rc, f"{name} {spec}: {lib.miseg_last_error().decode()}"
            said = lib.miseg_last_error().decode()
            assert match in said, said
            # the plan refuses with the launch's code and text and names no kernel; the question entry point answers 0
            pl = L.WinattnPlan()
            assert plan_fn(C.byref(prm), C.byref(pl)) == rc and lib.miseg_last_error().decode() == said and pl.kernel == L.WINATTN_NONE, f"{name} {spec}"
            assert asks(C.byref(prm)) == 0, f"{name} {spec}: a refused call answered 1"
        torch.cuda.synchronize()
        for t in outs:
            assert bool((t == SENT).all()), f"{spec}: a refused call wrote something"

    for dtype in (F32, BF):
        attempt(S((8, 8, 7), (8, 8, 7), (0, 0, 0), 1, 16, tw=8), dtype, UNSUPPORTED, "max 384 tokens")                 # 448 tokens
        attempt(S((8, 8, 8), (4, 4, 4), (4, 0, 0), 1, 16), dtype, BADARG, "shift must be < window")
        attempt(S((8, 8, 8), (4, 4, 4), (0, 0, 5), 1, 16), dtype, BADARG, "shift must be < window")
        attempt(S((7, 7, 7), (7, 7, 7), (0, 0, 0), 1, 16), dtype, BADARG, "smaller than the 343-token window", table_tw=6)
        attempt(S((4, 4, 4), (4, 4, 4), (0, 0, 0), 2, 40), dtype, UNSUPPORTED, "head_dim 20 not instantiated")
        attempt(S((4, 4, 4), (4, 4, 4), (0, 0, 0), 2, 12), dtype, UNSUPPORTED, "head_dim 6")
        attempt(S((4, 4, 4), (4, 4, 4), (0, 0, 0), 2, 136), dtype, UNSUPPORTED, "head_dim 68")
        attempt(S((6, 6, 6), (6, 6, 6), (0, 0, 0), 3, 48), dtype, BADARG, "must lie in [0, 1)", drop=(1.0, _key()))
        attempt(S((6, 6, 6), (6, 6, 6), (0, 0, 0), 3, 48), dtype, BADARG, "must lie in [0, 1)", drop=(-0.1, _key()))
        # a table gradient without a table: the query-lane kernel has no LDS bins for it (with and without padding, shifted or not)
        attempt(S((6, 6, 6), (6, 6, 6), (0, 0, 0), 3, 48, table=False), dtype, BADARG, "dbias_table given without a bias_table", dtable_without_table=True, bwd_only=True)
        attempt(S((9, 5, 6), (4, 4, 4), (2, 2, 2), 2, 32, table=False), dtype, BADARG, "dbias_table given without a bias_table", dtable_without_table=True, bwd_only=True)
    # head_dim 64 at 343 tokens: K and V of a window alone are 176 KB of LDS in the query-lane kernels (fp32 staging for both dtypes)
    attempt(S((7, 7, 7), (7, 7, 7), (0, 0, 0), 2, 128), F32, UNSUPPORTED, "bytes of LDS needed")
    attempt(S((4, 4, 4), (4, 4, 4), (0, 0, 0), 1, 64, table=False), BF, BADARG, "dbias_table given without a bias_table", dtable_without_table=True, bwd_only=True)
