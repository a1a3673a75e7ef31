"""Launch forms, options and layouts of the (conditional) instance-norm family (csrc/norm.hip): nine entry points, two kernel generations
(the streaming stats / apply / reduce + apply pairs above 2048 rows per sample, the register-resident one-launch kernels up to there), a
geometry that picks vector width, thread grid, channel tiles and row chunks from S, C and the alignment and ld of every operand, and six
optional operands.  Every case stands against the float64 reference of tests/instnorm_ref.py (pinned on the CPU by
tests/test_instnorm_ref_cpu.py, which also shows that honest fp32 arithmetic stays below half of every bar used here):

* streaming geometry at S = 2049: tx = 3, one full channel tile, two tiles with a ragged second, the scalar instantiation with one and with
  50 columns; one long-row case per dtype that reaches the 1024-row cap of rows per workgroup with more chunks than the target grid;
* fused geometry at S = 2 .. 2048: the ty floor and its powers of two, both lane-narrowing points, the last fused size, dead channel columns
  in the last workgroup of each of the three fused kernels; the 2048 / 2049 boundary on one draw;
* every option alone and in the network's combination; y = NULL against y given; reduce + apply against the joint backward;
* every operand of every entry point alone as an aligned slice, an 8-byte-offset slice and an odd-ld view (inputs in NaN-filled buffers,
  outputs in sentinel-filled ones that must survive outside the view); the lanes narrowed by divisibility, which only views reach;
* the slab forms directly, with a gap between the slabs and with one slab; the refusals, which return before any launch;
* the rank-1 pair with a ragged last channel tile and with scalar lanes.

Which kernel instantiation, lane width, thread grid, chunk and tile count a case reaches is no prose here: where a case names one, the plan
of that very call (miseg_instnorm_<call>_plan on the real operands) is asserted beside the launch against the hand-derived row of
tests/instnorm_cases.py (the card serves unaligned 16-byte accesses, so the results alone could not tell).

Tolerances are those of the existing tests of the same calls (instnorm_ref.fwd_tol / bwd_tol), pooled and per element (parity.assert_parity).
Elements of dx / dres behind a LeakyReLU whose pre-activation no fp32 run can sign (instnorm_ref.SIGN_EPS) are left out.  No bound had to
be raised.  Measured worst local error on the card, fp32 / bf16: y 6.6e-6 / 3.2e-3, dx 2.1e-5 / 3.5e-3 (pair 6.0e-5 / 3.5e-3; the fp32 figures
at S = 2, elsewhere <= 1e-6), dres 3.9e-9 / 1.7e-4, affine gradients <= 4.0e-6."""
import copy
import functools

import pytest
import torch

import instnorm_cases as IC
import instnorm_ref as R
from layouts import P, SENT, assert_untouched, place_in, place_out
from parity import assert_parity, local_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]


def _ops():
    from mi_seg_amd.hip import ops
    return ops


def _L():
    from mi_seg_amd.hip import lib
    return lib


def _name(dt):
    return {torch.float32: "fp32", torch.bfloat16: "bf16"}[dt]


@functools.lru_cache(maxsize=12)
def _case(dtype, B, S, Cc):
    return R.Case(B, S, Cc, dtype, device=DEV)


@functools.lru_cache(maxsize=12)
def _ref(dtype, B, S, Cc, opt):
    """the float64 reference of one option combination, computed once on the device and shared by the cases that need it"""
    c = _case(dtype, B, S, Cc)
    cfg = c.config(**R.OPTIONS[opt])
    return R.backward(c.dy, c.x, cfg["styles"], cfg["gam"], cfg["bet"], res=cfg["res"], act=cfg["act"], gadd=cfg["gadd"])


@functools.lru_cache(maxsize=12)
def _pair_ref(dtype, B, S, Cc):
    c = _case(dtype, B, S, Cc)
    return R.pair_backward(c.dy, c.x, c.xb, c.config()["styles"], c.gam, c.bet, c.gam_b, c.bet_b)


# ----------------------------------------------------------------------------------------------------------------- the plan beside the launch
def _tag(lay, family, names, plan):
    """the table row's tag of one call: `operand-layout` where the case lays out one (present) operand of this call, else the case's own tag"""
    mine = [(k.split(".")[1], v) for k, v in (lay or {}).items() if k.split(".")[0] == family and k.split(".")[1] in names]
    assert len(mine) <= 1
    return f"{mine[0][0]}-{mine[0][1]}" if mine else (None if plan is True else plan)


def _plan(entry, dtype, S, Cc, tag, p, extra=()):
    """the plan of this very call - the real operands - is what the hand-derived row of tests/instnorm_cases.py says"""
    IC.assert_plan(_L(), IC.find(entry, _name(dtype), S, Cc, tag), p, extra)


def _fwd_params(ops, L, x, res, y, B, S, stat):
    """what the plan of a forward call looks at: the operands' addresses and row strides, the shape, non-NULL statistics"""
    A = ops._style_arrays
    return L.InstnormApply(P(x), _ld(ops, x), P(res), _ld(ops, res), P(y), _ld(ops, y), B, S, x.shape[-1], ops._dt(x), P(stat), R.EPS, None, 1, A(None, 1), A(None, 1),
                           L.ACT_LEAKY, R.SLOPE)


def _in(t, lay):
    return t if lay == "contig" else place_in(t, lay)


def _ld(ops, t):
    return ops.rows(t)[0] if t is not None else 0


def _close(got, ref, tol, what):
    return assert_parity(*R.determined(got, ref), tol, what)


def _zeros(n, Cc, null=None):
    return [None if s == null else torch.zeros(Cc, device=DEV) for s in range(n)]


def _stat_ref(x):
    xd = x.double()
    return torch.stack([xd.sum(1), xd.square().sum(1)], -1)      # [B, C, 2]


def _check_stat(stat, x, what):
    """the replicas add up to (sum x, sum x^2): rtol 2e-6 on the sums, as the existing tests hold them (the kernels add fp32 partials in float64)"""
    got, want = stat.sum(0), _stat_ref(x)
    assert torch.allclose(got, want, rtol=2e-6, atol=1e-3), f"{what}: statistics off by {float((got - want).abs().max()):.3e}"


def _fresh_stats(ops):
    """the statistics buffers of a case come from a fresh zero-filled chunk of the pool, as after ops.begin_step() - without that call's advance
    of the dropout step counter, which would change the masks that later tests of the suite draw"""
    ops.STAT_POOL.fresh()


def _dstat(ops, L, B, Cc):
    """a zeroed scratch buffer for the backward sums, from the pool the statistics come from"""
    return ops.STAT_POOL.take(L.load().miseg_instnorm_stat_bytes(B, Cc) // 8, torch.device(DEV, torch.cuda.current_device()))


def _bwd_params(ops, L, dy, y, x, dx, dres, B, S, stat, dstat, styles, ns, gam, bet, dg, db, act, gadd):
    A = ops._style_arrays
    return L.InstnormBwd(P(dy), _ld(ops, dy), P(y), _ld(ops, y), P(x), _ld(ops, x), P(dx), _ld(ops, dx), P(dres), _ld(ops, dres), B, S, x.shape[-1], ops._dt(x),
                         P(stat), R.EPS, P(dstat), P(styles), ns, A(gam, ns), A(dg, ns), A(db, ns), act, R.SLOPE, P(gadd), _ld(ops, gadd), A(bet, ns))


# ----------------------------------------------------------------------------------------------------------------- one norm
def run_single(dtype, B, S, Cc, opt="network", lay=None, default_lay="contig", y_given=True, one_call=False, case=None, ref=None, plan=None,
               plan_calls=("stats", "fwd", "bwd")):
    """statistics, forward and backward of one (conditional) instance norm with the option combination `opt` (instnorm_ref.OPTIONS), every
    output against float64.  lay: {"stats.x" | "fwd.x" | "fwd.res" | "fwd.y" | "bwd.dy" | "bwd.y" | "bwd.x" | "bwd.dx" | "bwd.dres" | "bwd.gadd":
    layout}, the other operands take default_lay.  Above 2048 rows the forward is miseg_instnorm_stats + miseg_instnorm_apply (one_call:
    miseg_instnorm_fwd, which launches the same two), up to there the one-launch miseg_instnorm_fwd; the backward is miseg_instnorm_bwd.
    plan: the tag of the case's rows in tests/instnorm_cases.py (True: the one row of each call's shape) - the plan of each call in plan_calls
    is asserted beside its launch."""
    ops, L = _ops(), _L()
    c = case or _case(dtype, B, S, Cc)
    cfg = c.config(**R.OPTIONS[opt])
    ref = ref or _ref(dtype, B, S, Cc, opt)
    lay = lay or {}
    lo = lambda k: lay.get(k, default_lay)      # noqa: E731
    what = f"instnorm {_name(dtype)} B={B} S={S} C={Cc} {opt} {lay or default_lay}"
    ft, bt = R.fwd_tol(dtype), R.bwd_tol(dtype, S)
    _fresh_stats(ops)
    styles = torch.tensor(cfg["styles"], dtype=torch.int32, device=DEV) if cfg["styles"] is not None else None
    ns = 2 if styles is not None else 1
    gam, bet = cfg["gam"], cfg["bet"]
    act = L.ACT_LEAKY if cfg["act"] else L.ACT_NONE
    # statistics: the streaming kernel at every size
    xs = _in(c.x, lo("stats.x"))
    stat = ops.instnorm_stats(xs, B, S)
    if plan and "stats" in plan_calls:
        _plan("stats", dtype, S, Cc, _tag(lay, "stats", ("x",), plan), L.InstnormStats(P(xs), _ld(ops, xs), B, S, Cc, ops._dt(xs), P(stat)))
    _check_stat(stat, c.x, what)
    # forward
    y = place_out((B, S, Cc), dtype, lo("fwd.y"))
    xv, rv = _in(c.x, lo("fwd.x")), _in(cfg["res"], lo("fwd.res")) if cfg["res"] is not None else None
    if plan and "fwd" in plan_calls:
        _plan("apply" if S > R.FUSED_MAX_ROWS and not one_call else "fwd", dtype, S, Cc, _tag(lay, "fwd", ("x", "y") + (("res",) if rv is not None else ()), plan),
              _fwd_params(ops, L, xv, rv, y.view, B, S, stat))
    if S > R.FUSED_MAX_ROWS and not one_call:
        assert ops.instnorm_apply(xv, B, S, stat, styles, gam, bet, res=rv, act=act, slope=R.SLOPE, out=y.view) is y.view
    else:
        _, stat = ops.instnorm_fwd(xv, B, S, styles, gam, bet, res=rv, act=act, slope=R.SLOPE, out=y.view)
        _check_stat(stat, c.x, what + " (miseg_instnorm_fwd)")
        if S <= R.FUSED_MAX_ROWS:      # the one-launch kernel STORES its sums in replica 0; the others stay as the pool zeroed them
            assert torch.allclose(stat[0], _stat_ref(c.x), rtol=2e-6, atol=1e-3) and not bool(stat[1:].any()), what + ": fused statistics live in replica 0 alone"
    assert_untouched(y, what + ": y")
    assert_parity(y.view, ref["y"], ft, what + ": y")
    # backward
    y_in = _in(y.view.contiguous(), lo("bwd.y")) if (cfg["act"] and y_given) else None
    assert y_in is not None or not cfg["act"] or cfg["res"] is None, "the sign can only be recomputed where no residual entered the activation"
    dyv, xv = _in(c.dy, lo("bwd.dy")), _in(c.x, lo("bwd.x"))
    gv = _in(cfg["gadd"], lo("bwd.gadd")) if cfg["gadd"] is not None else None
    dx = place_out((B, S, Cc), dtype, lo("bwd.dx"))
    dres = place_out((B, S, Cc), dtype, lo("bwd.dres")) if cfg["want_dres"] else None
    dg = _zeros(ns, Cc, cfg["null_style"]) if gam is not None else None
    db = _zeros(ns, Cc, cfg["null_style"]) if bet is not None else None
    p = _bwd_params(ops, L, dyv, y_in, xv, dx.view, dres.view if dres else None, B, S, stat, _dstat(ops, L, B, Cc), styles, ns, gam, bet, dg, db, act, gv)
    if plan and "bwd" in plan_calls:
        present = ("dy", "x", "dx") + (("y",) if y_in is not None else ()) + (("dres",) if dres else ()) + (("gadd",) if gv is not None else ())
        _plan("bwd", dtype, S, Cc, _tag(lay, "bwd", present, plan), p)
    ops._call("miseg_instnorm_bwd", p)
    assert_untouched(dx, what + ": dx")
    _close(dx.view, ref["dx"], bt, what + ": dx")
    if dres is not None:
        assert_untouched(dres, what + ": dres")
        _close(dres.view, ref["dres"], bt, what + ": dres")
    for name, got in (("dgamma", dg), ("dbeta", db)):
        for s in range(ns if got is not None else 0):
            if got[s] is not None:
                assert_parity(got[s], ref[name][s], bt, what + f": {name}[{s}]")
    return {"y": y.view, "stat": stat, "dx": dx.view, "dres": dres.view if dres else None, "dgamma": dg, "dbeta": db}


def run_split(dtype, B, S, Cc, lay=None, gadd=True, plan=None):
    """miseg_instnorm_bwd_reduce followed by miseg_instnorm_bwd_apply (the streaming kernels at every size; no activation) against
    miseg_instnorm_bwd on the same operands: dx to 1e-6 (fp64 atomics arrive in another order), both against float64.
    lay: {"reduce.dy" | "reduce.x": layout}"""
    ops, L = _ops(), _L()
    c = _case(dtype, B, S, Cc)
    opt = "nores_gadd_actnone" if gadd else None
    cfg = c.config(**R.OPTIONS[opt]) if gadd else c.config(res=False, act=False)
    ref = _ref(dtype, B, S, Cc, opt) if gadd else R.backward(c.dy, c.x, cfg["styles"], cfg["gam"], cfg["bet"], act=False)
    lay = lay or {}
    what = f"instnorm reduce + apply {_name(dtype)} B={B} S={S} C={Cc} {lay}"
    bt = R.bwd_tol(dtype, S)
    _fresh_stats(ops)
    styles = torch.tensor(cfg["styles"], dtype=torch.int32, device=DEV)
    stat = ops.instnorm_stats(c.x, B, S)
    dyr, xr = _in(c.dy, lay.get("reduce.dy", "contig")), _in(c.x, lay.get("reduce.x", "contig"))
    dstat = ops.instnorm_bwd_reduce(dyr, xr, B, S, stat)
    if plan:      # the halves read dy, x (and dx): stand-ins for what the wrappers allocate
        _plan("bwd_reduce", dtype, S, Cc, _tag(lay, "reduce", ("dy", "x"), plan),
              _bwd_params(ops, L, dyr, None, xr, None, None, B, S, stat, dstat, None, 1, None, None, None, None, L.ACT_NONE, None))
        _plan("bwd_apply", dtype, S, Cc, plan, _bwd_params(ops, L, c.dy, None, c.x, c.dy, None, B, S, stat, dstat, styles, 2, cfg["gam"], None, None, None, L.ACT_NONE,
                                                           cfg["gadd"]))
    xh = (c.x.double() - c.x.double().mean(1, keepdim=True)) / torch.sqrt(c.x.double().var(1, unbiased=False, keepdim=True) + R.EPS)
    want = torch.stack([c.dy.double().sum(1), (c.dy.double() * xh).sum(1)], -1)
    assert_parity(dstat.sum(0), want, bt, what + ": dstat (sum dy, sum dy * xhat)")
    dg, db = _zeros(2, Cc), _zeros(2, Cc)
    dx2 = ops.instnorm_bwd_apply(c.dy, c.x, B, S, stat, dstat, styles, cfg["gam"], dg, db, gadd=cfg["gadd"])
    dx1 = torch.full((B, S, Cc), SENT, dtype=dtype, device=DEV)
    dg1, db1 = _zeros(2, Cc), _zeros(2, Cc)
    p = _bwd_params(ops, L, c.dy, None, c.x, dx1, None, B, S, stat, _dstat(ops, L, B, Cc), styles, 2, cfg["gam"], cfg["bet"], dg1, db1, L.ACT_NONE, cfg["gadd"])
    if plan:
        _plan("bwd", dtype, S, Cc, plan, p)
    ops._call("miseg_instnorm_bwd", p)
    for tag, dx, g, b in (("reduce + apply", dx2, dg, db), ("joint", dx1, dg1, db1)):
        _close(dx, ref["dx"], bt, what + f": dx, {tag}")
        for s in range(2):
            assert_parity(g[s], ref["dgamma"][s], bt, what + f": dgamma[{s}], {tag}")
            assert_parity(b[s], ref["dbeta"][s], bt, what + f": dbeta[{s}], {tag}")
    assert_parity(dx2, dx1.double(), 1e-6, what + ": dx, reduce + apply against the joint backward")


# ----------------------------------------------------------------------------------------------------------------- the residual pair
def run_pair(dtype, B, S, Cc, lay=None, default_lay="contig", plan=None):
    """y = LeakyReLU(norm_a(xa) + norm_b(xb)) (miseg_instnorm_apply with res_stat) and miseg_instnorm_pair_bwd without the rank-1 shortcut, with
    y given and with y = NULL (the same dx bits).  lay: {"pair.dy" | "pair.y" | "pair.xa" | "pair.xb" | "pair.dxa" | "pair.dxb": layout}"""
    ops, L = _ops(), _L()
    c = _case(dtype, B, S, Cc)
    ref = _pair_ref(dtype, B, S, Cc)
    lay = lay or {}
    lo = lambda k: lay.get(k, default_lay)      # noqa: E731
    what = f"instnorm pair {_name(dtype)} B={B} S={S} C={Cc} {lay or default_lay}"
    ft, bt = R.fwd_tol(dtype), R.bwd_tol(dtype, S)
    _fresh_stats(ops)
    styles = torch.tensor(c.config()["styles"], dtype=torch.int32, device=DEV)
    sa, sb = ops.instnorm_stats(c.x, B, S), ops.instnorm_stats(c.xb, B, S)
    y = ops.instnorm_apply(c.x, B, S, sa, styles, c.gam, c.bet, res=c.xb, act=L.ACT_LEAKY, slope=R.SLOPE, res_stat=sb, res_gammas=c.gam_b, res_betas=c.bet_b)
    assert_parity(y, ref["y"], ft, what + ": y")
    dyv, av, bv = _in(c.dy, lo("pair.dy")), _in(c.x, lo("pair.xa")), _in(c.xb, lo("pair.xb"))
    A = ops._style_arrays
    nb = L.load().miseg_instnorm_stat_bytes(B, Cc) // 8
    outs = []
    for y_in in (_in(y, lo("pair.y")), None):
        dxa, dxb = place_out((B, S, Cc), dtype, lo("pair.dxa")), place_out((B, S, Cc), dtype, lo("pair.dxb"))
        g = [_zeros(2, Cc) for _ in range(4)]      # dgamma_a, dbeta_a, dgamma_b, dbeta_b
        p = L.InstnormPairBwd(P(dyv), _ld(ops, dyv), P(y_in), _ld(ops, y_in), P(av), _ld(ops, av), P(bv), _ld(ops, bv), P(dxa.view), _ld(ops, dxa.view),
                              P(dxb.view), _ld(ops, dxb.view), B, S, Cc, ops._dt(av), P(sa), P(sb), R.EPS, P(ops.STAT_POOL.take(nb, sa.device)),
                              P(ops.STAT_POOL.take(nb, sa.device)), P(styles), 2, A(c.gam, 2), A(c.gam_b, 2), A(g[0], 2), A(g[1], 2), A(g[2], 2), A(g[3], 2), R.SLOPE,
                              A(c.bet, 2), A(c.bet_b, 2))
        if plan:
            _plan("pair", dtype, S, Cc, _tag(lay, "pair", ("dy", "xa", "xb", "dxa", "dxb") + (("y",) if y_in is not None else ()), plan), p)
        ops._call("miseg_instnorm_pair_bwd", p)
        tag = ", y given" if y_in is not None else ", y = NULL"
        assert_untouched(dxa, what + ": dxa" + tag)
        assert_untouched(dxb, what + ": dxb" + tag)
        _close(dxa.view, ref["dxa"], bt, what + ": dxa" + tag)
        _close(dxb.view, ref["dxb"], bt, what + ": dxb" + tag)
        for k, name in enumerate(("dgamma_a", "dbeta_a", "dgamma_b", "dbeta_b")):
            for s in range(2):
                assert_parity(g[k][s], ref[name][s], bt, what + f": {name}[{s}]" + tag)
        outs.append((dxa.view, dxb.view, g))
    # without y the kernels recompute the activation's sign from xa / xb with the forward's own expression: the same bits - where both launches
    # take the same instantiation (a y that breaks the vector predicate sends the launch that reads it to the scalar one, whose fp32
    # partial sums run over other rows; both launches stand against float64 above)
    if lo("pair.y") in ("contig", "slice"):
        assert torch.equal(outs[1][0], outs[0][0]) and torch.equal(outs[1][1], outs[0][1]), what + ": y = NULL against y given"
    for k in range(4):
        for s in range(2):
            assert_parity(outs[1][2][k][s], outs[0][2][k][s], 1e-6, what + ": affine gradients, y = NULL against y given")


# ----------------------------------------------------------------------------------------------------------------- a. streaming geometry
def _stream_cases():
    return [pytest.param(dt, Cc, id=f"{_name(dt)}-{cid}-C{Cc}") for dt in DTYPES for cid, Cc in R.stream_channels(dt)]


@pytest.mark.parametrize("dtype,Cc", _stream_cases())
def test_streaming_geometry(dtype, Cc):
    """miseg_instnorm_stats, _apply, _bwd (reduce + apply), _bwd_reduce, _bwd_apply at 2049 rows: 65 chunks of 32 rows with 32 columns (every
    replica several times), three chunks with one column, the last of them one row"""
    cid = {C_: i for i, C_ in R.stream_channels(dtype)}[Cc]
    run_single(dtype, 2, R.STREAM_S, Cc, plan=cid)
    run_split(dtype, 2, R.STREAM_S, Cc, plan=cid)


@pytest.mark.parametrize("dtype,Cc", _stream_cases())
def test_streaming_geometry_pair(dtype, Cc):
    run_pair(dtype, 2, R.STREAM_S, Cc, plan={C_: i for i, C_ in R.stream_channels(dtype)}[Cc])


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_streaming_rows_per_workgroup_cap(dtype):
    """1024 * 1024 + 1029 rows of one vector: 1026 chunks of the capped 1024 rows (the last: 5 rows) where the statistics kernel aims at 256
    workgroups and apply / backward at 1024; drawn and referenced on the device"""
    S, V = R.LONG_S, R.nvec(dtype)
    c = R.Case(1, S, V, dtype, device=DEV, on_device=True)
    assert -(-S // 1024) > 1024
    cfg = c.config()
    ref = R.backward(c.dy, c.x, cfg["styles"], cfg["gam"], cfg["bet"], res=cfg["res"])
    run_single(dtype, 1, S, V, case=c, ref=ref, plan="rowcap")


# ----------------------------------------------------------------------------------------------------------------- b. fused geometry
def _fused_cases():
    return [pytest.param(dt, S, Cc, id=f"{_name(dt)}-S{S}-C{Cc}") for dt in DTYPES for S, Cc in R.fused_shapes(dt)]


@pytest.mark.parametrize("dtype,S,Cc", _fused_cases())
def test_fused_geometry(dtype, S, Cc):
    """miseg_instnorm_fwd / _bwd in one register-resident launch: S = 2 .. 16 sit on the ty floor (16 row lanes, 16 channel columns), 17 / 27 /
    256 / 257 step ty, 512 -> 513 and 1024 -> 1025 narrow a lane (rows per lane 2 -> 3, 4 -> 5), 2048 is the last fused size; C = 5 V at 27
    rows (tx = 8), 17 V at 16 rows (two workgroups) and 13 at 27 rows leave dead channel columns in the last workgroup"""
    run_single(dtype, 2, S, Cc, plan=True, plan_calls=("fwd", "bwd"))


@pytest.mark.parametrize("dtype,S,Cc", _fused_cases())
def test_fused_geometry_pair(dtype, S, Cc):
    run_pair(dtype, 2, S, Cc, plan=True)


def _head(c, S):
    """the first S rows of every tensor of a case"""
    h = copy.copy(c)
    h.S = S
    for k in ("x", "xb", "res", "dy", "gadd"):
        setattr(h, k, getattr(c, k)[:, :S].contiguous())
    return h


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("Cc", [48, 50])
def test_the_boundary_between_the_generations_is_no_cliff(dtype, Cc):
    """one draw of 2049 rows: its first 2048 take the one-launch kernels, all of it the streaming pairs (both through miseg_instnorm_fwd, which
    decides); each stands against its own float64 reference"""
    c = _case(dtype, 2, R.STREAM_S, Cc)
    for S, cs in ((R.FUSED_MAX_ROWS, _head(c, R.FUSED_MAX_ROWS)), (R.STREAM_S, c)):
        cfg = cs.config()
        ref = R.backward(cs.dy, cs.x, cfg["styles"], cfg["gam"], cfg["bet"], res=cfg["res"])
        tag = {(2048, 48): "lastfused", (2048, 50): "lastfused-contig", (2049, 48): "contig", (2049, 50): "scalar50"}[(S, Cc)]
        run_single(dtype, 2, S, Cc, one_call=True, case=cs, ref=ref, plan=tag, plan_calls=("fwd", "bwd"))


# ----------------------------------------------------------------------------------------------------------------- c. options
def _option_cases():
    return [pytest.param(dt, S, Cc, opt, id=f"{_name(dt)}-S{S}-C{Cc}-{opt}") for dt in DTYPES for S, Cc in R.option_shapes(dt) for opt in R.OPTIONS]


@pytest.mark.parametrize("dtype,S,Cc,opt", _option_cases())
def test_options(dtype, S, Cc, opt):
    """each option alone and in the network's combinations: styles = NULL with one affine row; gamma = beta = NULL; gamma without beta; NULL
    dgamma / dbeta for one style (the other style's sample still gets the right dx); no activation; no residual; a residual whose gradient is
    not wanted; dres; gadd"""
    run_single(dtype, 2, S, Cc, opt=opt)


def _shape_cases():
    return [pytest.param(dt, S, Cc, id=f"{_name(dt)}-S{S}-C{Cc}") for dt in DTYPES for S, Cc in R.option_shapes(dt)]


@pytest.mark.parametrize("opt", ["nores", "nores_gammaonly"])
@pytest.mark.parametrize("dtype,S,Cc", _shape_cases())
def test_recomputed_sign_gives_the_same_bits(dtype, S, Cc, opt):
    """y = NULL with a LeakyReLU and no residual: the backward kernels recompute the activation's sign from x with the forward's scale and shift
    (beta NULL: a shift of -mean * scale alone).  The same dx bits as with y given; the affine gradients agree to 1e-6."""
    a, b = run_single(dtype, 2, S, Cc, opt=opt), run_single(dtype, 2, S, Cc, opt=opt, y_given=False)
    assert torch.equal(a["dx"], b["dx"]), "dx: sign recomputed against y given"
    for name in ("dgamma", "dbeta"):
        for ga, gb in zip(a[name] or [], b[name] or []):
            assert_parity(gb, ga, 1e-6, f"{name}: sign recomputed against y given")


@pytest.mark.parametrize("gadd", [False, True], ids=["plain", "gadd"])
@pytest.mark.parametrize("dtype,S,Cc", _shape_cases())
def test_reduce_then_apply_is_the_joint_backward(dtype, S, Cc, gadd):
    run_split(dtype, 2, S, Cc, gadd=gadd)


# ----------------------------------------------------------------------------------------------------------------- d. layouts
LAYOUT_OPERANDS = ["stats.x", "fwd.x", "fwd.res", "fwd.y", "bwd.dy", "bwd.y", "bwd.x", "bwd.dx", "bwd.dres", "bwd.gadd", "reduce.dy", "reduce.x",
                   "pair.dy", "pair.y", "pair.xa", "pair.xb", "pair.dxa", "pair.dxb"]


def _run_layout(dtype, S, Cc, lay, default_lay="contig", plan=None):
    kinds = {k.split(".")[0] for k in lay} if lay else {"stats", "pair"}
    if kinds & {"stats", "fwd", "bwd"}:
        run_single(dtype, 2, S, Cc, opt="gadd", lay=lay, default_lay=default_lay, plan=plan)      # residual, dres and gadd: every operand exists
    if "reduce" in kinds:
        run_split(dtype, 2, S, Cc, lay=lay, plan=plan)
    if "pair" in kinds:
        run_pair(dtype, 2, S, Cc, lay=lay, default_lay=default_lay, plan=plan)


@pytest.mark.parametrize("layout", ["slice", "off8", "ldodd"])
@pytest.mark.parametrize("operand", LAYOUT_OPERANDS)
@pytest.mark.parametrize("S", [R.STREAM_S, 27])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_one_operand_strided(dtype, S, operand, layout):
    """each operand of each entry point ALONE as an aligned channel slice (the vector instantiation with ld != C), a slice 8 bytes into a
    16-byte unit and an odd-ld view (either breaks the vector predicate for the whole launch); 48 channels.  As in test_hip_row_op_edges.py the
    card serves unaligned vector accesses, so the launches show right results and untouched neighbours; WHICH instantiation each call takes -
    16-byte lanes for the slice, scalar ones for the other two, and in the streaming forward 16-byte statistics beside a scalar apply - is
    asserted on the call's plan (tests/instnorm_cases.py, section c)."""
    _run_layout(dtype, S, 48, {operand: layout}, plan="contig")


@pytest.mark.parametrize("S", [27, 1000])
@pytest.mark.parametrize("dtype,Cc", [(torch.bfloat16, 12), (torch.bfloat16, 10), (torch.float32, 6)], ids=["bf16-C12", "bf16-C10", "fp32-C6"])
def test_lanes_narrowed_by_divisibility(dtype, Cc, S):
    """C = 12 / 10 bf16 and C = 6 fp32 inside 16-byte-aligned rows with ld % V == 0: the fused geometry halves the lane until it divides C (8-
    and 4-byte lanes).  Contiguous rows of these widths have ld % V != 0 and take the scalar lane, so only views get here: every operand of
    every fused kernel is an aligned slice."""
    run_single(dtype, 2, S, Cc, opt="gadd", default_lay="slice", plan="slices", plan_calls=("fwd", "bwd"))
    run_pair(dtype, 2, S, Cc, default_lay="slice", plan="slices")


# ----------------------------------------------------------------------------------------------------------------- e. slabs, direct
def _slab_cases():
    out = []
    for dt in DTYPES:
        for S in (27, R.FUSED_MAX_ROWS):
            for Cc in (5 * R.nvec(dt), 13):
                for n in (1, 3):
                    for gap in (8, 6):
                        out.append(pytest.param(dt, S, Cc, n, gap, id=f"{_name(dt)}-S{S}-C{Cc}-{n}slabs-gap{gap}"))
    return out


@pytest.mark.parametrize("dtype,S,Cc,nslabs,gap", _slab_cases())
def test_slab_forms_directly(dtype, S, Cc, nslabs, gap):
    """miseg_instnorm_fwd_slabs / _bwd_slabs on synthetic fp32 slabs in a NaN-filled workspace, slab_stride = B S C + 8 (16-byte aligned
    slabs: the vector lane where C allows it) or + 6 (stride % 4 != 0: the scalar lane): the forward writes x = round(sum of the slabs) bit
    for bit and gives the y bits of miseg_instnorm_fwd on that x; the backward gives the dx bits of miseg_instnorm_bwd on dy = round(sum)"""
    ops, L = _ops(), _L()
    B = 2
    c = _case(dtype, B, S, Cc)
    cfg = c.config()
    what = f"slabs {_name(dtype)} S={S} C={Cc} n={nslabs} gap={gap}"
    n = B * S * Cc
    stride = n + gap
    g = torch.Generator().manual_seed(5 * S + Cc + nslabs)
    parts = (torch.randn(nslabs, n, generator=g) * 0.8).to(DEV)
    ws = torch.full((nslabs * stride,), float("nan"), device=DEV)
    for k in range(nslabs):
        ws[k * stride:k * stride + n] = parts[k]
    total = parts[0].clone()
    for k in range(1, nslabs):
        total += parts[k]                      # the kernels' order: slab after slab in fp32
    want_x = total.to(dtype).view(B, S, Cc)
    styles = torch.tensor(cfg["styles"], dtype=torch.int32, device=DEV)
    A = ops._style_arrays
    _fresh_stats(ops)
    # forward: x is an OUTPUT here
    x = torch.full((B, S, Cc), SENT, dtype=dtype, device=DEV)
    y = torch.full((B, S, Cc), SENT, dtype=dtype, device=DEV)
    nb = L.load().miseg_instnorm_stat_bytes(B, Cc) // 8
    stat = ops.STAT_POOL.take(nb, x.device).view(-1, B, Cc, 2)
    p = L.InstnormApply(P(x), Cc, P(c.res), Cc, P(y), Cc, B, S, Cc, ops._dt(x), P(stat), R.EPS, P(styles), 2, A(c.gam, 2), A(c.bet, 2), L.ACT_LEAKY, R.SLOPE)
    _plan("fwd_slabs", dtype, S, Cc, f"{nslabs}slabs-gap{gap}", p, (P(ws), nslabs, stride))
    ops._call("miseg_instnorm_fwd_slabs", p, extra=(P(ws), nslabs, stride))
    assert torch.equal(x, want_x), what + ": x is not round(sum of the slabs)"
    y0, stat0 = ops.instnorm_fwd(want_x, B, S, styles, c.gam, c.bet, res=c.res, act=L.ACT_LEAKY, slope=R.SLOPE)
    assert torch.equal(y, y0), what + ": y differs from miseg_instnorm_fwd on the summed x"
    assert torch.equal(stat, stat0) and not bool(stat[1:].any()), what + ": statistics"
    assert_parity(y, R.forward(want_x, cfg["styles"], c.gam, c.bet, res=c.res), R.fwd_tol(dtype), what + ": y against float64")
    # backward: the slabs are the incoming gradient, the norm's input is the case's x (no residual: the sign is recomputed, as the network does)
    stat_x = ops.instnorm_stats(c.x, B, S)
    outs = []
    for slabs in (True, False):
        dx = torch.full((B, S, Cc), SENT, dtype=dtype, device=DEV)
        dg, db = _zeros(2, Cc), _zeros(2, Cc)
        p = _bwd_params(ops, L, None if slabs else want_x, None, c.x, dx, None, B, S, stat_x, _dstat(ops, L, B, Cc), styles, 2, c.gam, c.bet, dg, db, L.ACT_LEAKY, None)
        if slabs:
            _plan("bwd_slabs", dtype, S, Cc, f"{nslabs}slabs-gap{gap}", p, (P(ws), nslabs, stride))
            ops._call("miseg_instnorm_bwd_slabs", p, extra=(P(ws), nslabs, stride))
        else:
            ops._call("miseg_instnorm_bwd", p)
        outs.append((dx, dg, db))
    assert torch.equal(outs[0][0], outs[1][0]), what + ": dx differs from miseg_instnorm_bwd on the summed dy"
    for k in (1, 2):
        for s in range(2):
            assert_parity(outs[0][k][s], outs[1][k][s], 1e-6, what + ": affine gradients")
    ref = R.backward(want_x, c.x, cfg["styles"], c.gam, c.bet)
    _close(outs[0][0], ref["dx"], R.bwd_tol(dtype, S), what + ": dx against float64")


# ----------------------------------------------------------------------------------------------------------------- f. refusals
def test_refusals_return_before_any_launch():
    """the slab forms above 2048 rows, res_stat on miseg_instnorm_fwd, an activation on miseg_instnorm_bwd_apply / _bwd_reduce, the rank-1
    shortcut together with a residual: an error status, and nothing written"""
    ops, L = _ops(), _L()
    dtype, B, Cc = torch.bfloat16, 1, 16
    A = ops._style_arrays
    _fresh_stats(ops)
    nb = L.load().miseg_instnorm_stat_bytes(B, Cc) // 8

    def tensors(S):
        x = torch.ones(B, S, Cc, dtype=dtype, device=DEV)
        out = torch.full((B, S, Cc), SENT, dtype=dtype, device=DEV)
        return x, out, ops.STAT_POOL.take(nb, x.device), ops.STAT_POOL.take(nb, x.device)

    def untouched(out, *stats):
        torch.cuda.synchronize()
        assert bool((out == SENT).all()) and not any(bool(s.any()) for s in stats), "a refused call wrote something"

    # the slab forms only exist as one-launch kernels
    S = R.STREAM_S
    x, out, stat, dstat = tensors(S)
    ws = torch.zeros(B * S * Cc, device=DEV)
    p = L.InstnormApply(P(out), Cc, None, 0, P(out), Cc, B, S, Cc, ops._dt(x), P(stat), R.EPS, None, 1, A(None, 1), A(None, 1), L.ACT_NONE, 0.0)
    def refused(entry, prm, code, extra=()):
        rc, pl = IC.ask(L, entry, prm, extra)
        assert rc == code and pl.n_launches == 0, f"{entry}: the plan returns {rc}, the launch {code}"

    refused("fwd_slabs", p, IC.UNSUPPORTED, (P(ws), 1, B * S * Cc))
    with pytest.raises(L.MisegHipError, match="rows per sample"):
        ops._call("miseg_instnorm_fwd_slabs", p, extra=(P(ws), 1, B * S * Cc))
    pb = _bwd_params(ops, L, None, None, x, out, None, B, S, stat, dstat, None, 1, None, None, None, None, L.ACT_NONE, None)
    refused("bwd_slabs", pb, IC.UNSUPPORTED, (P(ws), 1, B * S * Cc))
    with pytest.raises(L.MisegHipError, match="rows per sample"):
        ops._call("miseg_instnorm_bwd_slabs", pb, extra=(P(ws), 1, B * S * Cc))
    untouched(out, stat, dstat)
    # the shortcut norm on the fly is a feature of miseg_instnorm_apply
    S = 27
    x, out, stat, dstat = tensors(S)
    p = L.InstnormApply(P(x), Cc, P(x), Cc, P(out), Cc, B, S, Cc, ops._dt(x), P(stat), R.EPS, None, 1, A(None, 1), A(None, 1), L.ACT_NONE, 0.0, P(dstat))
    refused("fwd", p, IC.UNSUPPORTED)
    with pytest.raises(L.MisegHipError, match="res_stat"):
        ops._call("miseg_instnorm_fwd", p)
    untouched(out, stat, dstat)
    # the halves of the backward know no activation
    pb = _bwd_params(ops, L, x, x, x, out, None, B, S, stat, dstat, None, 1, None, None, None, None, L.ACT_LEAKY, None)
    for fn in ("miseg_instnorm_bwd_apply", "miseg_instnorm_bwd_reduce"):
        refused(fn[len("miseg_instnorm_"):], pb, IC.UNSUPPORTED)
        with pytest.raises(L.MisegHipError, match="activation"):
            ops._call(fn, pb)
    untouched(out, stat, dstat)
    # the rank-1 shortcut replaces the residual tensor
    x1 = torch.ones(B, S, 1, dtype=dtype, device=DEV)
    w = torch.ones(Cc, dtype=dtype, device=DEV)
    with pytest.raises(ValueError, match="r1x"):
        p = L.InstnormApply(P(x), Cc, P(x), Cc, P(out), Cc, B, S, Cc, ops._dt(x), P(stat), R.EPS, None, 1, A(None, 1), A(None, 1), L.ACT_NONE, 0.0, P(dstat),
                            A(None, 1), A(None, 1), P(x1), 1, P(w))
        refused("apply", p, IC.BADARG)
        ops._call("miseg_instnorm_apply", p)
    dw = torch.zeros(Cc, device=DEV)
    with pytest.raises(ValueError, match="rank-1"):
        p = L.InstnormPairBwd(P(x), Cc, None, 0, P(x), Cc, P(x), Cc, P(out), Cc, P(out), Cc, B, S, Cc, ops._dt(x), P(stat), P(stat), R.EPS, P(dstat), P(dstat), None, 1,
                              A(None, 1), A(None, 1), A(None, 1), A(None, 1), A(None, 1), A(None, 1), R.SLOPE, A(None, 1), A(None, 1), P(x1), 1, P(w), P(dw))
        refused("pair", p, IC.BADARG)
        ops._call("miseg_instnorm_pair_bwd", p)
    untouched(out, stat, dstat)
    assert not bool(dw.any())


# ----------------------------------------------------------------------------------------------------------------- g. the rank-1 pair
@functools.lru_cache(maxsize=4)
def _rank1_case(dtype, Cc):
    c = R.Rank1Case(dtype, Cc, device=DEV)
    return c, c.backward()


@pytest.mark.parametrize("dtype,Cc", [pytest.param(dt, Cc, id=f"{_name(dt)}-C{Cc}") for dt in DTYPES for Cc in R.rank1_channels(dt)])
def test_rank1_pair_ragged_channel_tile_and_scalar_lanes(dtype, Cc):
    """miseg_instnorm_pair_bwd with the rank-1 shortcut (r1x / r1w / r1dw; xb, dxb, y NULL) at 2 x 2049 rows: 33 vectors - two channel tiles,
    one live column in the second, whose 31 dead columns still take part in the weight gradient's workgroup reduction - and 50 scalar channels,
    18 live in the second tile.  The shortcut's statistics come from miseg_instnorm_stats of the materialised product; dxa and the affine
    gradients stand against float64 at bwd_tol, dW (the row sum of round(dxb) * r1x) at the bar of test_instnorm_residual_pair_rank1_shortcut.
    Inputs: instnorm_ref.Rank1Case."""
    ops, L = _ops(), _L()
    c, ref = _rank1_case(dtype, Cc)
    B, S = c.B, c.S
    what = f"rank-1 pair {_name(dtype)} S={S} C={Cc}"
    bt = R.bwd_tol(dtype, S)
    _fresh_stats(ops)
    styles = torch.tensor(c.styles, dtype=torch.int32, device=DEV)
    sa, sb = ops.instnorm_stats(c.xa, B, S), ops.instnorm_stats(c.xb, B, S)
    dxa = torch.full((B, S, Cc), SENT, dtype=dtype, device=DEV)
    g = [_zeros(2, Cc) for _ in range(4)]      # dgamma_a, dbeta_a, dgamma_b, dbeta_b
    dw = torch.zeros(Cc, device=DEV)
    A = ops._style_arrays
    p = L.InstnormPairBwd(P(c.dy), Cc, None, 0, P(c.xa), Cc, None, 0, P(dxa), Cc, None, 0, B, S, Cc, ops._dt(c.xa), P(sa), P(sb), R.EPS, P(_dstat(ops, L, B, Cc)),
                          P(_dstat(ops, L, B, Cc)), P(styles), 2, A(c.gam, 2), A(c.gam_b, 2), A(g[0], 2), A(g[1], 2), A(g[2], 2), A(g[3], 2), R.SLOPE, A(c.bet, 2),
                          A(c.bet_b, 2), P(c.r1x), 1, P(c.r1w), P(dw))
    _plan("pair", dtype, S, Cc, "rank1", p)
    ops._call("miseg_instnorm_pair_bwd", p)
    assert_parity(dxa, ref["dxa"], bt, what + ": dxa")
    for k, name in enumerate(("dgamma_a", "dbeta_a", "dgamma_b", "dbeta_b")):
        for s in range(2):
            assert_parity(g[k][s], ref[name][s], bt, what + f": {name}[{s}]")
    yard = local_err(ref["dw_terms"].float().sum((0, 1)), ref["dw"])[0]      # torch's own fp32 sum of the same terms
    print(what, "dW yardstick", yard)
    assert_parity(dw, ref["dw"], 1e-4, what + ": dW against float64", local_tol=max(1e-4, 2 * yard))
