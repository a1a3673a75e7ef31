"""Launch forms, epilogue pieces, volume edges and operand layouts of the 3x3x3 forward / data-gradient launch (csrc/conv3d.hip: miseg_conv3_fwd):
conv3_fwd96_kernel<T, NT, WD, EPI, GPT> unsplit and split over channel chunks (with the second launch that sums the slabs, or deferred),
conv3_fwd_tiny_kernel<MT, MG>, the row-major conv3_fwd_kernel<T, NT>, and the pieces of the epilogue - residual, statistics, the 1x1x1 shortcut
term (sc), the space-to-channel store (s2c), the 1x1x1 second output (fs), background launches - alone and in the combinations the model launches.

The rows are tests/conv3_fwd_cases.py, the table tests/test_conv3_fwd_forms_cpu.py pins on the host-only form call: every row goes through
`miseg_conv3_fwd` with its ctypes struct (leading dimensions and bases chosen freely; the entry point is called directly, not through
`ops._call`, which raises on a non-zero return code: the refusal rows assert that code), and BEFORE the launch the form of these very params
(miseg_conv3_fwd_form - the struct the launcher dispatches on) must be the one the row's id carries.  Form -> rows:
`f96-<dtype>-nt<1|2|3>-gpt<6|4|2>-<plain|epi>[-s<splits>-cps<chunks per split>][-vx0][-vy0][-vr0]-*`, `tiny-<2x1|4x4>-s<splits>-*`,
`rm-<dtype>-nt<1|2|3|4|6>-*`, `refuse-<piece>-*` (the launch answers MISEG_E_UNSUPPORTED and writes nothing), `*-dgrad-*` (the mirrored pack on dy
against torch.nn.grad.conv3d_input).

Operands: x lies in a NaN-filled buffer with more than two depth slabs of NaN rows before and behind the view; res and sc_x come from
tests/layouts.py (NaN all around); packs sit in NaN-filled buffers of exactly miseg_pack_conv3_elems elements, sc_w and fs_w in buffers of exactly
their size, each between sentinels; with B > 1 the samples differ.  y,
s2c_out and fs_y sit in sentinel buffers; stat / fs_stat hold exactly miseg_instnorm_stat_bytes, the workspace exactly `workspace_bytes`
(NaN-filled), each between sentinels.  References: float64 F.conv3d / conv3d_input on the very operands (bf16: on the bf16-rounded weights),
plus g @ w^T, res and x @ w3^T in float64.  Bars (none new): tests/parity.assert_parity pooled and per element at fp32 2e-4, bf16 2e-2 (TOL of
tests/test_hip_kernels.py), with the `local_tol` rule of DESIGN.md section 3 wired in (computed only when a bf16 row exceeds the per-element bound,
and reported); statistics against float64 sums of the STORED output at rtol 1e-5, atol 1e-3.  Bit equalities, from identical arithmetic:
background = 1 equals background = 0; a strided or misaligned row equals its contiguous partner whenever the forms agree on (kernel, gpt, nt,
splits, cps); s2c equals the launch without it followed by ops.space_to_channel, the left channels of y untouched; the first output with fs
equals the output without it; every launch runs twice and y, s2c_out, fs_y and the slabs repeat bit for bit (the statistics are double atomics
and judged by their bar only).

NOT launched (pinned in tests/test_conv3_fwd_forms_cpu.py): volumes of 2^31 voxels (refused), grids beyond 66 000 voxels.

Measured on an MI355X, worst over the rows, pooled / per element (the last test of the file prints this table; no row needed the local_tol rule):
  96-byte kernel, unsplit   y        fp32 1.43e-7 / 7.65e-7   bf16 1.67e-3 / 3.14e-3      s2c_out  fp32 1.42e-7 / 6.80e-7   bf16 1.66e-3 / 2.89e-3
  96-byte kernel, split     y        fp32 1.58e-7 / 7.60e-7   bf16 1.68e-3 / 3.02e-3      slabs    fp32 1.54e-7 / 7.45e-7   bf16 3.26e-7 / 2.30e-6
  tiny kernel               y                                 bf16 1.87e-3 / 2.93e-3      slabs                             bf16 1.81e-7 / 9.16e-7
  row-major kernel          y        fp32 1.39e-7 / 6.64e-7   bf16 1.66e-3 / 2.79e-3
24 partner launches compared bit for bit, 2 skipped (the contiguous partner takes the tiny kernel).  No row exposed a defect; the one defect
of this work was found by reading and fixed before its rows ran (the tiny kernel's 16-byte slab store with Cout % 4 != 0).  Wall time of the
file: 2.0 s for its 161 cases (the slowest, 1.0 s, is the first launch of the process); tests/test_conv3_fwd_forms_cpu.py: 1.4 s for 166 cases.
The mutations that turn rows red: DESIGN.md section 3.2."""
import ctypes as C
import math
import time

import pytest
import torch
import torch.nn.functional as F

import conv3_fwd_cases as K
from layouts import SENT, assert_untouched, place_in, place_out
from parity import assert_parity, local_err
from test_hip_conv3_forms import TD, TOL, Guarded, addr, packs, place_x, rnd, same_bits

pytestmark = pytest.mark.gpu

WORST = {}             # (kernel group, dtype, quantity) -> [pooled, local, rows judged by the local_tol rule]
PARTNERS = [0, 0]      # bit comparisons with a partner launch made / skipped because the forms differ
SLOWEST = [0.0, ""]
T0 = [None]
OPS = {}


def _ops():
    from mi_seg_amd.hip import ops
    return ops


def _L():
    from mi_seg_amd.hip import lib
    return lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(autouse=True)
def _clock(request):
    if T0[0] is None:
        T0[0] = time.time()
    t = time.time()
    yield
    torch.cuda.synchronize()
    dt = time.time() - t
    if dt > SLOWEST[0]:
        SLOWEST[0], SLOWEST[1] = dt, request.node.name


class Out:
    """an output view of `shape` in the given layout, sentinels all around it (contiguous: between two guard runs)"""

    def __init__(self, shape, dtype, lay):
        self.slot = None if lay == "contig" else place_out(shape, dtype, lay)
        self.g = Guarded(math.prod(shape), dtype) if lay == "contig" else None
        self.view = self.g.t.view(shape) if lay == "contig" else self.slot.view

    def check(self, what):
        self.g.check(what) if self.slot is None else assert_untouched(self.slot, what)

    def untouched(self):
        return bool((self.view == SENT).all())


def exact(values, dtype):
    """`values` in a buffer of exactly their size between sentinels (sc_w, fs_w: a read beside them lands on a sentinel of 1536)"""
    return Guarded(values.numel(), dtype, values=values.to(dtype)).t.view(values.shape)


def operands(r):
    """(x values, pack, float64 reference of the bare convolution [B, D, H, W, Cout]) - shared by the rows of one shape, never modified"""
    key = (r["dt"], r["B"], r["dims"], r["Cin"], r["Cout"], r["dgrad"])
    if key not in OPS:
        dt, B, (D, H, W), Cin, Cout = TD[r["dt"]], r["B"], r["dims"], r["Cin"], r["Cout"]
        xv = rnd(B, D, H, W, Cin, dtype=dt, seed=501)
        x64 = xv.double().permute(0, 4, 1, 2, 3)
        if r["dgrad"]:      # the layer Cout -> Cin: its mirrored pack runs on dy
            w, _, pk = packs(Cout, Cin, r["dt"])
            ref = torch.nn.grad.conv3d_input((B, Cout, D, H, W), w.to(dt).double(), x64, padding=1)
        else:
            w, pk, _ = packs(Cin, Cout, r["dt"])
            ref = F.conv3d(x64, w.to(dt).double(), padding=1)
        OPS[key] = (xv, w, pk.t, ref.permute(0, 2, 3, 4, 1).contiguous())
    return OPS[key]


def piece_values(r):
    dt, B, (D, H, W), Cin, Cout = TD[r["dt"]], r["B"], r["dims"], r["Cin"], r["Cout"]
    v = {}
    if r["res"]:
        v["res"] = rnd(B, D, H, W, Cout, dtype=dt, seed=502)
    if r["sc"]:
        Csc = r["sc"][0]
        v["g"] = rnd(B, D, H, W, Csc, dtype=dt, seed=503)
        v["sc_w"] = (rnd(Cout, Csc, seed=504) / Csc ** 0.5).to(dt)
    if r["fs"]:
        v["fs_w"] = (rnd(Cout, Cin, seed=505) / Cin ** 0.5).to(dt)
    return v


def launch(r, judge_form=True):
    """the row's launch, twice, each into fresh outputs; every sentinel checked; returns the first run's outputs, form and return code"""
    L = _L()
    lib = L.load()
    dt, B, (D, H, W), Cout = TD[r["dt"]], r["B"], r["dims"], r["Cout"]
    xv, _, pk, _ = operands(r)
    v = piece_values(r)
    x = place_x(xv, r["dt"], r["lay"]["x"])
    res = place_in(v["res"], r["res"]) if r["res"] else None
    g = place_in(v["g"], r["sc"][1]) if r["sc"] else None
    scw = exact(v["sc_w"], dt) if r["sc"] else None
    fsw = exact(v["fs_w"], dt) if r["fs"] else None
    nstat = lib.miseg_instnorm_stat_bytes(B, Cout) // 8
    runs = []
    for _ in range(2):
        o = dict(y=Out((B, D, H, W, Cout), dt, r["lay"]["y"]))
        if r["s2c"]:
            o["s2c"] = Out((B, D // 2, H // 2, W // 2, 8 * r["s2c"]), dt, "contig")
        if r["fs"]:
            o["fs_y"] = Out((B, D, H, W, Cout), dt, r["fs"][1])
            if r["fs"][0]:
                o["fs_stat"] = Guarded(nstat, torch.float64, fill=0.0)
        if r["stat"]:
            o["stat"] = Guarded(nstat, torch.float64, fill=0.0)
        a = dict(x=addr(x), y=addr(o["y"].view), wpk=addr(pk), ws=0, res=addr(res), stat=addr(o["stat"].t) if "stat" in o else 0, sc_x=addr(g), sc_w=addr(scw),
                 s2c=addr(o["s2c"].view) if "s2c" in o else 0, fs_w=addr(fsw), fs_y=addr(o["fs_y"].view) if "fs_y" in o else 0,
                 fs_stat=addr(o["fs_stat"].t) if "fs_stat" in o else 0)
        prm = K.params(r, L, a)
        rc, f = K.form(L, prm)
        if judge_form:
            K.check_form(r, L, rc, f)
        if f.plan.workspace_bytes:
            o["ws"] = Guarded(f.plan.workspace_bytes // 4, fill=float("nan"))
            prm.workspace = addr(o["ws"].t)
        o["rc"], o["f"] = lib.miseg_conv3_fwd(C.byref(prm), _stream()), f
        for k, b in o.items():
            if k not in ("rc", "f"):
                b.check(f"{r['id']} {k}")
        runs.append(o)
    for k in ("y", "s2c", "fs_y"):
        if k in runs[0]:
            same_bits(runs[0][k].view, runs[1][k].view, f"{r['id']} {k}")
    if "ws" in runs[0]:
        same_bits(runs[0]["ws"].t, runs[1]["ws"].t, f"{r['id']} slabs")
    return runs[0]


def _group(r):
    k = r["form"]["kernel"]
    return {"TINY": "tiny", "RM": "row-major"}.get(k, "f96-split" if r["form"]["splits"] > 1 else "f96")


def parity(r, quantity, got, ref, compose=None):
    """assert_parity at TOL; a bf16 result beyond the per-element bound is judged by the local_tol rule: at most twice the local
    error of torch's own bf16 composition `compose()` against the same reference - never below TOL, and the pooled check keeps TOL"""
    what, tol = f"{r['id']} {quantity}", TOL[r["dt"]]
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
    w = WORST.setdefault((_group(r), r["dt"], quantity), [0.0, 0.0, 0])
    w[0], w[1], w[2] = max(w[0], pooled), max(w[1], loc), w[2] + int(rule)


def stats_match(r, what, stat, stored):
    """the fp64 statistics against float64 sums of the STORED (rounded) output"""
    B, Cout = r["B"], r["Cout"]
    s = stat.t.view(-1, B, Cout, 2).sum(0)
    yf = stored.double().reshape(B, -1, Cout)
    assert torch.allclose(s[..., 0], yf.sum(1), rtol=1e-5, atol=1e-3), f"{r['id']} {what}: sums"
    assert torch.allclose(s[..., 1], (yf * yf).sum(1), rtol=1e-5, atol=1e-3), f"{r['id']} {what}: sums of squares"


def s2c_order(t):
    """[B, D, H, W, C] -> [B, D/2, H/2, W/2, 8 C], block j = 4 (d & 1) + 2 (h & 1) + (w & 1)"""
    B, D, H, W, Cc = t.shape
    return t.reshape(B, D // 2, 2, H // 2, 2, W // 2, 2, Cc).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(B, D // 2, H // 2, W // 2, 8 * Cc)


def contiguous_partner(r):
    return dict(r, lay=dict(x="contig", y="contig"), res="contig" if r["res"] else None, sc=(r["sc"][0], "contig") if r["sc"] else None,
                fs=(r["fs"][0], "contig") if r["fs"] else None, bg=0, id=r["id"] + " (contiguous partner)")


def equal_where_the_arithmetic_is(r, o, p, keys, what):
    if K.same_arithmetic(o["f"]) != K.same_arithmetic(p["f"]):
        PARTNERS[1] += 1
        return
    PARTNERS[0] += 1
    for k in keys:
        if k in o:
            same_bits(o[k].t if k == "ws" else o[k].view, p[k].t if k == "ws" else p[k].view, f"{r['id']} {k} against {what}")


@pytest.mark.parametrize("r", K.FWD, ids=lambda r: r["id"])
def test_forward_launch(r):
    L = _L()
    dt, Cout = TD[r["dt"]], r["Cout"]
    xv, w, _, conv = operands(r)
    v = piece_values(r)
    o = launch(r)
    f = o["f"]
    if r["refuse"]:
        assert o["rc"] == K.UNSUPPORTED, (r["id"], o["rc"])
        assert all(o[k].untouched() for k in ("y", "s2c", "fs_y") if k in o), f"{r['id']}: a refused launch wrote an output"
        assert all(bool((o[k].t == 0).all()) for k in ("stat", "fs_stat") if k in o) and ("ws" not in o or bool(torch.isnan(o["ws"].t).all())), r["id"]
        return
    L.check(o["rc"], "miseg_conv3_fwd")
    wq = w.to(dt)

    def compose():      # torch's own composition in the compute dtype: every stage rounded as a chain of torch ops would
        x32 = xv.float().permute(0, 4, 1, 2, 3)
        c = (torch.nn.grad.conv3d_input((r["B"], Cout) + r["dims"], wq.float(), x32, padding=1) if r["dgrad"] else F.conv3d(x32, wq.float(), padding=1)).permute(0, 2, 3, 4, 1).to(dt)
        if f.plan.sc:
            c = (c.float() + (v["g"].float() @ v["sc_w"].float().t()).to(dt).float()).to(dt)
        return (c.float() + v["res"].float()).to(dt) if r["res"] else c

    if f.plan.defer_slabs:      # the launch stops after its slabs: y and the statistics are the caller's next launch's
        assert o["y"].untouched() and bool((o["stat"].t == 0).all()), f"{r['id']}: a deferred launch wrote y or the statistics"
        slabs = o["ws"].t.double().view((f.plan.splits,) + tuple(conv.shape)).sum(0)
        parity(r, "slabs", slabs, conv)
        return
    ref = conv
    if f.plan.sc:
        ref = ref + v["g"].double() @ v["sc_w"].double().t()
    if r["res"]:
        ref = ref + v["res"].double()
    y, Cl = o["y"].view, r["s2c"] if f.plan.s2c else 0
    if Cl:
        assert bool((y[..., :Cl] == SENT).all()), f"{r['id']}: the left channels of y were written"
        parity(r, "s2c", o["s2c"].view, s2c_order(ref[..., :Cl]), lambda: s2c_order(compose()[..., :Cl]))
    parity(r, "y", y[..., Cl:], ref[..., Cl:], lambda: compose()[..., Cl:])
    if r["stat"]:
        assert not Cl
        stats_match(r, "stat", o["stat"], y)
    if f.plan.fs:
        parity(r, "fs_y", o["fs_y"].view, xv.double() @ v["fs_w"].double().t(), lambda: (xv.float() @ v["fs_w"].float().t()).to(dt))
        if "fs_stat" in o:
            stats_match(r, "fs_stat", o["fs_stat"], o["fs_y"].view)
    # bit equalities with partner launches of identical arithmetic
    lays = [r["lay"]["x"], r["lay"]["y"], r["res"], r["sc"][1] if r["sc"] else None, r["fs"][1] if r["fs"] else None]
    if r["bg"] or any(lay not in (None, "contig") for lay in lays):
        equal_where_the_arithmetic_is(r, o, launch(contiguous_partner(r), judge_form=False), ("y", "s2c", "fs_y", "ws"), "the contiguous foreground launch")
    if Cl:
        p = launch(dict(r, s2c=0, id=r["id"] + " (without s2c)"), judge_form=False)
        assert K.same_arithmetic(p["f"]) == K.same_arithmetic(f)
        same_bits(y[..., Cl:], p["y"].view[..., Cl:], f"{r['id']} right channels against the launch without s2c")
        from mi_seg_amd.hip.functional import STD_OFFSETS
        same_bits(o["s2c"].view, _ops().space_to_channel(p["y"].view[..., :Cl], STD_OFFSETS), f"{r['id']} s2c_out against space_to_channel of the plain output")
    if f.plan.fs:
        p = launch(dict(r, fs=None, id=r["id"] + " (without fs)"), judge_form=False)
        assert K.same_arithmetic(p["f"]) == K.same_arithmetic(f)
        same_bits(y, p["y"].view, f"{r['id']} first output against the launch without fs")


def test_zz_report_the_worst_errors():
    """prints the error table of this run (pytest -s): kernel group, dtype, quantity, worst pooled and per-element error, rows judged by the local_tol rule"""
    for (grp, dt, q), (pooled, loc, rule) in sorted(WORST.items()):
        print(f"WORST {grp:10s} {dt:4s} {q:5s} pooled {pooled:.2e} local {loc:.2e} local_tol-rule rows {rule}")
    print(f"PARTNERS compared bit for bit {PARTNERS[0]}, skipped (another form) {PARTNERS[1]}")
    print(f"WALL {time.time() - T0[0]:.1f} s, slowest case {SLOWEST[0]:.2f} s: {SLOWEST[1]}")
    assert WORST
