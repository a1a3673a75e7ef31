"""Launch forms, volume edges and operand layouts of the 3x3x3 weight-gradient kernels (csrc/conv3d.hip): miseg_conv3_wgrad - the slab kernel's
pipelined and plain loop (conv3_wgrad_kernel<T, WBD, PIPED>), its direct epilogue and its slab route with the reduce launch, the narrow kernels
(conv3_wgrad_narrow_kernel<NCO, NCI>), the tiny kernels (conv3_wgrad_tiny_kernel<S>) -, miseg_conv3_wgrad_group (conv3_wgrad_group_kernel<T, WBD,
PIPED, WALK>) and the weight packs (miseg_pack_conv3_weight / miseg_pack_conv3_batch).

The rows are tests/conv3_cases.py, the table tests/test_conv3_forms_cpu.py pins on the host-only form calls: every row goes through
`ops._call` with its ctypes struct (leading dimensions and bases chosen freely), and BEFORE the launch the form of these very params
(miseg_conv3_wgrad_form / miseg_conv3_wgrad_group_form - the struct the launchers dispatch on) must be the one the row's id carries.  Form ->
rows: `wgrad-<dtype>-<piped|plain>-<walk|one>-<direct1|direct2|slabs-spg1|slabs-spgN>[-atomic]-*` (the plain loop: fp32 always, bf16 through
ragged channels `40 -> 72`, misaligned operands `x-off8` / `dy-ldodd`, a volume thinner than a brick `d3` / `h7` / `w5`; `walk`: a workgroup
walks several bricks, through `cap1|2|3` = max_workgroups or 256 bricks and more; `direct2` stores (modes 0 and 2), `direct1` adds (mode 1);
`spgN`: more than one split per reduce group), `narrow-<NCO>x<NCI>[-cap][-walk]-mode<m>-*`, `wtiny-s<3|6>-mode<m>-*` (B = 64 is the last batch
they take: `not-tiny-b65-*` answers the slab kernel), `not-narrow-*`, `not-tiny-*`, `group-<plain|mixed>[-walk]-<dtype>` (the four (PIPED, WALK)
grids, direct and slab layers, layers of one and of two bricks that the target's unit count ignores).

Operands: x lies in a NaN-filled buffer of rows with more than two depth slabs of NaN rows before and behind the view (a halo read outside the
volume poisons the result) and NaN beside every row where the layout leaves room; dy comes from tests/layouts.py (NaN all around); with B = 2
the samples differ; dw sits between sentinels and starts from random values in modes 0 and 1 (mode 0 must overwrite them, mode 1 is judged
as after - before) and from zeros in mode 2; the workspace is NaN-filled, holds exactly `workspace_bytes` and sits between sentinels (grouped:
exactly miseg_conv3_wgrad_group_workspace_bytes); packs are written into NaN-filled buffers of exactly miseg_pack_conv3_elems elements between
sentinels, and the batched launch must give the same bits.  References are float64 torch.nn.grad.conv3d_weight on the very operands the kernel
got; tests/parity.py judges pooled and per element at the tolerances tests/test_hip_kernels.py uses for these calls (fp32 2e-4, bf16 2e-2, twice
that for mode 1; the tiny kernels 1e-5 and 1e-4 for mode 1).  The `local_tol` rule of DESIGN.md section 3 is wired in (max(tol, 2 x the local error
of torch's own bf16 composition against the same float64 reference), computed only when a bf16 row exceeds the per-element bound, and reported).
Every launch runs twice: the slab sets (workspaces) and every gradient with a single producer per element (direct epilogue, narrow, tiny) must
repeat bit for bit; the atomic reduce is judged by parity only.

NOT launched (pinned in tests/test_conv3_forms_cpu.py): the `span >= 2^31` exit from the pipelined loop (a halo slab of 2 GB); the reduce launch
with ONE group per tile (plain read-modify-write instead of atomics), which needs Cout x ceil(Cin / 48) >= 2048.  The forward and data-gradient
kernels (miseg_conv3_fwd) have no rows here: their table is tests/conv3_fwd_cases.py, launched by tests/test_hip_conv3_fwd_forms.py.

Measured on an MI355X, worst over the rows, pooled / per element (the last test of the file prints this table; no row needed the local_tol rule):
  dw, slab kernels      fp32 3.4e-7 / 1.4e-6    bf16 1.7e-7 / 8.3e-7   (bars 2e-4 / 2e-2: bf16 products are exact in fp32, only the order of summation differs)
  dw, grouped launch    fp32 2.8e-7 / 9.3e-7    bf16 2.5e-7 / 1.1e-6
  dw, tiny kernels                              bf16 6.9e-7 / 2.4e-6   (bar 1e-5)
No row exposed a defect: no wrong number, no overwritten sentinel, no NaN read.  Wall time of the file: 1.6 s for its 64 cases (the slowest,
0.5 s, is the first launch of the process).

That the file can fail - seven mutations of the kernels, each built from a copy outside the repository and run once; all give wrong numbers from
in-bounds accesses only (loops that do less, dropped terms).  Red rows of this file / of the older tests (tests/test_hip_kernels.py
`test_conv3_fwd_dgrad_wgrad`, `test_conv3_wgrad_grouped`, `test_conv3_wgrad_tiny_volumes`, `test_conv3_exact_integers`, tests/test_hip_conv3_wgrad_ahead.py):
  1. the plain (not pipelined) brick loop ended after its first brick: all ten `wgrad-*-plain-walk-*` rows and all six `group-*` rows (their
     layers walk 4 .. 14 bricks); the `piped-walk` rows stay green / old: 3 red (`128 -> 256` fp32 at 12^3, both grouped tests);
  2. the narrow reduce started at slab 1: all ten `narrow-*` rows / old: the four 16 / 32-channel bf16 cases and the exact-integer test red;
  3. the scalar staging of x dropped its last channel: `*-x-off8`, `*-x-ldodd-dy-off8`, `not-narrow-x-off8`, `not-tiny-x-off8`, `group-plain-bf16`,
     `group-plain-walk-bf16` (their sliced / 8-byte-based layers) / old: 4 red (the ragged-channel cases);
  4. the direct epilogue in mode 1 stored instead of adding: the three `*-direct1-*` rows and all six `group-*` rows / old: 4 red;
  5. the reduce kernel's remainder loop dropped (groups of fewer than four splits lose them): all 27 `*-slabs-*` rows and the six `group-*` rows /
     old: 38 red;
  6. the grouped kernel's WALK form stopped after its first unit: the three `group-*-walk-*` rows / old: the `background` case of the
     grouped test of test_hip_conv3_wgrad_ahead.py red, everything else green;
  7. the tiny kernels skipped their last sample: the four `wtiny-*` rows with B > 1 / old: the three B > 1 cases of `test_conv3_wgrad_tiny_volumes` red.
The older tests caught each mutation too, through other shapes; what they did not observe is WHICH form a case ran, operands that are not
contiguous and aligned, and writes beside dw, the workspace and the packs."""
import ctypes as C
import time

import pytest
import torch

import conv3_cases as K
from layouts import SENT, _bits, place_in
from parity import assert_parity, local_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {"f32": 2e-4, "bf16": 2e-2}
TINY_WGRAD_TOL, TINY_WGRAD_ACC_TOL = 1e-5, 1e-4      # tests/test_hip_kernels.py::test_conv3_wgrad_tiny_volumes
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
GUARD = 64
WORST = {}             # (call, dtype, quantity) -> [pooled, local, rows judged by the local_tol rule]
SLOWEST = [0.0, ""]
T0 = [None]


def _ops():
    from mi_seg_amd.hip import ops
    return ops


def _L():
    from mi_seg_amd.hip import lib
    return lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rnd(*shape, dtype=torch.float32, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed + 7 * sum(shape))
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(dtype)


def addr(t):
    return int(t.data_ptr()) if t is not None else 0


class Guarded:
    """n elements of `dtype` between two runs of GUARD sentinels"""

    def __init__(self, n, dtype=torch.float32, fill=SENT, values=None):
        self.buf = torch.full((GUARD + n + GUARD,), SENT, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + n]
        self.t.copy_(values.reshape(-1)) if values is not None else self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0

    def check(self, what):
        g = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]])
        assert bool((g == SENT).all()), f"{what}: a sentinel beside the buffer was overwritten"


def place_x(values, dtn, lay):
    """the convolution's input [B, D, H, W, C] in a NaN-filled buffer of rows: more than two depth slabs of NaN rows before and behind the
    view (a halo read outside the volume poisons the result), NaN beside every row where the layout leaves room"""
    B, D, H, W, Cc = values.shape
    off, ld = K.layout(Cc, dtn, lay)
    rows = B * D * H * W
    pre = -(-(2 * H * W + W + 2) // 16) * 16
    buf = torch.full((pre + rows + pre, ld), float("nan"), dtype=values.dtype, device=DEV)
    view = buf[pre:pre + rows, off:off + Cc].unflatten(0, (B, D, H, W))
    view.copy_(values)
    assert (view.data_ptr() % 16 == 0) == (lay != "off8") and view.stride(-2) == ld
    return view


def check_layout(r, view, c, lay):
    off, ld = K.layout(c, r["dt"], lay)
    assert view.stride(-2) == ld and (view.data_ptr() % 16 == 0) == (lay != "off8"), (r.get("id"), view.stride(), ld)


def _note(call, dt, quantity, pooled, loc, rule):
    w = WORST.setdefault((call, dt, quantity), [0.0, 0.0, 0])
    w[0], w[1], w[2] = max(w[0], pooled), max(w[1], loc), w[2] + int(rule)


def parity(r, call, quantity, got, ref, tol, compose=None):
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
    _note(call, r["dt"], quantity, pooled, loc, rule)


def same_bits(a, b, what):
    assert torch.equal(_bits(a.contiguous()), _bits(b.contiguous())), f"{what}: two launches with a fixed order of summation differ"


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


# ---------------------------------------------------------------------------------------------------------------- packs
PACKS = {}


def layer_weight(ci, co, seed=0):
    return rnd(co, ci, 3, 3, 3, seed=42 + seed) / (27 * ci) ** 0.5


def packs(ci, co, dtn):
    """(w, fwd pack, bwd pack) of a layer: miseg_pack_conv3_weight into NaN-filled buffers of exactly miseg_pack_conv3_elems elements between
    sentinels - a slot the pack kernel leaves unwritten and a convolution reads would poison that convolution's output"""
    key = (ci, co, dtn)
    if key not in PACKS:
        L, ops = _L(), _ops()
        lib = L.load()
        dt = L.BF16 if dtn == "bf16" else L.F32
        w = layer_weight(ci, co)
        f = Guarded(lib.miseg_pack_conv3_elems(ci, co, dt, 0), TD[dtn], fill=float("nan"))
        b = Guarded(lib.miseg_pack_conv3_elems(ci, co, dt, 1), TD[dtn], fill=float("nan"))
        ops._call("miseg_pack_conv3_weight", L.PackConv3(addr(w), addr(f.t), addr(b.t), ci, co, dt))
        f.check(f"forward pack {key}")
        b.check(f"backward pack {key}")
        PACKS[key] = (w, f, b)
    return PACKS[key]


@pytest.mark.parametrize("dtn", ["bf16", "f32"])
def test_packs_stay_inside_their_buffers_and_the_batched_launch_gives_the_same_bits(dtn):
    L = _L()
    lib = L.load()
    dt = L.BF16 if dtn == "bf16" else L.F32
    shapes = [(ci, co) for ci, co, d in K.PACK_SHAPES if d == dtn]
    descs = (L.PackConv3Desc * len(shapes))()
    mine, tile0 = [], 0
    for i, (ci, co) in enumerate(shapes):
        w, f, b = packs(ci, co, dtn)
        f2 = Guarded(f.t.numel(), TD[dtn], fill=float("nan"))
        b2 = Guarded(b.t.numel(), TD[dtn], fill=float("nan"))
        descs[i] = L.PackConv3Desc(addr(w), addr(f2.t), addr(b2.t), ci, co, tile0, 0)
        tile0 += lib.miseg_pack_conv3_tiles(ci, co, dt)
        mine.append((f2, b2))
    raw = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(DEV)
    L.check(lib.miseg_pack_conv3_batch(raw.data_ptr(), len(shapes), tile0, dt, None, None, _stream()), "pack_conv3_batch")
    for (ci, co), (f2, b2) in zip(shapes, mine):
        _, f, b = packs(ci, co, dtn)
        f2.check(f"batched forward pack {ci}->{co}")
        b2.check(f"batched backward pack {ci}->{co}")
        same_bits(f.t, f2.t, f"forward pack {ci}->{co} {dtn}")
        same_bits(b.t, b2.t, f"backward pack {ci}->{co} {dtn}")


# ---------------------------------------------------------------------------------------------------------------- weight gradient
def _wgrad_operands(l, seed):
    B, (D, H, W), Cin, Cout, dt = l["B"], l["dims"], l["Cin"], l["Cout"], TD[l["dt"]]
    xv = rnd(B, D, H, W, Cin, dtype=dt, seed=seed)
    x = place_x(xv, l["dt"], l["lay"]["x"])
    dy = place_in(rnd(B, D, H, W, Cout, dtype=dt, seed=seed + 1), l["lay"]["dy"])
    check_layout(l, dy, Cout, l["lay"]["dy"])
    base = torch.zeros(Cout, Cin, 3, 3, 3, device=DEV) if l["acc"] == 2 else rnd(Cout, Cin, 3, 3, 3, seed=seed + 2)
    ref = torch.nn.grad.conv3d_weight(xv.double().permute(0, 4, 1, 2, 3), base.shape, dy.double().permute(0, 4, 1, 2, 3), padding=1)
    return xv, x, dy, base, ref


def _wgrad_judge(r, l, call, dw, base, ref, xv, dy, tol, tol_acc):
    dw = dw.view(base.shape)
    got = dw - base if l["acc"] == 1 else dw      # mode 0 overwrites random values, mode 1 adds to them, mode 2 starts from zeros
    parity(r, call, "dw", got, ref, tol_acc if l["acc"] == 1 else tol,
           lambda: torch.nn.grad.conv3d_weight(xv.permute(0, 4, 1, 2, 3), base.shape, dy.permute(0, 4, 1, 2, 3).contiguous(), padding=1))


@pytest.mark.parametrize("r", K.WGRAD, ids=lambda r: r["id"])
def test_weight_gradient(r):
    L, ops = _L(), _ops()
    xv, x, dy, base, ref = _wgrad_operands(r, 301)
    runs = []
    for _ in range(2):
        dw = Guarded(base.numel(), values=base)
        prm = K.wgrad_params(r, L, dict(x=addr(x), dy=addr(dy), dw=addr(dw.t), ws=0))
        rc, f = K.wgrad_form(L, prm)
        K.check_wgrad_form(r, L, rc, f)
        ws = Guarded(f.plan.workspace_bytes // 4, fill=float("nan")) if f.plan.workspace_bytes else None
        prm.workspace = addr(ws.t) if ws else 0
        ops._call("miseg_conv3_wgrad", prm)
        dw.check(r["id"] + " dw")
        if ws:
            ws.check(r["id"] + " workspace")
        runs.append((dw.t, ws.t if ws else None, f))
    f = runs[0][2]
    slab_kernel = f.plan.kernel in (L.CONV3_WGRAD_F32, L.CONV3_WGRAD_BF16)
    if runs[0][1] is not None and not (slab_kernel and f.direct):      # the slab set repeats bit for bit
        same_bits(runs[0][1], runs[1][1], r["id"] + " slabs")
    if not slab_kernel or f.direct or f.reduce_groups == 1:               # a single producer per element; the atomic reduce is judged by parity only
        same_bits(runs[0][0], runs[1][0], r["id"] + " dw")
    tiny = f.plan.kernel == L.CONV3_WGRAD_TINY
    _wgrad_judge(r, r, "wgrad_tiny" if tiny else "wgrad", runs[0][0], base, ref, xv, dy, TINY_WGRAD_TOL if tiny else TOL[r["dt"]],
                 TINY_WGRAD_ACC_TOL if tiny else 2 * TOL[r["dt"]])


@pytest.mark.parametrize("r", K.GROUP, ids=lambda r: r["id"])
def test_grouped_weight_gradient(r):
    L = _L()
    lib = L.load()
    ops_ = [_wgrad_operands(l, 401 + 10 * i) for i, l in enumerate(r["layers"])]
    runs = []
    for _ in range(2):
        dws = [Guarded(o[3].numel(), values=o[3]) for o in ops_]
        descs = K.group_params(r, L, [dict(x=addr(o[1]), dy=addr(o[2]), dw=addr(d.t)) for o, d in zip(ops_, dws)])
        rc, forms = K.group_form(r, L, descs)
        K.check_group_form(r, L, rc, forms)
        nb = lib.miseg_conv3_wgrad_group_workspace_bytes(descs, len(r["layers"]))
        assert nb == sum(f.plan.workspace_bytes for f in forms) > 0
        ws = Guarded(nb // 4, fill=float("nan"))
        L.check(lib.miseg_conv3_wgrad_group(descs, len(r["layers"]), addr(ws.t), _stream()), "conv3_wgrad_group")
        ws.check(r["id"] + " workspace")
        for i, d in enumerate(dws):
            d.check(f"{r['id']} dw of layer {i}")
        runs.append((dws, ws, forms))
    same_bits(runs[0][1].t, runs[1][1].t, r["id"] + " slabs")
    for i, (l, (xv, x, dy, base, ref)) in enumerate(zip(r["layers"], ops_)):
        if runs[0][2][i].direct:
            same_bits(runs[0][0][i].t, runs[1][0][i].t, f"{r['id']} dw of layer {i}")
        _wgrad_judge(dict(r, id=f"{r['id']} layer {i}"), l, "wgrad_group", runs[0][0][i].t, base, ref, xv, dy, TOL[r["dt"]], 2 * TOL[r["dt"]])


def test_zz_report_the_worst_errors():
    """prints the error table of this run (pytest -s): call, dtype, quantity, worst pooled and per-element error, rows judged by the local_tol rule"""
    for (call, dt, q), (pooled, loc, rule) in sorted(WORST.items()):
        print(f"WORST {call:11s} {dt:4s} {q:5s} pooled {pooled:.2e} local {loc:.2e} local_tol-rule rows {rule}")
    print(f"WALL {time.time() - T0[0]:.1f} s, slowest case {SLOWEST[0]:.2f} s: {SLOWEST[1]}")
    assert WORST
