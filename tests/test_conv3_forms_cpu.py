"""The launch forms of the 3x3x3 weight-gradient kernels, host only (miseg_conv3_wgrad_form, miseg_conv3_wgrad_group_form: the structs the
launchers of csrc/conv3d.hip dispatch on): every row of tests/conv3_cases.py answers the form its id carries, every value of every form field
a launcher switches on is reached by some row, the forms agree with the public plan, and the forms that no GPU test launches are pinned here:
the `span >= 2^31` exit from the pipelined loop and the single-group (non-atomic) reduce of a split weight gradient.  CPU only: the form
calls touch no device; tests/test_hip_conv3_forms.py launches the same rows on the card."""
import ctypes as C

import pytest

import conv3_cases as K
from test_conv3_plan import WGRAD_ROWS

A = K.A


def _L():
    from mi_seg_amd.hip import lib
    return lib


def _wgrad_form(r):
    L = _L()
    return K.wgrad_form(L, K.wgrad_params(r, L, K.wgrad_standins(r)))


def _group_form(r):
    L = _L()
    descs = K.group_params(r, L, [K.wgrad_standins(l) for l in r["layers"]])
    return descs, K.group_form(r, L, descs)


@pytest.mark.parametrize("r", K.WGRAD, ids=lambda r: r["id"])
def test_weight_gradient_row_takes_the_form_its_id_names(r):
    L = _L()
    rc, f = _wgrad_form(r)
    K.check_wgrad_form(r, L, rc, f)
    prm = K.wgrad_params(r, L, K.wgrad_standins(r))
    pl = L.Conv3WgradPlan()
    assert L.load().miseg_conv3_wgrad_plan(C.byref(prm), C.byref(pl)) == 0
    assert (pl.kernel, pl.workspace_bytes) == (f.plan.kernel, f.plan.workspace_bytes), r["id"]


@pytest.mark.parametrize("r", K.GROUP, ids=lambda r: r["id"])
def test_grouped_row_takes_the_forms_it_names(r):
    L = _L()
    descs, (rc, forms) = _group_form(r)
    K.check_group_form(r, L, rc, forms)
    assert L.load().miseg_conv3_wgrad_group_workspace_bytes(descs, len(r["layers"])) == sum(f.plan.workspace_bytes for f in forms)
    for l, f in zip(r["layers"], forms):
        assert f.plan.workspace_bytes == (0 if f.direct else f.ncob * f.ncib * f.nsplit * 27 * 48 * 48 * 4)
        assert f.fill == int(not f.direct and l["acc"] == 0) and f.group_target in range(7, 17)
    # a layer with at most two bricks is ignored by the target's unit count: without those layers the others keep their splits
    many = [i for i, f in enumerate(forms) if f.nbricks > 2]
    assert len(many) < len(forms), "the row holds a layer of at most two bricks"
    if 0 in many:      # (descs[0] carries the cap)
        sub = (L.Conv3Wgrad * len(many))(*[descs[i] for i in many])
        fsub = (L.Conv3WgradForm * len(many))()
        assert L.load().miseg_conv3_wgrad_group_form(sub, len(many), fsub) == 0
        assert [f.nsplit for f in fsub] == [forms[i].nsplit for i in many] and fsub[0].group_target == forms[0].group_target


def test_every_form_value_a_launcher_switches_on_is_reached():
    L = _L()
    slab, narrow, wtiny, routes = set(), set(), set(), set()
    for r in K.WGRAD:
        _, f = _wgrad_form(r)
        if f.plan.kernel == L.CONV3_WGRAD_NARROW:
            narrow.add((f.narrow_nco, f.narrow_nci, int(f.workgroups == r["cap"]), int(f.bricks_per_workgroup > 1)))
        elif f.plan.kernel == L.CONV3_WGRAD_TINY:
            wtiny.add((f.tiny_s, r["acc"]))
        else:
            slab.add((r["dt"], f.piped, int(f.bricks_per_workgroup > 1), f.vec_x, f.vec_dy))
            routes.add((r["dt"], f.direct, r["acc"], 0 if f.direct else (1 if f.spg == 1 else 2)))
    loops = {(dt, p, w) for dt, p, w, _, _ in slab}
    assert loops == {("f32", 0, 0), ("f32", 0, 1), ("bf16", 0, 0), ("bf16", 0, 1), ("bf16", 1, 0), ("bf16", 1, 1)}, sorted(loops)
    assert {(vx, vd) for _, p, _, vx, vd in slab if not p} == {(1, 1), (0, 1), (1, 0), (0, 0)}
    for dt in ("f32", "bf16"):      # the direct epilogue in modes 0, 1, 2 (0 and 2 store), the slab route in modes 0, 1, 2
        assert {(d, a) for t, d, a, _ in routes if t == dt and d} == {(2, 0), (1, 1), (2, 2)}, dt
        assert {a for t, d, a, s in routes if t == dt and not d and s == 1} == {0, 1, 2}, dt
    assert {a for t, d, a, s in routes if not d and s == 2} == {0, 1, 2}
    assert {(a, b) for a, b, _, _ in narrow} == {(1, 1), (1, 2), (2, 1), (2, 2)} and {(c, w) for _, _, c, w in narrow} >= {(0, 0), (1, 1)}, sorted(narrow)
    assert {s for s, _ in wtiny} == {3, 6} and {a for _, a in wtiny} == {0, 1, 2}

    grids, layer_forms = set(), set()
    for r in K.GROUP:
        _, (_, forms) = _group_form(r)
        grids |= {(r["dt"], f.piped, f.walk) for f in forms}
        layer_forms |= {(f.direct, int(f.nsplit > 1), f.fill) for f in forms}
    assert grids == {("bf16", 0, 0), ("bf16", 0, 1), ("bf16", 1, 0), ("bf16", 1, 1), ("f32", 0, 0), ("f32", 0, 1)}, sorted(grids)
    assert layer_forms == {(1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 1, 1)}, sorted(layer_forms)


def test_the_forms_agree_with_the_plans_on_the_bench_shapes():
    L = _L()
    lib = L.load()
    for dt, S, Cin, Cout, kernel, ws, _ in WGRAD_ROWS:
        p = L.Conv3Wgrad(A, Cin, A, Cout, A, 1, S, S, S, Cin, Cout, dt, 0, None, 0)
        f = L.Conv3WgradForm()
        assert lib.miseg_conv3_wgrad_form(C.byref(p), C.byref(f)) == 0
        assert (f.plan.kernel, f.plan.workspace_bytes) == (kernel, ws)
        if kernel in (L.CONV3_WGRAD_F32, L.CONV3_WGRAD_BF16):      # the bench's bf16 layers with whole 48-channel blocks and a whole brick per axis are the pipelined ones
            assert f.piped == int(dt == 1 and Cin % 48 == 0 and Cout % 48 == 0 and S >= 8)


def test_the_forms_no_gpu_test_launches():
    L = _L()
    lib = L.load()
    # the pipelined weight-gradient loop keeps 32-bit item offsets: a halo slab of 2^31 bytes or more leaves it
    w = L.Conv3WgradForm()
    for side, piped in ((1024, 1), (2048, 0)):      # 6 x side^2 rows of 96 bytes: 0.6e9 / 2.4e9 bytes
        q = L.Conv3Wgrad(A, 48, A, 48, A, 1, 8, side, side, 48, 48, L.BF16, 0, None, 0)
        assert lib.miseg_conv3_wgrad_form(C.byref(q), C.byref(w)) == 0 and (w.piped, w.plan.kernel) == (piped, L.CONV3_WGRAD_BF16)
    # a split weight gradient whose reduce launch has ONE group per tile (plain read-modify-write, no atomics) needs 2048 (co, ci-block) tiles
    q = L.Conv3Wgrad(A, 96, A, 1024, A, 1, 5, 9, 11, 96, 1024, L.BF16, 0, None, 0)
    assert lib.miseg_conv3_wgrad_form(C.byref(q), C.byref(w)) == 0 and (w.direct, w.reduce_groups, w.spg, w.nsplit) == (0, 1, 5, 5)
    q = L.Conv3Wgrad(A, 96, A, 1008, A, 1, 5, 9, 11, 96, 1008, L.BF16, 0, None, 0)
    assert lib.miseg_conv3_wgrad_form(C.byref(q), C.byref(w)) == 0 and w.reduce_groups == 2


def test_the_form_calls_refuse_bad_params():
    L = _L()
    lib = L.load()
    w = L.Conv3WgradForm()
    assert lib.miseg_conv3_wgrad_form(None, C.byref(w)) != 0 and lib.miseg_conv3_wgrad_form(C.byref(L.Conv3Wgrad(A, 48, A, 48, A, 1, 8, 8, 8, 48, 48, 7, 0, None, 0)), C.byref(w)) != 0      # unknown dtype
    assert lib.miseg_conv3_wgrad_form(C.byref(L.Conv3Wgrad(A, 48, A, 48, A, 1, 0, 8, 8, 48, 48, 1, 0, None, 0)), C.byref(w)) != 0      # empty volume
    one = (L.Conv3Wgrad * 1)(L.Conv3Wgrad(A, 48, A, 48, A, 1, 8, 8, 8, 48, 48, 1, 0, None, 0))
    assert lib.miseg_conv3_wgrad_group_form(one, 0, (L.Conv3WgradForm * 1)()) != 0 and lib.miseg_conv3_wgrad_group_form(one, 25, (L.Conv3WgradForm * 1)()) != 0
    assert lib.miseg_conv3_wgrad_group_form(one, 1, None) != 0
