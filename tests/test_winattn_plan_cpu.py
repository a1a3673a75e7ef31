"""One host-side plan per attention launch (miseg_winattn_fwd_plan / miseg_winattn_bwd_plan): the table of tests/winattn_cases.py - the
production window shapes, every spec tests/test_hip_winattn_forms.py launches, the layout variants, the edges of every predicate and every
refusal - against plan fields worked out by hand from the dispatcher as it was before the plan existed; every instantiation of the four
kernel families reached by some row and listed by its launcher; nothing a launcher divides or strides by is zero; the two question entry
points equal the plan on every row, and over a seeded sweep answer what the parent commit's library answered wherever the plan accepts the
call.  CPU only."""
import ctypes as C

import pytest

import winattn_cases as G


def _L():
    from mi_seg_amd.hip import lib
    return lib


def _plans(spec, dt, kw):
    """((forward code, plan, message), (backward ...), params)"""
    L, so = _L(), _L().load()
    f, b = G.params(L, spec, dt, **kw)
    out = []
    for fn, prm in ((so.miseg_winattn_fwd_plan, f), (so.miseg_winattn_bwd_plan, b)):
        pl = L.WinattnPlan()
        rc = fn(C.byref(prm), C.byref(pl))
        out.append((rc, pl, so.miseg_last_error().decode() if rc else ""))
    return out[0], out[1], (f, b)


@pytest.mark.parametrize("row", G.ROWS, ids=lambda r: r[0])
def test_plan_of_the_table_rows(row):
    _, spec, dt, kw, exp_f, exp_b = row
    fwd, bwd, (f, b) = _plans(spec, dt, kw)
    so = _L().load()
    for bw, (rc, pl, msg), exp in ((0, fwd, exp_f), (1, bwd, exp_b)):
        want = G.expected(spec, dt, exp, bw, kw.get("drop_p", 0.0), kw.get("dtable", True), kw.get("tw"))
        assert rc == want.pop("rc", 0), msg
        assert {k: getattr(pl, k) for k in want} == want
        if rc != 0:      # a refusal: kernel none, every field zero, the launch's own text
            assert exp[2] in msg and all(getattr(pl, k) == 0 for k, _ in pl._fields_)
            continue
        # nothing a launcher or a kernel divides or strides by is zero
        assert pl.grid_x > 0 and pl.grid_y > 0 and pl.grid_z > 0 and 0 < pl.threads <= 1024 and pl.threads == 64 * pl.waves and 0 < pl.lds_bytes <= 160 * 1024
        assert pl.grid_x * pl.grid_y * pl.grid_z == pl.units and pl.tokens > 0 and pl.table_size >= 0
        assert pl.kernel != G.GLOBAL or (pl.tiles % 2 == 0 and pl.tiles * 16 >= pl.tokens > (pl.tiles - 2) * 16 and (bw == 0 or pl.grid_x % 2 == 0))
        assert pl.kernel != G.QUERY_LANE or (pl.threads >= pl.tokens and pl.hd4 * 4 * spec.heads == spec.C)
        assert pl.kernel != G.WINDOW or (pl.tokens <= 352 and (bw == 0 or pl.table_size <= 2200))
    # the question entry points are these plans
    assert G.answers(so, f, b) == tuple(int(rc == 0 and pl.kernel in (G.WINDOW, G.GLOBAL)) for rc, pl, _ in (fwd, bwd))


def test_literal_figures_of_the_production_rows():
    """the stage-1 launch of the bench nets (96^3 patch: a 48^3 grid of 48 channels in windows of 7^3) spelled out in full"""
    by = {r[0]: r for r in G.ROWS}
    _, spec, dt, kw, _, _ = by["production-stage1-48x48x48"]
    (rc, pl, _), (rcb, plb, _), _ = _plans(spec, dt, kw)
    got = lambda p: (p.kernel, p.mask, p.drop, p.table_grad, p.waves, p.hd4, p.tiles, p.vec, p.grid_x, p.grid_y, p.grid_z, p.threads, p.tokens, p.table_size, p.units, p.lds_bytes)
    assert rc == 0 and got(pl) == (G.WINDOW, 1, 0, 0, 8, 0, 0, 1, 1029, 1, 1, 512, 343, 2197, 1029, 47060)
    assert rcb == 0 and got(plb) == (G.WINDOW, 1, 0, 1, 8, 0, 0, 1, 1029, 1, 1, 512, 343, 2197, 1029, 81216)
    _, spec, dt, kw, _, _ = by["production-stage4-6x6x6"]
    (rc, pl, _), (rcb, plb, _), _ = _plans(spec, dt, kw)
    assert got(pl) == (G.WINDOW, 0, 0, 0, 11, 0, 0, 1, 24, 1, 1, 704, 216, 2197, 24, 47060)
    _, spec, dt, kw, _, _ = by["global-n216-the-vit"]
    (rc, pl, _), (rcb, plb, _), _ = _plans(spec, dt, kw)
    assert got(pl) == (G.GLOBAL, 0, 0, 0, 4, 0, 14, 0, 4, 12, 2, 256, 216, 0, 96, 61952) and got(plb) == (G.GLOBAL, 0, 0, 0, 4, 0, 14, 0, 8, 12, 2, 256, 216, 0, 192, 125696)
    _, spec, dt, kw, _, _ = by["geometry-fp32-B2-10x9x8-w7x7x7-s3x3x3-h2c32-amp4"]
    (rc, pl, _), (rcb, plb, _), _ = _plans(spec, dt, kw)
    assert got(pl) == (G.QUERY_LANE, 1, 0, 0, 6, 4, 0, 0, 16, 2, 1, 384, 343, 2197, 32, 4 * (2 * 343 * 16 + 2197 + 5 * 343 + 48))
    assert got(plb) == (G.QUERY_LANE, 1, 0, 1, 6, 4, 0, 0, 16, 2, 1, 384, 343, 2197, 32, 4 * (2 * 343 * 16 + 2 * 2197 + 5 * 343 + 48))


def _reached():
    fwd, bwd, glob, ql = set(), set(), set(), set()
    for _, spec, dt, kw, _, _ in G.ROWS:
        (rc, pl, _), (rcb, plb, _), _ = _plans(spec, dt, kw)
        for bw, r, p in ((0, rc, pl), (1, rcb, plb)):
            if r != 0:
                continue
            if p.kernel == G.WINDOW:
                (bwd if bw else fwd).add(((p.mask, p.table_grad, p.waves, p.drop) if bw else (p.mask, p.waves, p.drop), p.vec))
            elif p.kernel == G.GLOBAL:
                glob.add((bw, p.tiles, p.drop))
            else:
                ql.add((bw, dt, p.hd4))
    return fwd, bwd, glob, ql


def test_every_form_is_reached_by_some_row_and_by_no_unlisted_one():
    fwd, bwd, glob, ql = _reached()
    assert fwd == {(f, v) for f in G.WINDOW_FWD_FORMS for v in (0, 1)} and len(fwd) == 16      # 2 x 2 x 2 forms, each in both vec states
    assert bwd == {(f, v) for f in G.WINDOW_BWD_FORMS for v in (0, 1)} and len(bwd) == 16
    assert glob == {(bw,) + f for f in G.GLOBAL_FORMS for bw in (0, 1)} and len(glob) == 32
    assert ql == {(bw,) + f for f in G.QUERY_LANE_FORMS for bw in (0, 1)} and len(ql) == 24
    # ... and they are the launchers' own lists: nothing instantiated that no plan reaches, nothing reached that is not instantiated
    l_fwd, l_bwd, l_ql, l_glob = G.launcher_forms()
    assert sorted(l_fwd) == sorted(G.WINDOW_FWD_FORMS) and sorted(l_bwd) == sorted(G.WINDOW_BWD_FORMS)
    assert sorted(l_ql) == sorted(G.QUERY_LANE_FORMS) and sorted(l_glob) == sorted(G.GLOBAL_FORMS)


def test_the_rows_cover_every_spec_the_gpu_file_launches():
    import torch
    import winattn_ref as W
    rows = {(str(r[1]), r[2]) for r in G.ROWS}
    code = {torch.float32: G.F32, torch.bfloat16: G.BF16}
    for s, dts in W.GEOMETRY + W.HEAD_DIMS:
        assert all((str(s), code[dt]) in rows for dt in dts), s
    for s in W.OPTION_SPECS:
        assert (str(s), G.F32) in rows and (str(s), G.BF16) in rows
    for s in W.GLOBAL + [W.GLOBAL_ABOVE, W.PRODUCTION]:
        assert (str(s), G.BF16) in rows
    ids = [r[0] for r in G.ROWS]
    assert len(ids) == len(set(ids)) and len(ids) >= 200


def test_plan_refuses_a_null_plan_and_null_params():
    L, so = _L(), _L().load()
    pl = L.WinattnPlan()
    assert so.miseg_winattn_fwd_plan(None, C.byref(pl)) == G.BADARG and b"winattn_fwd: null params" in so.miseg_last_error()
    assert so.miseg_winattn_bwd_plan(None, C.byref(pl)) == G.BADARG and b"winattn_bwd: null pointer" in so.miseg_last_error()
    f, b = G.params(L, G.W.LAYOUT_SPEC)
    assert so.miseg_winattn_fwd_plan(C.byref(f), None) == G.BADARG and so.miseg_winattn_bwd_plan(C.byref(b), None) == G.BADARG
    assert so.miseg_winattn_on_matrix_cores(None) == 0 and so.miseg_winattn_bwd_on_matrix_cores(None) == 0


# sha256 over the answers of the two question entry points to the sweep below on the parameter sets the plan accepts, as libmiseg_hip.so of
# the PARENT commit (73fcda5, the dispatchers before the plan) gave them: scripts/winattn_answer_digest.py --lib <a build of that commit>.
# Of the 63185 forward and 65583 backward sets the plan refuses, the parent answered 1 for 5597 (3020 drop_p outside [0, 1), 2577 a table too
# large for LDS) and 2026 (1952 drop_p, 74 dbias_table without a table), every one in a class of DESIGN.md 3.4; this tree answers 0 there.  A change of this constant is a change of what the library answers - a decision, not a refresh.
SWEEP_SEED, SWEEP_COUNT = 20261021, 120000
PARENT_DIGEST = "80d4b0cccac0c4d861fdb69a04b83f85d3bc4373aa5402718cd7d5987dddb393"


def test_the_question_entry_points_answer_what_the_parent_answered():
    L, so = _L(), _L().load()
    l_fwd, l_bwd, l_ql, l_glob = (set(x) for x in G.launcher_forms())
    seen = set()

    def each(f, b, plans, codes, got):
        for bw, (pl, rc) in enumerate(zip(plans, codes)):
            if rc != 0:      # refused: no kernel, and the question is answered with 0
                assert pl.kernel == G.NONE and got[bw] == 0
                continue
            # whatever the sweep draws: an accepted plan names an instantiated kernel and a launchable grid
            if pl.kernel == G.WINDOW:
                assert ((pl.mask, pl.table_grad, pl.waves, pl.drop) in l_bwd) if bw else ((pl.mask, pl.waves, pl.drop) in l_fwd)
            elif pl.kernel == G.GLOBAL:
                assert (pl.tiles, pl.drop) in l_glob
            else:
                assert pl.kernel == G.QUERY_LANE and (f.dtype, pl.hd4) in l_ql
            assert got[bw] == int(pl.kernel != G.QUERY_LANE)
            assert pl.grid_x * pl.grid_y * pl.grid_z == pl.units > 0 and 0 < pl.threads <= 1024 and 0 < pl.lds_bytes <= 160 * 1024
            seen.add((bw, pl.kernel))

    digest, n = G.sweep(so, so, L, SWEEP_COUNT, SWEEP_SEED, each=each)
    assert not n["refused_yes"]
    assert seen == {(bw, k) for bw in (0, 1) for k in (G.QUERY_LANE, G.WINDOW, G.GLOBAL)}
    assert min(n["accepted"]) > 40000 and min(n["yes"]) > 5000 and min(n["refused"]) > 10000, n
    assert digest == PARENT_DIGEST, n
