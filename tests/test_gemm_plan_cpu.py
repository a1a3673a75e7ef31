"""One host-side plan per miseg_gemm launch (miseg_gemm_plan): the table of tests/gemm_cases.py - the GEMM shapes of the bench nets and
the edges of every predicate - against plan fields worked out by hand from the dispatcher as it was before the plan existed; every kernel
family, every small and streaming instantiation, every output mode reached by some row; no divisor of a launch is zero; the seven question
entry points equal the plan's fields on every row, and over a seeded sweep answer what the parent commit's library answered.  FORM_ROWS, the
card-sized rows tests/test_hip_gemm_forms.py launches, are pinned the same way and reach every form without ROWS.  CPU only."""
import ctypes as C

import pytest

import gemm_cases as G


def _L():
    from mi_seg_amd.hip import lib
    return lib


def _plan(kw):
    L = _L()
    p = G.params(L, **kw)
    pl = L.GemmPlan()
    rc = L.load().miseg_gemm_plan(C.byref(p), C.byref(pl))
    return rc, pl, p


@pytest.mark.parametrize("row", G.ROWS, ids=lambda r: r[0])
def test_plan_of_the_table_rows(row):
    _, kw, expect = row
    _check_row(kw, expect, *_plan(kw))


def _form_plan(kw):
    L = _L()
    p = G.form_params(L, kw)
    pl = L.GemmPlan()
    rc = L.load().miseg_gemm_plan(C.byref(p), C.byref(pl))
    return rc, pl, p


@pytest.mark.parametrize("row", G.FORM_ROWS, ids=lambda r: r[0])
def test_plan_of_the_form_rows(row):
    """the rows tests/test_hip_gemm_forms.py launches on the card: each one's plan, with its operands in the row's layouts, has the fields worked
    out by hand, and the shape is as small as its family allows (every one of them is accepted)"""
    _, kw, expect = row
    rc, pl, p = _form_plan(kw)
    assert "rc" not in expect and "kernel" in expect
    _check_row(kw, expect, rc, pl, p)
    assert pl.kernel != G.SMALL or kw["M"] <= 2048
    assert _L().load().miseg_gemm_workspace_bytes(C.byref(p)) == pl.workspace_bytes


def _check_row(kw, expect, rc, pl, p):
    assert rc == expect.get("rc", 0)
    if rc != 0:
        assert pl.kernel == G.NONE and _L().load().miseg_last_error()
    got = {f: getattr(pl, f) for f in expect if f != "rc"}
    assert got == {f: v for f, v in expect.items() if f != "rc"}
    # the question entry points are this plan's fields
    assert G.answers(_L().load(), p) == (pl.fuses_stat, pl.fuses_anorm, pl.fuses_bstat, pl.fuses_scatter, pl.tn_fuses_colsum,
                                         pl.splits if pl.tn_fuses_colsum else 0, pl.workspace_bytes)
    if rc == 0:      # whatever a launcher or a kernel of this family divides by or strides with
        assert pl.grid_x > 0 and pl.grid_y > 0 and pl.grid_z > 0
        if pl.kernel == G.SMALL:
            assert pl.mtw > 0 and pl.ntw > 0 and pl.row_tiles > 0 and pl.col_groups > 0 and pl.cols_per_group == 16 * pl.ntw
            assert pl.grid_x == pl.row_tiles * pl.col_groups and pl.col_groups * pl.cols_per_group == kw["N"]
        if pl.kernel == G.STREAM:
            assert pl.k16 * 16 == kw["K"] and pl.nch > 0 and pl.col_groups == pl.grid_y and pl.col_groups * pl.cols_per_group == kw["N"] and pl.cols_per_group % 16 == 0
            assert 0 < pl.lds_bytes <= 160 * 1024 and (pl.stat == 0 or pl.cols_per_group <= 16 * pl.nch)
        if pl.kernel in (G.NT_GENERIC, G.TN_GENERIC, G.TN_STREAM):
            assert pl.splits == pl.grid_z > 0 and pl.k_per_split > 0 and (pl.splits - 1) * pl.k_per_split < kw["K"] <= pl.splits * pl.k_per_split
        if pl.kernel == G.NT_GENERIC:
            assert pl.nt in (1, 2, 3, 4)
        if pl.kernel == G.TN_STREAM:
            assert pl.wm * pl.wn == 4 and (pl.reduce_groups == 0) == (pl.reduce_blocks == 0) and pl.workspace_bytes == (pl.splits > 1) * pl.splits * kw["M"] * kw["N"] * 4


def test_every_launch_form_is_reached_by_a_row():
    plans = [_plan(kw)[1] for _, kw, e in G.ROWS if e.get("rc", 0) == 0]
    assert {pl.kernel for pl in plans} == {G.RANK1, G.RANK1_STAT, G.SMALL, G.STREAM, G.NT_GENERIC, G.TN_STREAM, G.TN_GENERIC}
    assert {pl.nt for pl in plans if pl.kernel == G.NT_GENERIC} == {3, 4}      # 1 and 2: the form rows below
    assert {(pl.wm, pl.wn) for pl in plans if pl.kernel == G.TN_STREAM} == {(4, 1), (1, 4), (2, 2)}
    for k in (G.NT_GENERIC, G.TN_GENERIC):
        assert {(pl.out_mode, pl.zero_fill) for pl in plans if pl.kernel == k} == {(G.STORE, 0), (G.ACCUMULATE, 0), (G.ATOMIC, 1), (G.ATOMIC, 0)}
    assert {(pl.out_mode, pl.zero_fill, min(pl.reduce_groups, 2)) for pl in plans if pl.kernel == G.TN_STREAM} == {
        (G.STORE, 1, 2), (G.ACCUMULATE, 0, 2), (G.STORE, 0, 0), (G.STORE, 0, 1)}
    assert {(pl.al_a, pl.al_b) for pl in plans if pl.kernel == G.NT_GENERIC} == {(1, 1), (0, 1), (1, 0)}
    # the instantiations: the table's own rows reach many, the form rows (a shape per tile / per K, a request each) every one, and no other
    small, stream = set(), set()
    for kw, form in G.form_rows():
        rc, pl, _ = _plan(kw)
        assert rc == 0
        got = ("small", pl.mtw, pl.ntw, pl.gelu, pl.stat, pl.anorm) if pl.kernel == G.SMALL else ("stream", pl.k16, pl.gelu, pl.nch, pl.stat, pl.scat, pl.anorm)
        assert got == form and (pl.kernel == G.SMALL or pl.kernel == G.STREAM)
        (small if pl.kernel == G.SMALL else stream).add(got[1:])
    assert small == G.SMALL_FORMS and len(small) == 36 and stream == G.STREAM_FORMS and len(stream) == 26
    # ... and they are the launchers' own lists: nothing instantiated that no plan reaches, nothing reached that is not instantiated
    listed_small, listed_stream = G.launcher_forms()
    assert sorted(listed_small) == sorted(G.SMALL_FORMS) and sorted(listed_stream) == sorted(G.STREAM_FORMS)
    assert {(pl.mtw, pl.ntw, pl.gelu, pl.stat, pl.anorm) for pl in plans if pl.kernel == G.SMALL} <= G.SMALL_FORMS
    assert {(pl.k16, pl.gelu, pl.nch, pl.stat, pl.scat, pl.anorm) for pl in plans if pl.kernel == G.STREAM} <= G.STREAM_FORMS
    assert {_plan(dict(M=4095, N=n, K=40))[1].nt for n in (8, 16, 24, 32, 40, 48, 56, 64, 96)} == {1, 2, 3, 4}


def test_the_form_rows_alone_reach_every_launch_form():
    """without ROWS: the seven families, the 36 + 26 instantiations and no other, nt 1 .. 4 under each dtype pair, both al_a and both al_b on
    each generic kernel, the three TN wave forms, every (output mode, zero fill) pair of the generic kernels, and the TN streaming path with
    one split, one reduce group, several reduce groups, accumulate, tn_colsum and defer_reduce"""
    rows = [(kw, _form_plan(kw)[1]) for _, kw, _ in G.FORM_ROWS]
    plans = [pl for _, pl in rows]
    assert {pl.kernel for pl in plans} == {G.RANK1, G.RANK1_STAT, G.SMALL, G.STREAM, G.NT_GENERIC, G.TN_STREAM, G.TN_GENERIC}
    assert {(pl.mtw, pl.ntw, pl.gelu, pl.stat, pl.anorm) for pl in plans if pl.kernel == G.SMALL} == G.SMALL_FORMS
    assert {(pl.k16, pl.gelu, pl.nch, pl.stat, pl.scat, pl.anorm) for pl in plans if pl.kernel == G.STREAM} == G.STREAM_FORMS
    assert {G.dtypes(kw) + (pl.nt,) for kw, pl in rows if pl.kernel == G.NT_GENERIC} == {(d, o, n) for d, o in ((0, 0), (1, 0), (1, 1)) for n in (1, 2, 3, 4)}
    assert {G.dtypes(kw) for kw, pl in rows if pl.kernel == G.TN_GENERIC} == {(0, 0), (1, 0), (1, 1)}
    assert {G.dtypes(kw) for kw, pl in rows if pl.kernel in (G.RANK1, G.RANK1_STAT)} == {(0, 0), (1, 1)}
    for k in (G.NT_GENERIC, G.TN_GENERIC):
        assert {pl.al_a for pl in plans if pl.kernel == k} == {0, 1} and {pl.al_b for pl in plans if pl.kernel == k} == {0, 1}
        assert {(pl.out_mode, pl.zero_fill) for pl in plans if pl.kernel == k} == {(G.STORE, 0), (G.ACCUMULATE, 0), (G.ATOMIC, 1), (G.ATOMIC, 0)}
    tns = [(kw, pl) for kw, pl in rows if pl.kernel == G.TN_STREAM]
    assert {(pl.wm, pl.wn) for _, pl in tns} == {(4, 1), (1, 4), (2, 2)}
    assert {(pl.out_mode, pl.zero_fill, min(pl.reduce_groups, 2), pl.splits > 1) for _, pl in tns} == {
        (G.STORE, 0, 0, False), (G.ACCUMULATE, 0, 0, False), (G.STORE, 0, 1, True), (G.ACCUMULATE, 0, 1, True), (G.STORE, 1, 2, True), (G.ACCUMULATE, 0, 2, True),
        (G.STORE, 0, 0, True)}      # (the last: defer_reduce)
    assert any(kw.get("colsum") for kw, _ in tns) and any(kw.get("defer") and pl.reduce_groups == 0 and pl.splits > 1 for kw, pl in tns)
    assert any(pl.splits % 16 and pl.splits > 16 for _, pl in tns)
    # the streaming NT kernel: a wave with more than one tile under every family whose sums or stores live across tiles, more than one chunk
    walks = {(pl.stat, pl.scat, pl.anorm) for kw, pl in rows if pl.kernel == G.STREAM and -(-kw["M"] // 32) > 4 * pl.grid_x}
    assert walks >= {(1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 0, 1)}
    assert {pl.nch for kw, pl in rows if pl.kernel == G.STREAM and pl.cols_per_group > 16 * pl.nch} >= {3, 12}
    assert any(pl.kernel == G.STREAM and pl.stat == 2 and pl.col_groups == 2 and pl.k16 == 18 for pl in plans)
    # the small kernel's grids: below the eight XCDs, a multiple of eight, not a multiple of eight
    gx = {pl.grid_x for pl in plans if pl.kernel == G.SMALL}
    assert any(g < 8 for g in gx) and any(g >= 8 and g % 8 == 0 for g in gx) and any(g > 8 and g % 8 for g in gx)
    # one exact-integer row per family
    assert {pl.kernel for kw, pl in rows if kw.get("ints")} == {G.RANK1, G.RANK1_STAT, G.SMALL, G.STREAM, G.NT_GENERIC, G.TN_STREAM, G.TN_GENERIC}
    ids = [r[0] for r in G.FORM_ROWS]
    assert len(ids) == len(set(ids))


def _instantiated(pl, small, stream):
    if pl.kernel == G.SMALL:
        return (pl.mtw, pl.ntw, pl.gelu, pl.stat, pl.anorm) in small
    if pl.kernel == G.STREAM:
        return (pl.k16, pl.gelu, pl.nch, pl.stat, pl.scat, pl.anorm) in stream
    return pl.kernel != G.NT_GENERIC or pl.nt in (1, 2, 3, 4)


def test_every_accepted_plan_on_a_dense_grid_names_an_instantiated_kernel():
    """every M of the small kernel against every N up to 384 (the norm-backward sums' limit) and some beyond, under each of the six requests;
    the streaming kernel's K against N up to the LDS limit: a plan that is accepted names a kernel of the launchers' lists (read from
    gemm.hip), and a request the question entry point said yes to is accepted"""
    L, so = _L(), _L().load()
    small, stream = (set(x) for x in G.launcher_forms())
    pl, tiles = L.GemmPlan(), set()
    for (g, s, a), req in G.REQUESTS.items():
        for N in list(range(16, 400, 16)) + [768, 2304, 3072, 4608, 16384]:
            p = G.params(L, 1, N, 64, **req)
            for M in range(1, 2049):
                p.M = M
                rc = so.miseg_gemm_plan(C.byref(p), C.byref(pl))
                asked_yes = {(0, 1, 0): pl.fuses_stat, (0, 2, 0): pl.fuses_bstat, (0, 0, 1): pl.fuses_anorm, (1, 0, 1): pl.fuses_anorm}.get((g, s, a), 1)
                assert rc == (0 if asked_yes else G.UNSUPPORTED), (M, N, req)
                if rc == 0:
                    assert pl.kernel == G.SMALL and (pl.gelu, pl.stat, pl.anorm) == (g, s, a) and _instantiated(pl, small, stream), (M, N, req, pl.mtw, pl.ntw)
                    tiles.add((pl.mtw, pl.ntw, g, s, a))
        for K in (48, 96, 144, 192, 288, 384):
            for N in range(16, 1024, 16):
                for M in (4096, 13824, 110592):
                    p = G.params(L, M, N, K, **req)
                    if so.miseg_gemm_plan(C.byref(p), C.byref(pl)) == 0:
                        assert _instantiated(pl, small, stream), (M, N, K, req)
    assert tiles == G.SMALL_FORMS      # the grid alone lands on every small instantiation


def test_no_row_is_listed_twice():
    ids = [r[0] for r in G.ROWS]
    assert len(ids) == len(set(ids)) and len(ids) >= 120


def test_plan_refuses_a_null_plan_and_null_params():
    so = _L().load()
    assert so.miseg_gemm_plan(None, C.byref(_L().GemmPlan())) == G.BADARG
    assert so.miseg_gemm_plan(C.byref(G.params(_L(), 64, 64, 64)), None) == G.BADARG
    assert G.answers(so, G.params(_L(), 0, 48, 4096, tn=1)) == (0,) * 7      # an empty product streams nothing (and divides by nothing)


# sha256 over the answers of the seven question entry points to the sweep below, as libmiseg_hip.so of the PARENT commit (61e7339, the
# dispatcher before miseg_gemm_plan) gave them: scripts/gemm_answer_digest.py, run against a build of that commit.  A change of this
# constant is a change of what the library answers - a decision, not a refresh.
SWEEP_SEED, SWEEP_COUNT = 20261020, 200000
PARENT_DIGEST = "6b8766a9a17f2d28d2ab49b25953d0fc0c6151b986d813f1f6c366f5cac1b944"


def test_the_question_entry_points_answer_what_the_parent_answered():
    L, so = _L(), _L().load()
    small, stream = (set(x) for x in G.launcher_forms())
    pl = L.GemmPlan()

    def each(p):      # whatever the sweep draws: an accepted plan names an instantiated kernel
        assert so.miseg_gemm_plan(C.byref(p), C.byref(pl)) != 0 or _instantiated(pl, small, stream), (p.M, p.N, p.K)

    digest, asked, yes = G.sweep(so, L, SWEEP_COUNT, SWEEP_SEED, each=each)
    assert asked > SWEEP_COUNT + 10000 and all(n >= 10 for n in yes.values()), yes      # every question answers yes now and then (scatter, the rarest: 16 times)
    assert digest == PARENT_DIGEST
