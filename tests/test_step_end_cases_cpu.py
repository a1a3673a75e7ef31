"""The table of the step-end reduction launches (tests/step_end_cases.py) without a GPU: unique ids, every hand-written form against the
restated host arithmetic and against what its id spells, every form the launchers can take named here with at least one row, the float64
references (tests/step_end_ref.py) against naive loops, the exactness of the integer runs, and the launchers' refusals, which fire before
anything is launched."""
import ctypes as C

import pytest
import torch

import step_end_cases as S
import step_end_ref as R


def _all_rows():
    return [(fam, r) for fam, rows, _, _ in S.FAMILIES for r in rows]


def test_ids_are_unique():
    ids = [r[0] for _, r in _all_rows()] + [r[0] for r in S.COLSUM_SHARED]
    assert len(ids) == len(set(ids)), sorted(i for i in set(ids) if ids.count(i) > 1)


@pytest.mark.parametrize("family", [f[0] for f in S.FAMILIES])
def test_every_rows_form_is_the_restated_one_and_what_its_id_spells(family):
    _, rows, form, spell = next(f for f in S.FAMILIES if f[0] == family)
    assert rows
    for rid, kw, want in rows:
        assert form(kw) == want, (rid, form(kw), want)
        assert rid.endswith("-" + spell(want)), rid
        if "dt" in kw:
            assert f"-{kw['dt']}-" in rid, rid


def _has(rows, pred):
    return [r[0] for r in rows if pred(r[1], r[2])]


def test_every_named_form_has_a_row():
    """the forms of the issue, written out: deleting a row that is the only one of its form fails here"""
    tn, red, csb, cs = S.TN_ROWS, S.REDUCE_ROWS, S.COLSUM_BATCH_ROWS, S.COLSUM_ROWS
    want = []
    for dt, kedges, stage in (("bf16", (1, 31, 32, 95, 96, 97), 96), ("f32", (1, 3, 5, 63, 64, 65), 64)):
        d = lambda k, dt=dt: k["dt"] == dt
        for K in kedges:
            want.append((f"tn {dt} K edge {K}", _has(tn, lambda k, f: d(k) and k["K"] == K and (k["M"], k["N"]) == (64, 64) and f[2] == 1 and f[3] == S.cdiv(K, stage) * stage)))
        want.append((f"tn {dt} two splits, short second", _has(tn, lambda k, f: d(k) and k["K"] == 2049 and f[2] == 2 and k["K"] % f[3] != 0 and (k["M"], k["N"]) == (8, 8))))
        want.append((f"tn {dt} three splits", _has(tn, lambda k, f: d(k) and k["K"] == 4100 and f[2] == 3 and (k["M"], k["N"]) == (8, 8))))
        want.append((f"tn {dt} K 98304", _has(tn, lambda k, f: d(k) and k["K"] == 98304 and f[2] == (47 if dt == "bf16" else 48) and (k["M"], k["N"]) == (8, 8))))
        for v in (1, 7, 63, 64, 65, 100):
            want.append((f"tn {dt} M {v}", _has(tn, lambda k, f: d(k) and k["M"] == v and "regroup" not in k)))
            want.append((f"tn {dt} N {v}", _has(tn, lambda k, f: d(k) and k["N"] == v and "regroup" not in k)))
        for lay in ("off8", "ldodd", "off2" if dt == "bf16" else "off4"):
            want.append((f"tn {dt} A {lay}", _has(tn, lambda k, f: d(k) and k.get("la") == lay and "lb" not in k and "lc" not in k and (f[5], f[6]) == (0, 1))))
            want.append((f"tn {dt} B {lay}", _has(tn, lambda k, f: d(k) and k.get("lb") == lay and "la" not in k and "lc" not in k and (f[5], f[6]) == (1, 0))))
        for lay in ("slice", "off4"):
            want.append((f"tn {dt} C {lay}", _has(tn, lambda k, f: d(k) and k.get("lc") == lay and "la" not in k and "lb" not in k)))
        want.append((f"tn {dt} store", _has(tn, lambda k, f: d(k) and f[4] == S.STORE and k.get("zeroed") == 1 and f[2] == 1)))
        want.append((f"tn {dt} add", _has(tn, lambda k, f: d(k) and f[4] == S.ADD and not k.get("zeroed"))))
        want.append((f"tn {dt} atomics onto zeros", _has(tn, lambda k, f: d(k) and f[4] == S.ATOMIC and k.get("zeroed") == 1)))
        want.append((f"tn {dt} atomics onto content", _has(tn, lambda k, f: d(k) and f[4] == S.ATOMIC and not k.get("zeroed"))))
        for rg, N, M in ((9, 72, 64), (8, 64, 33)):
            for split in (False, True):
                want.append((f"tn {dt} regroup {rg} split {split}", _has(tn, lambda k, f: d(k) and k.get("regroup") == rg and k["N"] == N and k["M"] == M and (f[2] > 1) == split)))
        # column sums, batched
        n = S.NVEC[dt]
        for rows in (1, 31, 512, 513, 767):
            want.append((f"colsum_batch {dt} vector rows {rows}", _has(csb, lambda k, f: d(k) and k["C"] == 64 and k["rows"] == rows and f[2] == "vec" and "lx" not in k)))
        for C_ in (n, 64 + n, 136):
            want.append((f"colsum_batch {dt} vector C {C_}", _has(csb, lambda k, f: d(k) and k["C"] == C_ and f[2] == "vec")))
        want.append((f"colsum_batch {dt} vector slice", _has(csb, lambda k, f: d(k) and k.get("lx") == "slice" and f[2] == "vec")))
        for C_ in (7, 65, 100):
            want.append((f"colsum_batch {dt} C {C_}", _has(csb, lambda k, f: d(k) and k["C"] == C_)))
        for C_ in (7, 65):
            for rows in (1, 3, 513):
                want.append((f"colsum_batch {dt} scalar C {C_} rows {rows}", _has(csb, lambda k, f: d(k) and k["C"] == C_ and k["rows"] == rows and f[2] == "scalar")))
        for lay in ("off8", "ldodd", "off2" if dt == "bf16" else "off4"):
            want.append((f"colsum_batch {dt} scalar C 64 {lay}", _has(csb, lambda k, f: d(k) and k["C"] == 64 and k.get("lx") == lay and f[2] == "scalar")))
        want.append((f"colsum_batch {dt} shared out", [r[0] for r in S.COLSUM_SHARED if r[1] == dt]))
        # the lone column sum
        for acc in (0, 1):
            a = lambda k, acc=acc: d(k) and k["accumulate"] == acc
            for cv in (1, 3, 32, 33):
                want.append((f"colsum {dt} acc {acc} cv {cv}", _has(cs, lambda k, f: a(k) and f[3] == "vec" and k["C"] == cv * n and "lx" not in k)))
            want.append((f"colsum {dt} acc {acc} idle thread", _has(cs, lambda k, f: a(k) and f[0] * f[1] == 255)))
            want.append((f"colsum {dt} acc {acc} scalar 7", _has(cs, lambda k, f: a(k) and f[3] == "scalar" and k["C"] == 7)))
            want.append((f"colsum {dt} acc {acc} C 300", _has(cs, lambda k, f: a(k) and k["C"] == 300)))
            want.append((f"colsum {dt} acc {acc} scalar, ten channel tiles", _has(cs, lambda k, f: a(k) and f[3] == "scalar" and f[5] == 10)))
            for rows in (1, 127, 128, 129):
                want.append((f"colsum {dt} acc {acc} rows {rows}", _has(cs, lambda k, f: a(k) and k["rows"] == rows)))
            want.append((f"colsum {dt} acc {acc} 65535 rows", _has(cs, lambda k, f: a(k) and k["rows"] == 65535 and k["C"] == 8 and f[2] == 128)))
            want.append((f"colsum {dt} acc {acc} 65536 rows", _has(cs, lambda k, f: a(k) and k["rows"] == 65536 and k["C"] == 8 and f[2] == 512)))
            for lay, br in (("slice", "vec"), ("off8", "scalar"), ("ldodd", "scalar")):
                want.append((f"colsum {dt} acc {acc} {lay}", _has(cs, lambda k, f: a(k) and k.get("lx") == lay and f[3] == br)))
    want.append(("tn cap", _has(tn, lambda k, f: k["dt"] == "bf16" and (k["M"], k["N"], k["K"]) == (1024, 1024, 10240) and f[2] == 4 and S.cdiv(k["K"], 2048) == 5)))
    # the batched partial-tile sum
    for s in (1, 7, 8, 9, 32, 33, 64, 70):
        want.append((f"reduce splits {s}", _has(red, lambda k, f: (k["M"], k["N"], k["splits"]) == (16, 64, s) and "lc" not in k and "regroup" not in k)))
    for (M, N), t in (((1, 4), 1), ((3, 340), 255), ((16, 64), 256), ((1, 1028), 257)):
        want.append((f"reduce threads {t}", _has(red, lambda k, f: (k["M"], k["N"]) == (M, N) and f[0] == t)))
    for store, lays in (("rmw16", ("contig", "slice")), ("rmw1", ("ldodd", "off4"))):
        for lay in lays:
            want.append((f"reduce {store} {lay}", _has(red, lambda k, f: k.get("lc", "contig") == lay and f[2] == store)))
            want.append((f"reduce atomic {lay} at 33 splits", _has(red, lambda k, f: k.get("lc", "contig") == lay and f[2] == "atomic" and k["splits"] == 33)))
    want.append(("reduce short second group", _has(red, lambda k, f: f[1] == 2 and k["splits"] % 32 not in (0, 8, 16, 24))))
    want.append(("reduce unroll tail", _has(red, lambda k, f: f[1] == 1 and k["splits"] % 8 != 0 and k["splits"] > 8)))
    for s, store in ((9, "regroup-rmw"), (40, "regroup-atomic")):
        want.append((f"reduce regroup 8 at {s} splits", _has(red, lambda k, f: k.get("regroup") == 8 and k["N"] == 64 and k["splits"] == s and f[2] == store)))
    missing = [name for name, ids in want if not ids]
    assert not missing, missing


def test_the_full_launches_are_full_and_mixed():
    for dt in ("bf16", "f32"):
        g = S.tn_group(dt)
        assert len(g) == S.GEMM_GROUP
        assert g[0][2][7] == 1 and g[-1][2][7] == 1 and max(r[2][7] for r in g) > 1      # the first and the last problem: one workgroup each
        assert {r[2][4] for r in g} == {S.STORE, S.ADD, S.ATOMIC} and any(r[1].get("regroup") for r in g)
        assert {(r[2][5], r[2][6]) for r in g} >= {(1, 1), (0, 1), (1, 0), (0, 0)}
        b = S.colsum_batch_group(dt)
        assert len(b) == S.COLSUM_BATCH and {r[2][2] for r in b} == {"vec", "scalar"}
    assert len(S.REDUCE_BATCH) == S.TN_REDUCE_BATCH
    assert {r[2][2] for r in S.REDUCE_BATCH} == {"rmw16", "rmw1", "atomic", "regroup-rmw", "regroup-atomic"}


def test_every_integer_row_is_exact_in_fp32():
    """inputs and earlier content are integers of at most INT_MAX in magnitude (exact in bf16): every partial sum of every element stays an
    integer below 2^24, so fp32 adds them without rounding in any order - atomics included"""
    assert float(torch.tensor(float(S.INT_MAX), dtype=torch.bfloat16)) == S.INT_MAX
    worst = 0
    for fam, (rid, kw, _) in _all_rows():
        b = S.int_bound(fam, kw)
        assert b < 2 ** 24, (rid, b)
        worst = max(worst, b)
    for rid, _, descs in S.COLSUM_SHARED:
        assert sum(S.int_bound("colsum_batch", d) for d in descs) < 2 ** 24, rid
    assert worst == 98304 * 16 + 4


def test_references_agree_with_naive_loops():
    g = torch.Generator().manual_seed(5)
    for K, M, N, rg in ((5, 3, 4, 0), (7, 2, 6, 3), (1, 4, 8, 2)):
        a, b = torch.randn(K, M, generator=g), torch.randn(K, N, generator=g)
        got = R.regrouped(R.tn_product(a, b), rg)
        want = torch.tensor(R.naive_tn(a.tolist(), b.tolist(), rg), dtype=torch.float64)
        assert torch.allclose(got, want, rtol=1e-13, atol=1e-13), (K, M, N, rg)
        p = torch.randn(K, M, N, generator=g)
        assert torch.allclose(R.partial_sum(p), torch.tensor(R.naive_partial_sum(p.tolist()), dtype=torch.float64), rtol=1e-13, atol=1e-13)
        assert torch.allclose(R.colsum(a), torch.tensor(R.naive_colsum(a.tolist()), dtype=torch.float64), rtol=1e-13, atol=1e-13)
    # the index map by hand: N = 6, regroup 3 -> columns (j, c) = (0,0) (0,1) (0,2) (1,0) (1,1) (1,2) go to c * 2 + j
    assert R.regroup_index(6, 3).tolist() == [0, 2, 4, 1, 3, 5]
    x = torch.arange(6.0).view(1, 6)
    assert R.regrouped(x, 3).tolist() == [[0.0, 3.0, 1.0, 4.0, 2.0, 5.0]]
    before = torch.tensor([1.0, 2.0])
    assert R.accumulate(before, torch.tensor([0.5, 0.5], dtype=torch.float64)).tolist() == [1.5, 2.5]
    assert R.accumulate(before, torch.tensor([0.5, 0.5], dtype=torch.float64), keep=False).tolist() == [0.5, 0.5]


def test_launchers_refuse_bad_arguments_before_any_launch():
    """every call is wrong in exactly one way and must come back MISEG_E_BADARG with miseg_last_error set: the host checks run before
    anything is launched, so the stand-in addresses are never read and no device is needed"""
    from mi_seg_amd.hip import lib as L
    so = L.load()
    A = 1 << 20

    def refused(rc, what, word):
        assert rc == S.BADARG, (what, rc)
        msg = so.miseg_last_error().decode()
        assert word in msg, (what, msg)

    def tn(**kw):
        d = dict(A=A, lda=64, B=A, ldb=64, C=A, ldc=64, M=64, N=64, K=100, zeroed=0, regroup=0, pad_=0)
        d.update(kw)
        return L.GemmTnDesc(**d)

    def red(**kw):
        d = dict(partial=A, C=A, ldc=64, M=16, N=64, splits=9, block0=0, regroup=0, pad_=0)
        d.update(kw)
        return L.TnReduceDesc(**d)

    def csb(**kw):
        d = dict(x=A, ldx=64, rows=100, out=A, C=64, block0=0)
        d.update(kw)
        return L.ColsumDesc(**d)

    def cs(**kw):
        d = dict(x=A, ldx=64, rows=100, C=64, dtype=L.BF16, out=A, accumulate=1)
        d.update(kw)
        return L.Colsum(**d)

    def call(fn, T, items, *args):
        a = (T * len(items))(*items)      # alive until the call has returned
        return fn(C.addressof(a), *args)

    # the batch sizes: none, and one more than the kernel arguments hold
    for n in (0, S.GEMM_GROUP + 1):
        refused(call(so.miseg_gemm_tn_group, L.GemmTnDesc, [tn()] * (S.GEMM_GROUP + 1), n, L.BF16, None), f"tn_group n={n}", "gemm_tn_group")
    for n in (0, S.TN_REDUCE_BATCH + 1):
        refused(call(so.miseg_gemm_tn_reduce_batch, L.TnReduceDesc, [red()] * (S.TN_REDUCE_BATCH + 1), n, None), f"reduce n={n}", "gemm_tn_reduce_batch")
    for n in (0, S.COLSUM_BATCH + 1):
        refused(call(so.miseg_colsum_batch, L.ColsumDesc, [csb()] * (S.COLSUM_BATCH + 1), n, L.BF16, None), f"colsum_batch n={n}", "colsum_batch")
    assert (S.GEMM_GROUP, S.TN_REDUCE_BATCH, S.COLSUM_BATCH) == (24, 32, 32)
    refused(so.miseg_gemm_tn_group(None, 1, L.BF16, None), "tn_group NULL", "gemm_tn_group")
    refused(so.miseg_gemm_tn_reduce_batch(None, 1, None), "reduce NULL", "gemm_tn_reduce_batch")
    refused(so.miseg_colsum_batch(None, 1, L.BF16, None), "colsum_batch NULL", "colsum_batch")
    refused(so.miseg_colsum(None, None), "colsum NULL", "colsum")

    # one descriptor wrong, behind a good one (the index in the message is the bad one's)
    for kw in (dict(N=62), dict(splits=0), dict(regroup=7), dict(regroup=-1), dict(partial=None), dict(C=None), dict(M=0)):
        refused(call(so.miseg_gemm_tn_reduce_batch, L.TnReduceDesc, [red(), red(**kw)], 2, None), f"reduce {kw}", "descriptor 1")
    for kw in (dict(regroup=7), dict(regroup=-2), dict(A=None), dict(B=None), dict(C=None), dict(M=0), dict(N=0), dict(K=0)):
        refused(call(so.miseg_gemm_tn_group, L.GemmTnDesc, [tn(), tn(**kw)], 2, L.BF16, None), f"tn_group {kw}", "problem 1")
    for kw in (dict(x=None), dict(out=None), dict(rows=0), dict(C=0)):
        refused(call(so.miseg_colsum_batch, L.ColsumDesc, [csb(), csb(**kw)], 2, L.BF16, None), f"colsum_batch {kw}", "descriptor 1")
        refused(so.miseg_colsum(C.byref(cs(**kw)), None), f"colsum {kw}", "colsum")

    # a dtype that is neither bf16 nor fp32; the lone column sum refuses it before it clears `out` (accumulate 0)
    assert {L.F32, L.BF16} == {0, 1}
    for dt in (2, -1):
        refused(call(so.miseg_gemm_tn_group, L.GemmTnDesc, [tn()], 1, dt, None), f"tn_group dtype {dt}", "dtype")
        refused(call(so.miseg_colsum_batch, L.ColsumDesc, [csb()], 1, dt, None), f"colsum_batch dtype {dt}", "dtype")
        for acc in (1, 0):
            refused(so.miseg_colsum(C.byref(cs(dtype=dt, accumulate=acc)), None), f"colsum dtype {dt} accumulate {acc}", "dtype")
