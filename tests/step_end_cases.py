"""The table of the step-end reduction launches (tests/test_hip_step_end_forms.py launches every row, tests/test_step_end_cases_cpu.py pins the
table without a device): miseg_gemm_tn_group, miseg_gemm_tn_reduce_batch, miseg_colsum_batch and miseg_colsum - what StepQueues.flush of
hip/ops.py issues at the end of a training step.

A row is (id, keywords, form).  The form was worked out by hand from the launcher's text (csrc/gemm.hip, csrc/elementwise.hip) and the id spells
it; `tn_form`, `reduce_form`, `colsum_batch_form` and `colsum_form` restate the launchers' host arithmetic so that the CPU test can hold every
hand-written form to it.  These restatements are LABELS: the library exposes no plan for these four calls, so which form a launch took is not
observed on the card - a row shows that the result is right and the neighbouring bytes survive at the shape that is meant to reach the form.

Layouts are those of tests/layouts.py (restated in `layout`): `contig`, `slice` (aligned, ld != C, ld % N == 0), `off8` / `off4` / `off2` (the
base 8 / 4 / 2 bytes into a 16-byte unit), `ldodd` (aligned base, ld % N != 0).  dtype: "bf16" (8 elements per 16 bytes) or "f32" (4).  CPU only."""

NVEC = {"bf16": 8, "f32": 4}
ESIZE = {"bf16": 2, "f32": 4}
DTYPE_CODE = {"f32": 0, "bf16": 1}      # MISEG_F32 / MISEG_BF16 of include/miseg_hip.h
BADARG = -1
GEMM_GROUP, TN_REDUCE_BATCH, COLSUM_BATCH = 24, 32, 32      # MISEG_GEMM_GROUP, MISEG_TN_REDUCE_BATCH, MISEG_COLSUM_BATCH
STORE, ADD, ATOMIC = 0, 1, 2
MODE_NAME = {STORE: "store", ADD: "add", ATOMIC: "atomic"}
INT_MAX = 4             # |v| <= 4 in the exact-integer runs (exact in bf16)


def cdiv(a, b):
    return -(-a // b)


def layout(c, n, lay):
    """(offset in elements, ld) of a view of c columns in tests/layouts.py::Slot for a type with n elements per 16 bytes"""
    cp = cdiv(c, n) * n
    return {"contig": (0, c), "slice": (n, cp + 3 * n), "off8": (n // 2, cp + 2 * n), "ldodd": (0, cp + n + 1), "off4": (n // 4, cp + 2 * n),
            "off2": (n // 8, cp + 2 * n)}[lay]


def vec_ok(c, n, lay):
    """the launchers' operand predicate: 16-byte aligned base and ld % n == 0 (the column-sum kernels ask C % n == 0 too: see their forms)"""
    off, ld = layout(c, n, lay)
    return off % n == 0 and ld % n == 0


# ------------------------------------------------------------------------------------------------ miseg_gemm_tn_group
def tn_form(kw):
    """(gx, gy, split, kps, mode, va, vb, blocks) of one problem of miseg_gemm_tn_group: 64 x 64 tiles, 96-row (bf16) / 64-row (fp32) stages"""
    n, bk = NVEC[kw["dt"]], (96 if kw["dt"] == "bf16" else 64)
    M, N, K = kw["M"], kw["N"], kw["K"]
    gx, gy = cdiv(M, 64), cdiv(N, 64)
    split = min(cdiv(K, 2048), 1024 // (gx * gy))
    split = max(split, 1)
    kps = cdiv(cdiv(K, split), bk) * bk
    split = cdiv(K, kps)
    mode = ATOMIC if split > 1 else (STORE if kw.get("zeroed") else ADD)
    return (gx, gy, split, kps, mode, int(vec_ok(M, n, kw.get("la", "contig"))), int(vec_ok(N, n, kw.get("lb", "contig"))), gx * gy * split)


def tn_spell(f):
    gx, gy, split, kps, mode, va, vb, blocks = f
    return f"g{gx}x{gy}-s{split}-kps{kps}-{MODE_NAME[mode]}-{'v' if va else 's'}a-{'v' if vb else 's'}b-wg{blocks}"


def _tn(tag, dt, M, N, K, form, **kw):
    return (f"tn-{dt}-{tag}-m{M}-n{N}-k{K}-{tn_spell(form)}", dict(dt=dt, M=M, N=N, K=K, **kw), form)


def _tn_rows():
    rows = []
    for dt, off_small in (("bf16", "off2"), ("f32", "off4")):
        bk = 96 if dt == "bf16" else 64
        a64 = 1           # M = 64 / N = 64 contiguous: ld % n == 0
        # K edges, one split: below one MFMA step, one step, one short of a stage, a stage, one past it
        kedges = (1, 31, 32, 95, 96, 97) if dt == "bf16" else (1, 3, 5, 63, 64, 65)
        for i, K in enumerate(kedges):
            rows.append(_tn("kedge", dt, 64, 64, K, (1, 1, 1, bk if i < 5 else 2 * bk, ADD, a64, a64, 1), group=int(i not in (1, 3))))
        # the split path at M = N = 8: two splits with a short second, three, the count the rounded stage lowers (bf16: 48 -> 47)
        split_forms = {"bf16": ((2049, 2, 1056), (4100, 3, 1440), (98304, 47, 2112)), "f32": ((2049, 2, 1088), (4100, 3, 1408), (98304, 48, 2048))}[dt]
        for K, s, kps in split_forms:
            rows.append(_tn("split", dt, 8, 8, K, (1, 1, s, kps, ATOMIC, 1, 1, s), group=int(K != 98304)))
        rows.append(_tn("split-zeroed", dt, 8, 8, 2049, (1, 1, 2, split_forms[0][2], ATOMIC, 1, 1, 2), zeroed=1, group=1))
        # tile edges: M, N in 1, 7, 63, 64, 65, 100, each value on each side once
        kt = 2 * bk
        # (M, N, gx, gy, va / vb for bf16, va / vb for fp32): a contiguous operand is a vector operand when its width divides by 8 / 4
        for M, N, gx, gy, v8, v4 in ((1, 1, 1, 1, (0, 0), (0, 0)), (7, 100, 1, 2, (0, 0), (0, 1)), (63, 65, 1, 2, (0, 0), (0, 0)), (64, 7, 1, 1, (1, 0), (1, 0)),
                                     (65, 63, 2, 1, (0, 0), (0, 0)), (100, 64, 2, 1, (0, 1), (1, 1))):
            va, vb = v8 if dt == "bf16" else v4
            rows.append(_tn("tile", dt, M, N, 100, (gx, gy, 1, kt, ADD, va, vb, gx * gy), group=1))
        # operand layouts: A alone, B alone, C alone
        for lay in ("slice", "off8", "ldodd", off_small):
            v = int(lay == "slice")
            rows.append(_tn(f"a-{lay}", dt, 64, 64, 100, (1, 1, 1, kt, ADD, v, 1, 1), la=lay, group=int(lay != "slice")))
            rows.append(_tn(f"b-{lay}", dt, 64, 64, 100, (1, 1, 1, kt, ADD, 1, v, 1), lb=lay, group=int(lay != "slice")))
        for lay in ("slice", "off4"):
            rows.append(_tn(f"c-{lay}", dt, 64, 64, 100, (1, 1, 1, kt, ADD, 1, 1, 1), lc=lay, group=int(lay == "off4")))
            rows.append(_tn(f"c-{lay}-zeroed", dt, 64, 64, 100, (1, 1, 1, kt, STORE, 1, 1, 1), lc=lay, zeroed=1))
        # modes: a zero slot that is stored (16-byte and scalar stores)
        rows.append(_tn("zeroed", dt, 64, 64, 100, (1, 1, 1, kt, STORE, 1, 1, 1), zeroed=1, group=2))      # group=2: the last problem of the full launch
        rows.append(_tn("zeroed", dt, 65, 63, 100, (2, 1, 1, kt, STORE, 0, 0, 2), zeroed=1))
        # regroup: column j * regroup + c lands at c * (N / regroup) + j
        n = NVEC[dt]
        k2 = split_forms[0][2]
        rows.append(_tn("regroup9", dt, 64, 72, 100, (1, 2, 1, kt, ADD, 1, int(72 % n == 0), 2), regroup=9, group=1))
        rows.append(_tn("regroup9", dt, 64, 72, 2049, (1, 2, 2, k2, ATOMIC, 1, int(72 % n == 0), 4), regroup=9, group=1))
        rows.append(_tn("regroup8", dt, 33, 64, 100, (1, 1, 1, kt, ADD, 0, 1, 1), regroup=8))
        rows.append(_tn("regroup8-zeroed", dt, 33, 64, 100, (1, 1, 1, kt, STORE, 0, 1, 1), regroup=8, zeroed=1))
        rows.append(_tn("regroup8", dt, 33, 64, 2049, (1, 1, 2, k2, ATOMIC, 0, 1, 2), regroup=8, group=1))
    # the 1024 / (gx * gy) cap: 5 splits wanted, 4 allowed
    rows.append(_tn("cap", "bf16", 1024, 1024, 10240, (16, 16, 4, 2592, ATOMIC, 1, 1, 1024)))
    return rows


TN_ROWS = _tn_rows()


def tn_group(dt):
    """the 24 problems of the one full launch: rows marked `group`, ordered so that the first and the last are one workgroup each"""
    rows = [r for r in TN_ROWS if r[1]["dt"] == dt and r[1].get("group")]
    return [r for r in rows if r[1]["group"] == 1] + [r for r in rows if r[1]["group"] == 2]


# ------------------------------------------------------------------------------------------------ miseg_gemm_tn_reduce_batch
SPLIT_GROUP = 32      # TNB_SG: splits per thread group


def reduce_form(kw):
    """(threads per split group, split groups, store form) of one descriptor"""
    M, N, s = kw["M"], kw["N"], kw["splits"]
    groups = cdiv(s, SPLIT_GROUP)
    lay = kw.get("lc", "contig")
    off, ld = layout(N, 4, lay)
    if kw.get("regroup"):
        store = "regroup-rmw" if groups == 1 else "regroup-atomic"
    elif groups > 1:
        store = "atomic"
    else:
        store = "rmw16" if (off % 4 == 0 and ld % 4 == 0) else "rmw1"
    return (M * (N // 4), groups, store)


def reduce_spell(f):
    return f"t{f[0]}-g{f[1]}-{f[2]}"


def _red(tag, M, N, splits, form, **kw):
    return (f"reduce-{tag}-m{M}-n{N}-s{splits}-{reduce_spell(form)}", dict(M=M, N=N, splits=splits, **kw), form)


REDUCE_ROWS = [
    # splits: one, the eight-wide unroll's tail of seven, none, one; the 32 | 33 boundary; two whole groups; a short third
    _red("splits", 16, 64, 1, (256, 1, "rmw16")),
    _red("splits", 16, 64, 7, (256, 1, "rmw16")),
    _red("splits", 16, 64, 8, (256, 1, "rmw16")),
    _red("splits", 16, 64, 9, (256, 1, "rmw16")),
    _red("splits", 16, 64, 32, (256, 1, "rmw16")),
    _red("splits", 16, 64, 33, (256, 2, "atomic")),
    _red("splits", 16, 64, 40, (256, 2, "atomic")),
    _red("splits", 16, 64, 64, (256, 2, "atomic")),
    _red("splits", 16, 64, 65, (256, 3, "atomic")),
    _red("splits", 16, 64, 70, (256, 3, "atomic")),
    # thread counts: 1, 255, 257 (256 is the rows above)
    _red("threads", 1, 4, 9, (1, 1, "rmw16")),
    _red("threads", 1, 4, 33, (1, 2, "atomic")),
    _red("threads", 3, 340, 9, (255, 1, "rmw16")),
    _red("threads", 3, 340, 33, (255, 2, "atomic")),
    _red("threads", 1, 1028, 9, (257, 1, "rmw16")),
    _red("threads", 1, 1028, 33, (257, 2, "atomic")),
    _red("ragged", 5, 12, 8, (15, 1, "rmw16")),
    _red("ragged", 5, 12, 32, (15, 1, "rmw16")),
    _red("ragged", 5, 12, 33, (15, 2, "atomic")),
    _red("ragged", 5, 12, 64, (15, 2, "atomic")),
    # C: an aligned slice (16-byte read-modify-write at ld != N), ldc % 4 != 0 and a base 4 bytes off (scalar), each also with atomics
    _red("c-slice", 16, 64, 9, (256, 1, "rmw16"), lc="slice"),
    _red("c-slice", 16, 64, 33, (256, 2, "atomic"), lc="slice"),
    _red("c-ldodd", 16, 64, 9, (256, 1, "rmw1"), lc="ldodd"),
    _red("c-ldodd", 16, 64, 33, (256, 2, "atomic"), lc="ldodd"),
    _red("c-off4", 16, 64, 9, (256, 1, "rmw1"), lc="off4"),
    _red("c-off4", 16, 64, 33, (256, 2, "atomic"), lc="off4"),
    # the regrouped store
    _red("regroup8", 16, 64, 9, (256, 1, "regroup-rmw"), regroup=8),
    _red("regroup8", 16, 64, 40, (256, 2, "regroup-atomic"), regroup=8),
    _red("regroup8-c-slice", 16, 64, 9, (256, 1, "regroup-rmw"), regroup=8, lc="slice"),
    _red("regroup8-c-ldodd", 16, 64, 40, (256, 2, "regroup-atomic"), regroup=8, lc="ldodd"),
    _red("regroup9", 7, 72, 9, (126, 1, "regroup-rmw"), regroup=9),
    _red("regroup9", 7, 72, 40, (126, 2, "regroup-atomic"), regroup=9),
]
REDUCE_BATCH = REDUCE_ROWS      # the one full launch: all 32 rows as its 32 descriptors


# ------------------------------------------------------------------------------------------------ miseg_colsum_batch
def colsum_batch_form(kw):
    """(512-row chunks, 64-channel tiles, branch) of one descriptor"""
    n = NVEC[kw["dt"]]
    C = kw["C"]
    vec = C % n == 0 and vec_ok(C, n, kw.get("lx", "contig"))
    return (cdiv(kw["rows"], 512), cdiv(C, 64), "vec" if vec else "scalar")


def colsum_batch_spell(f):
    return f"{f[0]}x{f[1]}-{f[2]}"


def _csb(tag, dt, rows, C, form, **kw):
    return (f"colsumb-{dt}-{tag}-r{rows}-c{C}-{colsum_batch_spell(form)}", dict(dt=dt, rows=rows, C=C, **kw), form)


def _csb_rows():
    out = []
    for dt, small in (("bf16", "off2"), ("f32", "off4")):
        n = NVEC[dt]
        # vector branch: rows below TY, one chunk exactly, one row past it, a ragged second chunk (the clamped re-read)
        for rows, chunks in ((1, 1), (31, 1), (512, 1), (513, 2), (767, 2), (1024, 2), (1025, 3), (1536, 3)):
            out.append(_csb("vec", dt, rows, 64, (chunks, 1, "vec")))
        out.append(_csb("one-vector", dt, 1, n, (1, 1, "vec")))
        out.append(_csb("one-vector", dt, 513, n, (2, 1, "vec")))
        out.append(_csb("second-tile-one-vector", dt, 513, 64 + n, (2, 2, "vec")))
        for rows, chunks in ((1, 1), (31, 1), (512, 1), (767, 2)):
            out.append(_csb("three-tiles", dt, rows, 136, (chunks, 3, "vec")))
        out.append(_csb("x-slice", dt, 513, 64, (2, 1, "vec"), lx="slice"))
        out.append(_csb("x-slice", dt, 1025, 136, (3, 3, "vec"), lx="slice"))
        # scalar branch: C % n != 0 ...
        for rows, chunks in ((1, 1), (3, 1), (513, 2)):
            for C, tiles in ((7, 1), (65, 2), (100, 2)):
                br = "vec" if (C == 100 and dt == "f32") else "scalar"      # 100 divides by four: fp32 takes the vector branch there
                out.append(_csb("c-ragged", dt, rows, C, (chunks, tiles, br)))
        # ... or one clause of the vector predicate broken alone
        for lay in ("off8", "ldodd", small):
            out.append(_csb(f"x-{lay}", dt, 513, 64, (2, 1, "scalar"), lx=lay))
            out.append(_csb(f"x-{lay}", dt, 31, 64 + n, (1, 2, "scalar"), lx=lay))
    return out


COLSUM_BATCH_ROWS = _csb_rows()


def colsum_batch_group(dt):
    """the 32 descriptors of the one full launch: the first 32 rows of the dtype (both branches among them)"""
    return [r for r in COLSUM_BATCH_ROWS if r[1]["dt"] == dt][:COLSUM_BATCH]


# two descriptors that add into the same `out`: (id, dtype, the two descriptors' keywords)
COLSUM_SHARED = [
    ("colsumb-bf16-shared-out-vec-and-scalar", "bf16", (dict(dt="bf16", rows=513, C=64), dict(dt="bf16", rows=3, C=64, lx="ldodd"))),
    ("colsumb-f32-shared-out-vec-and-scalar", "f32", (dict(dt="f32", rows=767, C=68), dict(dt="f32", rows=513, C=68, lx="off8"))),
    ("colsumb-bf16-shared-out-two-scalar", "bf16", (dict(dt="bf16", rows=513, C=7), dict(dt="bf16", rows=1, C=7))),
]


# ------------------------------------------------------------------------------------------------ miseg_colsum
def colsum_form(kw):
    """(tx, ty, rows per block, branch, grid x, grid y) of the lone column sum"""
    n = NVEC[kw["dt"]]
    C, rows = kw["C"], kw["rows"]
    vec = C % n == 0 and vec_ok(C, n, kw.get("lx", "contig"))
    cv = C // n if vec else C
    tx = min(cv, 32)
    ty = 256 // tx
    rpb = 512 if rows >= 65536 else 128
    return (tx, ty, rpb, "vec" if vec else "scalar", cdiv(rows, rpb), cdiv(cv, tx))


def colsum_spell(f):
    return f"tx{f[0]}-ty{f[1]}-rpb{f[2]}-{f[3]}-g{f[4]}x{f[5]}"


def _cs(tag, dt, rows, C, form, **kw):
    out = []
    for acc in (0, 1):
        out.append((f"colsum-{dt}-{tag}-r{rows}-c{C}-acc{acc}-{colsum_spell(form)}", dict(dt=dt, rows=rows, C=C, accumulate=acc, **kw), form))
    return out


def _cs_rows():
    out = []
    for dt in ("bf16", "f32"):
        n = NVEC[dt]
        # vector: cv = 1, 3 (85 row lanes and one idle thread), 32, 33 (a second channel tile of one vector)
        for cv, tx, ty, gy in ((1, 1, 256, 1), (3, 3, 85, 1), (32, 32, 8, 1), (33, 32, 8, 2)):
            out += _cs(f"cv{cv}", dt, 129, cv * n, (tx, ty, 128, "vec", 2, gy))
        # scalar
        out += _cs("scalar", dt, 129, 7, (7, 36, 128, "scalar", 2, 1))
        if dt == "bf16":
            out += _cs("scalar", dt, 129, 300, (32, 8, 128, "scalar", 2, 10))
        else:      # 300 is four-divisible: fp32 takes the vector kernel at cv = 75; 301 is its scalar row
            out += _cs("cv75", dt, 129, 300, (32, 8, 128, "vec", 2, 3))
            out += _cs("scalar", dt, 129, 301, (32, 8, 128, "scalar", 2, 10))
        # rows around one block
        for rows in (1, 127, 128):
            out += _cs("cv3", dt, rows, 3 * n, (3, 85, 128, "vec", 1, 1))
            out += _cs("scalar", dt, rows, 7, (7, 36, 128, "scalar", 1, 1))
        # the 128- to 512-row block switch
        t8 = 8 // n
        out += _cs("below-switch", dt, 65535, 8, (t8, 256 // t8, 128, "vec", 512, 1))
        out += _cs("at-switch", dt, 65536, 8, (t8, 256 // t8, 512, "vec", 128, 1))
        # operand layouts
        out += _cs("x-slice", dt, 129, 3 * n, (3, 85, 128, "vec", 2, 1), lx="slice")
        stx, sty = {"bf16": (24, 10), "f32": (12, 21)}[dt]      # the scalar kernel on the same 24 / 12 channels: a lane per channel
        out += _cs("x-off8", dt, 129, 3 * n, (stx, sty, 128, "scalar", 2, 1), lx="off8")
        out += _cs("x-ldodd", dt, 129, 3 * n, (stx, sty, 128, "scalar", 2, 1), lx="ldodd")
    return out


COLSUM_ROWS = _cs_rows()

FAMILIES = (("tn", TN_ROWS, tn_form, tn_spell), ("reduce", REDUCE_ROWS, reduce_form, reduce_spell),
            ("colsum_batch", COLSUM_BATCH_ROWS, colsum_batch_form, colsum_batch_spell), ("colsum", COLSUM_ROWS, colsum_form, colsum_spell))


def int_bound(family, kw):
    """the largest |sum| an element of the exact-integer run can reach: inputs and the slot's earlier content hold integers of at most INT_MAX"""
    terms = {"tn": lambda: kw["K"] * INT_MAX * INT_MAX, "reduce": lambda: kw["splits"] * INT_MAX, "colsum_batch": lambda: kw["rows"] * INT_MAX,
             "colsum": lambda: kw["rows"] * INT_MAX}[family]()
    return terms + INT_MAX
