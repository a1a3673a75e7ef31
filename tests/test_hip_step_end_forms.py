"""Launch forms, edges and operand layouts of the step-end reductions - what StepQueues.flush (hip/ops.py) issues when a training step ends: every
bias gradient of the network and every weight gradient that does not go through the lone miseg_gemm or the conv weight-gradient kernels.
  miseg_gemm_tn_group          gemm_tn_group_kernel<bf16 | float> over gemm_tn_body<T, float, 96> (csrc/gemm.hip): up to 24 TN products, 64 x 64 tiles
  miseg_gemm_tn_reduce_batch   gemm_tn_reduce_batch_kernel (csrc/gemm.hip): up to 32 deferred partial-tile sums, groups of 32 splits, eight loads in flight
  miseg_colsum_batch           colsum_batch_kernel<T> (csrc/elementwise.hip): up to 32 column sums, 512-row chunks x 64-channel tiles, vector and scalar branch
  miseg_colsum                 colsum_kernel<T, VEC>: tx x ty threads, 128- or 512-row blocks

The rows are those of tests/step_end_cases.py, which tests/test_step_end_cases_cpu.py pins on the host (every form of the list below has a row; the
hand-written form of every row equals the restated launcher arithmetic and what the id spells).  Every row goes through the C entry point with its
ctypes struct (L.GemmTnDesc, L.TnReduceDesc, L.ColsumDesc, L.Colsum), not through `ops`.  The library has no plan for these calls: which form ran is
not observed; the rows show that the result is right and the neighbouring bytes survive at the shape that is meant to reach the form.  Form -> rows:
  `tn-<dt>-kedge-*`         K = 1, 31, 32, 95, 96, 97 (bf16, 96-row stage) / 1, 3, 5, 63, 64, 65 (fp32, 64-row stage, MFMA k = 4) at M = N = 64, unsplit
  `tn-<dt>-split*-*`        M = N = 8: K = 2049 (two splits, the second short; onto content and `-zeroed` onto zeros), 4100 (three), 98304 (bf16: the
                            rounded stage lowers 48 splits to 47; fp32: 48); `tn-bf16-cap-*` 1024 x 1024 x 10240: five splits wanted, 1024 / 256 = 4 allowed
  `tn-<dt>-tile-*`          (M, N) = (1, 1), (7, 100), (63, 65), (64, 7), (65, 63), (100, 64): va / vb follow the width of the contiguous operand
  `tn-<dt>-a-<lay>` `-b-`   A alone / B alone as slice (vector, ld != width), off8, ldodd, off2 (bf16) / off4 (fp32): va / vb false;  `-c-slice`, `-c-off4`
                            (scalar store), each adding and `-zeroed` (storing);  `-zeroed-*` the store mode with 16-byte (64 x 64) and scalar (65 x 63) stores
  `tn-<dt>-regroup9-*` `-regroup8-*`   N = 72 / regroup 9 at M = 64 and N = 64 / regroup 8 at the ragged M = 33, unsplit (add; regroup 8 also store) and split
  `reduce-splits-*`         1, 7, 8, 9, 32 | 33, 40, 64, 65, 70 splits at 16 x 64: the unroll's tail, the read-modify-write | atomics boundary, a second group of
                            one split, of eight, a whole one, a third of one and of six;  `reduce-threads-*` M * N / 4 = 1, 255, 257 (256: the rows before) at 9
                            and 33 splits;  `reduce-ragged-*` 15 threads;  `reduce-c-<slice|ldodd|off4>-*` the 16-byte read-modify-write at ld != N, the
                            scalar one (ldc % 4 != 0; base 4 bytes off), each also at 33 splits (atomics);  `reduce-regroup8*` / `-regroup9-*` with 9 and 40 splits
  `colsumb-<dt>-vec-*`      C = 64 with 1, 31, 512, 513, 767, 1024, 1025, 1536 rows;  `-one-vector-` C = 8 / 4;  `-second-tile-one-vector-` C = 72 / 68;
                            `-three-tiles-` C = 136;  `-x-slice-`;  scalar branch: `-c-ragged-` C = 7, 65, 100 x rows 1, 3, 513 (fp32 takes the vector branch
                            at C = 100), `-x-<off8|ldodd|off2|off4>-` C = 64 (and 72 / 68 on 31 rows): each clause of the vector predicate broken alone;
                            `colsumb-*-shared-out-*`: two descriptors that add into one `out`
  `colsum-<dt>-cv<1|3|32|33>-*`  the vector kernel (cv = 3: 3 x 85 threads, one idle);  `-scalar-` C = 7 and 300 (fp32: 301; its C = 300 is `-cv75-`);  rows 1, 127,
                            128, 129;  `-below-switch-` / `-at-switch-` 65535 | 65536 rows at C = 8;  `-x-slice-`, `-x-off8-`, `-x-ldodd-`;  every row with
                            accumulate 0 (the earlier content of `out` must be gone) and 1
and one launch of 24 problems per dtype (the first and the last one workgroup each, split and regrouped ones between them), one of all 32 reduce rows and one of
32 column sums per dtype (both branches), each compared per descriptor with the same descriptor launched alone: bit-equal where an element has one
writer, by parity otherwise.

Operands: inputs from tests/layouts.py::place_in in the row's layout (NaN all around: a read outside the view poisons the result); the partial tiles are
exactly splits * M * N floats between NaN and must come back unwritten; C from place_out (every byte beside the view must survive), a contiguous C and
every `out` between two runs of sentinels.  Outputs start from random content (`zeroed` rows: from zeros, the contract of the flag).  Two runs per row:
  integers   |v| <= 4 in the inputs and in the earlier content: every sum is an integer below 2^24 (98304 * 16 + 4 at the most), exact in fp32 in any
             order, so EVERY row - the atomic ones too - must equal the float64 reference bit for bit.  This run catches a lost or doubled row.
  floats     randn, judged by tests/parity.py::assert_parity, pooled and per element, at the bars the older tests hold these calls to: 1e-5 for the grouped
             TN product and the column sums (tests/test_hip_kernels.py), 2e-6 for the partial-tile sum (fp32 additions only).  Outputs are fp32 and bf16
             operands are exact in fp32.  The local_tol rule of DESIGN.md section 3 is wired in (beyond the per-element bar: at most twice the local error of
             the same sum done by torch in fp32 against the same float64 reference) and counted.  Rows with one writer per element launch twice and repeat
             bit for bit; atomic rows are judged by parity both times.
References: tests/step_end_ref.py (A.double().T @ B.double(), an explicit index map for `regroup`, .double().sum, before + term for the accumulate modes).

Measured on an MI355X, worst over all rows and both launches, pooled / per element (the last test prints this table; no row needed the local_tol rule):
  grouped TN product    3.1e-7 / 1.7e-6   (bar 1e-5; 142 arrays)        partial-tile sum   1.7e-7 / 2.1e-7   (bar 2e-6; 96)
  batched column sums   2.3e-7 / 4.3e-7   (bar 1e-5; 195)              lone column sum    5.9e-7 / 5.8e-7   (bar 1e-5; 116)
Wall time of the file run alone: 1.7 s for its 246 cases (the slowest, 0.9 s, is the first launch of the process); all 246 are green inside
the whole suite too.

What the rows exposed: no wrong number, no overwritten sentinel, no NaN, no differing bit on the four kernels.  One defect in a launcher, found by the
refusal test on the host: miseg_colsum with accumulate 0 cleared `out` BEFORE it refused an unknown dtype (the fill ran ahead of the dtype dispatch), so
a refused call had already written; the dtype is now checked first.

That the file can fail - eight mutations of gemm.hip / elementwise.hip, each built from a copy outside the repository and run once; all only do less or
permute inside the view (no access is widened, no launch geometry changed).  Red here / red among the older tests of the same calls
(tests/test_hip_kernels.py, test_hip_row_op_edges.py, test_hip_tn_stream_group.py, test_hip_gemm_forms.py):
  1. colsum_batch adds the clamped in-flight rows (`keep = 1`): 33 - every vector row but those of 512, 1024, 1536 rows (whole trips of 8 x TY), the fp32
     C = 100 rows, two `shared-out` cases, both full launches / old: NONE;
  2. the colsum_batch scalar branch skips its last row lane: 21 - every scalar row of 4 rows or more (the 1- and 3-row ones never reach lane 3), two
     `shared-out` cases, both full launches / old: NONE;
  3. the partial-tile sum drops the tail loop behind its eight-wide unroll: 23 - the 22 reduce rows with splits % 32 % 8 != 0 in a group and the full launch
     / old: 8 (three `bias_gradient` and one `transposed_conv_regrouping` case of test_hip_kernels.py, four of test_hip_tn_stream_group.py);
  4. its second split group returns early: 17 - the 16 rows with more than 32 splits and the full launch / old: 4 (the tallest streaming shapes);
  5. grouped TN workgroups with bz >= 1 return early: 15 - the eight `-split-` rows, the four split `-regroup*-` rows, `tn-bf16-cap-*`, both full
     launches / old: 3 (ops.gemm_tn sends its lone tall fallback products through the same launcher: K = 4096, 13824, 110592);
  6. the `regroup` column map of gemm_tn_body replaced by its inverse (stays inside the view): 6 - the four `-regroup9-` rows at N = 72 and both full
     launches; at N = 64 / regroup 8 the map is its own inverse and no row can see it / old: 8 (`transposed_conv_regrouping`);
  7. the same in the partial-tile sum: 3 - `reduce-regroup9-*` at 9 and 40 splits and the full launch; the N = 64 / regroup 8 rows stay green for the
     reason above, which is why the reduce table has N = 72 / regroup 9 rows beside them / old: 4;
  8. the lone colsum's last ty lane skipped: 56 - every `colsum-*` row whose last lane has a row to read (not the 1-row ones; at cv = 1, 256 row
     lanes, only the 512-row blocks of `-at-switch-` reach lane 255) / old: 36 (test_colsum_layouts of test_hip_row_op_edges.py).
What the older tests did not observe: the batched column sums at all beyond one aligned bf16 shape of whole chunks (mutations 1, 2), the grouped launch's
split path on purpose (5 is seen only through the lone fallback), and writes beside C and `out`."""
import ctypes as C
import time

import pytest
import torch

import step_end_cases as S
import step_end_ref as R
from layouts import SENT, _bits, assert_untouched, place_in, place_out
from parity import assert_parity, local_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
TOL = {"tn": 1e-5, "reduce": 2e-6, "colsum_batch": 1e-5, "colsum": 1e-5}
GUARD = 64
WORST = {}             # family -> [pooled, local, judgements by the local_tol rule, arrays judged]
SLOWEST = [0.0, ""]
T0 = [None]


def _L():
    from mi_seg_amd.hip import lib
    return lib


def _seed(rid, salt):
    return (sum((i + 1) * ord(ch) for i, ch in enumerate(rid)) * 31 + salt) % (2 ** 31)


def values(shape, dtype, ints, seed):
    """random floats, or integers in [-INT_MAX, INT_MAX] (exact in bf16; every sum of them is exact in fp32)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    if ints:
        return torch.randint(-S.INT_MAX, S.INT_MAX + 1, shape, generator=g, device=DEV).to(dtype)
    return torch.randn(*shape, generator=g, device=DEV).to(dtype)


class Guarded:
    """n fp32 elements between two runs of GUARD fill values: sentinels around an output, NaN around an input"""

    def __init__(self, n, fill=SENT):
        self.buf = torch.full((GUARD + n + GUARD,), fill, dtype=torch.float32, device=DEV)
        self.t = self.buf[GUARD:GUARD + n]
        assert self.t.data_ptr() % 16 == 0

    def check(self, what):
        g = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]])
        assert bool((g == SENT).all()), f"{what}: a sentinel beside the buffer was overwritten"


class OutSlot:
    """an fp32 [M][N] output: tests/layouts.py::place_out for the non-contiguous layouts, a contiguous one between two runs of sentinels"""

    def __init__(self, shape, lay):
        self.slot = place_out(shape, torch.float32, lay) if lay != "contig" else None
        self.guarded = Guarded(shape[0] * shape[1]) if lay == "contig" else None
        self.view = self.slot.view if self.slot is not None else self.guarded.t.view(*shape)

    def check(self, what):
        assert_untouched(self.slot, what) if self.slot is not None else self.guarded.check(what)


def addr(t):
    return int(t.data_ptr())


def same_bits(a, b, what):
    assert torch.equal(_bits(a.contiguous()), _bits(b.contiguous())), what


def parity(fam, what, got, ref, compose):
    """assert_parity at the family's bar; an honest result beyond the per-element bound is judged at twice the local error of the same sum done by
    torch in fp32 (`compose`) against the same float64 reference - the local_tol rule of DESIGN.md section 3 - and counted"""
    tol = TOL[fam]
    try:
        pooled, loc = assert_parity(got, ref, tol, what)
        rule = False
    except AssertionError:
        lt = max(tol, 2 * local_err(compose().double(), ref)[0])
        pooled, loc = assert_parity(got, ref, tol, what, local_tol=lt)
        rule = True
    print(f"PARITY {what}: pooled {pooled:.3e} local {loc:.3e}{' (local_tol rule)' if rule else ''}")
    w = WORST.setdefault(fam, [0.0, 0.0, 0, 0])
    w[0], w[1], w[2], w[3] = max(w[0], pooled), max(w[1], loc), w[2] + int(rule), w[3] + 1


def exact(what, got, ref):
    """the integer run: every sum is an integer below 2^24, so the fp32 result equals the float64 reference bit for bit in any order of adding"""
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    bad = got.double() != ref
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} element(s) of the exact-integer run differ, first at {tuple(bad.nonzero()[0].tolist())}: "
                                 f"got {float(got[tuple(bad.nonzero()[0].tolist())])}, reference {float(ref[tuple(bad.nonzero()[0].tolist())])}")


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def launch(name, *args):
    rc = getattr(_L().load(), name)(*args)
    assert rc == 0, (name, rc, _L().load().miseg_last_error().decode())


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


def _check_view(rid, view, c, n, lay):
    off, ld = S.layout(c, n, lay)
    assert view.stride(-2) == ld and view.data_ptr() % 16 == (off * view.element_size()) % 16, (rid, lay, view.stride(), ld)


# ------------------------------------------------------------------------------------------------ miseg_gemm_tn_group
class TnProblem:
    def __init__(self, row, ints):
        self.rid, kw, self.form = row
        self.kw, self.ints = kw, ints
        dt, n = TD[kw["dt"]], S.NVEC[kw["dt"]]
        M, N, K = kw["M"], kw["N"], kw["K"]
        self.av, self.bv = values((K, M), dt, ints, _seed(self.rid, 1)), values((K, N), dt, ints, _seed(self.rid, 2))
        self.a, self.b = place_in(self.av, kw.get("la", "contig")), place_in(self.bv, kw.get("lb", "contig"))
        _check_view(self.rid, self.a, M, n, kw.get("la", "contig"))
        _check_view(self.rid, self.b, N, n, kw.get("lb", "contig"))
        self.c = OutSlot((M, N), kw.get("lc", "contig"))
        _check_view(self.rid, self.c.view, N, 4, kw.get("lc", "contig"))
        # zeroed: the slot is known to hold zeros (the contract of the flag); otherwise it holds earlier content
        self.c0 = torch.zeros(M, N, device=DEV) if kw.get("zeroed") else values((M, N), torch.float32, ints, _seed(self.rid, 3))
        self.single_writer = self.form[2] == 1
        self._ref = None

    def desc(self):
        kw = self.kw
        return _L().GemmTnDesc(A=addr(self.a), lda=self.a.stride(0), B=addr(self.b), ldb=self.b.stride(0), C=addr(self.c.view), ldc=self.c.view.stride(0),
                               M=kw["M"], N=kw["N"], K=kw["K"], zeroed=kw.get("zeroed", 0), regroup=kw.get("regroup", 0), pad_=0)

    def reset(self):
        self.c.view.copy_(self.c0)

    def result(self):
        self.c.check(f"{self.rid} C")
        return self.c.view.clone()

    def ref(self):
        if self._ref is None:
            self._ref = R.accumulate(self.c0, R.regrouped(R.tn_product(self.av, self.bv), self.kw.get("regroup", 0)))
        return self._ref

    def compose(self):
        return self.c0 + R.regrouped(self.av.float().t() @ self.bv.float(), self.kw.get("regroup", 0))


def run_tn(problems):
    """one launch of the problems in this order; returns each problem's C"""
    L = _L()
    dt = problems[0].kw["dt"]
    assert all(p.kw["dt"] == dt for p in problems)
    for p in problems:
        p.reset()
    descs = (L.GemmTnDesc * len(problems))(*[p.desc() for p in problems])
    launch("miseg_gemm_tn_group", C.addressof(descs), len(problems), S.DTYPE_CODE[dt], stream())
    return [p.result() for p in problems]


@pytest.mark.parametrize("row", S.TN_ROWS, ids=lambda r: r[0])
def test_tn_group_row(row):
    for ints in (True, False):
        p = TnProblem(row, ints)
        got = run_tn([p])[0]
        if ints:
            exact(p.rid + " C (integers)", got, p.ref())
            continue
        parity("tn", p.rid + " C", got, p.ref(), p.compose)
        again = run_tn([p])[0]
        if p.single_writer:
            same_bits(got, again, p.rid + ": two launches with one writer per element differ")
        else:
            parity("tn", p.rid + " C, second launch", again, p.ref(), p.compose)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_tn_group_full_launch_equals_its_problems_alone(dt):
    """24 problems in one launch (the first and the last one workgroup each, split ones between them): every problem finds its own
    descriptor through block0 and computes what it computes alone"""
    rows = S.tn_group(dt)
    assert len(rows) == S.GEMM_GROUP
    for ints in (True, False):
        ps = [TnProblem(r, ints) for r in rows]
        together = run_tn(ps)
        for p, got in zip(ps, together):
            if ints:
                exact(p.rid + " C in the full launch (integers)", got, p.ref())
                continue
            parity("tn", p.rid + " C in the full launch", got, p.ref(), p.compose)
            alone = run_tn([p])[0]
            if p.single_writer:
                same_bits(got, alone, p.rid + ": the full launch and the problem alone differ")
            else:
                parity("tn", p.rid + " C alone", alone, p.ref(), p.compose)


# ------------------------------------------------------------------------------------------------ miseg_gemm_tn_reduce_batch
class ReduceProblem:
    def __init__(self, row, ints):
        self.rid, kw, self.form = row
        self.kw, self.ints = kw, ints
        M, N, s = kw["M"], kw["N"], kw["splits"]
        self.pbuf = Guarded(s * M * N, fill=float("nan"))      # exactly splits * M * N floats, NaN all around
        self.pv = values((s, M, N), torch.float32, ints, _seed(self.rid, 1))
        self.pbuf.t.copy_(self.pv.reshape(-1))
        self.c = OutSlot((M, N), kw.get("lc", "contig"))
        _check_view(self.rid, self.c.view, N, 4, kw.get("lc", "contig"))
        self.c0 = values((M, N), torch.float32, ints, _seed(self.rid, 3))
        self.single_writer = self.form[1] == 1
        self._ref = None

    def desc(self):
        kw = self.kw
        return _L().TnReduceDesc(partial=addr(self.pbuf.t), C=addr(self.c.view), ldc=self.c.view.stride(0), M=kw["M"], N=kw["N"], splits=kw["splits"], block0=0,
                                 regroup=kw.get("regroup", 0), pad_=0)

    def reset(self):
        self.c.view.copy_(self.c0)

    def result(self):
        self.c.check(f"{self.rid} C")
        same_bits(self.pbuf.t, self.pv.reshape(-1), f"{self.rid}: the partial tiles were written")
        return self.c.view.clone()

    def ref(self):
        if self._ref is None:
            self._ref = R.accumulate(self.c0, R.regrouped(R.partial_sum(self.pv), self.kw.get("regroup", 0)))
        return self._ref

    def compose(self):
        return self.c0 + R.regrouped(self.pv.sum(0), self.kw.get("regroup", 0))


def run_reduce(problems):
    L = _L()
    for p in problems:
        p.reset()
    descs = (L.TnReduceDesc * len(problems))(*[p.desc() for p in problems])
    launch("miseg_gemm_tn_reduce_batch", C.addressof(descs), len(problems), stream())
    return [p.result() for p in problems]


@pytest.mark.parametrize("row", S.REDUCE_ROWS, ids=lambda r: r[0])
def test_tn_reduce_batch_row(row):
    for ints in (True, False):
        p = ReduceProblem(row, ints)
        got = run_reduce([p])[0]
        if ints:
            exact(p.rid + " C (integers)", got, p.ref())
            continue
        parity("reduce", p.rid + " C", got, p.ref(), p.compose)
        again = run_reduce([p])[0]
        if p.single_writer:
            same_bits(got, again, p.rid + ": two launches with one writer per element differ")
        else:
            parity("reduce", p.rid + " C, second launch", again, p.ref(), p.compose)


def test_tn_reduce_batch_full_launch_equals_its_descriptors_alone():
    """32 descriptors in one launch: every store form, one to three split groups, one and two workgroups per group"""
    assert len(S.REDUCE_BATCH) == S.TN_REDUCE_BATCH
    for ints in (True, False):
        ps = [ReduceProblem(r, ints) for r in S.REDUCE_BATCH]
        together = run_reduce(ps)
        for p, got in zip(ps, together):
            if ints:
                exact(p.rid + " C in the full launch (integers)", got, p.ref())
                continue
            parity("reduce", p.rid + " C in the full launch", got, p.ref(), p.compose)
            alone = run_reduce([p])[0]
            if p.single_writer:
                same_bits(got, alone, p.rid + ": the full launch and the descriptor alone differ")
            else:
                parity("reduce", p.rid + " C alone", alone, p.ref(), p.compose)


# ------------------------------------------------------------------------------------------------ miseg_colsum_batch, miseg_colsum
class ColsumProblem:
    """one column sum: x in the row's layout inside NaN, `out` (C floats) between sentinels, holding earlier content"""

    def __init__(self, rid, kw, ints, out=None, salt=0):
        self.rid, self.kw, self.ints = rid, kw, ints
        dt, n = TD[kw["dt"]], S.NVEC[kw["dt"]]
        rows, Cc = kw["rows"], kw["C"]
        self.xv = values((rows, Cc), dt, ints, _seed(rid, 1 + salt))
        self.x = place_in(self.xv, kw.get("lx", "contig"))
        _check_view(rid, self.x, Cc, n, kw.get("lx", "contig"))
        self.out = out if out is not None else Guarded(Cc)
        self.o0 = values((Cc,), torch.float32, ints, _seed(rid, 3))
        self._sum = None

    def desc(self):
        return _L().ColsumDesc(x=addr(self.x), ldx=self.x.stride(0), rows=self.kw["rows"], out=addr(self.out.t), C=self.kw["C"], block0=0)

    def params(self):
        return _L().Colsum(x=addr(self.x), ldx=self.x.stride(0), rows=self.kw["rows"], C=self.kw["C"], dtype=S.DTYPE_CODE[self.kw["dt"]], out=addr(self.out.t),
                           accumulate=self.kw["accumulate"])

    def reset(self):
        self.out.t.copy_(self.o0)

    def result(self):
        self.out.check(self.rid + " out")
        return self.out.t.clone()

    def sum(self):
        if self._sum is None:
            self._sum = R.colsum(self.xv)
        return self._sum

    def ref(self, keep=True):
        return R.accumulate(self.o0, self.sum(), keep)

    def compose(self, keep=True):
        s = self.xv.float().sum(0)
        return self.o0 + s if keep else s


def run_colsum_batch(problems):
    L = _L()
    dt = problems[0].kw["dt"]
    assert all(p.kw["dt"] == dt for p in problems)
    for p in problems:
        p.reset()
    descs = (L.ColsumDesc * len(problems))(*[p.desc() for p in problems])
    launch("miseg_colsum_batch", C.addressof(descs), len(problems), S.DTYPE_CODE[dt], stream())
    return [p.result() for p in problems]


@pytest.mark.parametrize("row", S.COLSUM_BATCH_ROWS, ids=lambda r: r[0])
def test_colsum_batch_row(row):
    rid, kw, form = row
    for ints in (True, False):
        p = ColsumProblem(rid, kw, ints)
        got = run_colsum_batch([p])[0]
        if ints:
            exact(rid + " out (integers)", got, p.ref())
            continue
        parity("colsum_batch", rid + " out", got, p.ref(), p.compose)
        again = run_colsum_batch([p])[0]
        if form[0] == 1:      # one chunk: one workgroup, one atomic, per channel
            same_bits(got, again, rid + ": two launches with one writer per element differ")
        else:
            parity("colsum_batch", rid + " out, second launch", again, p.ref(), p.compose)


@pytest.mark.parametrize("case", S.COLSUM_SHARED, ids=lambda c: c[0])
def test_colsum_batch_two_descriptors_add_into_one_out(case):
    rid, dt, (ka, kb) = case
    for ints in (True, False):
        pa = ColsumProblem(rid, ka, ints, salt=10)
        pb = ColsumProblem(rid, kb, ints, out=pa.out, salt=20)      # the same slot, the same earlier content
        got = run_colsum_batch([pa, pb])[1]
        ref = pa.ref() + pb.sum()
        if ints:
            exact(rid + " out (integers)", got, ref)
        else:
            parity("colsum_batch", rid + " out", got, ref, lambda: pa.compose() + pb.xv.float().sum(0))


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_colsum_batch_full_launch_equals_its_descriptors_alone(dt):
    """32 descriptors of both branches in one launch"""
    rows = S.colsum_batch_group(dt)
    assert len(rows) == S.COLSUM_BATCH
    for ints in (True, False):
        ps = [ColsumProblem(r[0], r[1], ints) for r in rows]
        together = run_colsum_batch(ps)
        for r, p, got in zip(rows, ps, together):
            if ints:
                exact(p.rid + " out in the full launch (integers)", got, p.ref())
                continue
            parity("colsum_batch", p.rid + " out in the full launch", got, p.ref(), p.compose)
            alone = run_colsum_batch([p])[0]
            if r[2][0] == 1:
                same_bits(got, alone, p.rid + ": the full launch and the descriptor alone differ")
            else:
                parity("colsum_batch", p.rid + " out alone", alone, p.ref(), p.compose)


def run_colsum(p):
    p.reset()
    params = p.params()
    launch("miseg_colsum", C.byref(params), stream())
    return p.result()


@pytest.mark.parametrize("row", S.COLSUM_ROWS, ids=lambda r: r[0])
def test_colsum_row(row):
    rid, kw, form = row
    keep = bool(kw["accumulate"])      # accumulate 0: the earlier content of `out` must be gone
    for ints in (True, False):
        p = ColsumProblem(rid, kw, ints)
        got = run_colsum(p)
        if ints:
            exact(rid + " out (integers)", got, p.ref(keep))
            continue
        parity("colsum", rid + " out", got, p.ref(keep), lambda: p.compose(keep))
        again = run_colsum(p)
        if form[4] == 1:      # one row block: one atomic per channel
            same_bits(got, again, rid + ": two launches with one writer per element differ")
        else:
            parity("colsum", rid + " out, second launch", again, p.ref(keep), lambda: p.compose(keep))


def test_zz_report_the_worst_errors():
    """prints the error table of this run (pytest -s): family, worst pooled and per-element error, judgements by the local_tol rule"""
    for fam, (pooled, loc, rule, n) in sorted(WORST.items()):
        print(f"WORST {fam:13s} bar {TOL[fam]:.0e} pooled {pooled:.2e} local {loc:.2e} local_tol-rule judgements {rule} of {n}")
    print(f"WALL {time.time() - T0[0]:.1f} s, slowest case {SLOWEST[0]:.2f} s: {SLOWEST[1]}")
    assert WORST
