"""Launch forms, K and row edges and operand layouts of the GEMM kernels (csrc/gemm.hip) behind miseg_gemm: the rank-1 kernels
(gemm_nt_k1_kernel, gemm_nt_k1_stat_kernel), gemm_nt_small_kernel<MTW, NTW, GELU, STAT, ANORM> in its 36 instantiations, gemm_nt_stream_kernel<K16,
GELU, NCH, STAT, SCAT, ANORM> in its 26, gemm_nt_kernel<T, TO, NT>, gemm_tn_kernel<T, TO> and gemm_tn_stream_kernel with its partial-tile sum.

The rows are FORM_ROWS of tests/gemm_cases.py, the table tests/test_gemm_plan_cpu.py pins on the host: every row goes through `ops._call("miseg_gemm",
p)` with its L.Gemm struct, and BEFORE the launch miseg_gemm_plan of these very params must have the fields the row expects (the id spells them) and
miseg_gemm_workspace_bytes must equal the plan's.  Form -> rows:
  `small-<mtw>x<ntw>-<plain|gelu|anorm|anorm-gelu|stat|bstat>-m<M>-k<K>-*`  the six tiles at a ragged M that keeps the tile, six epilogues each, K of
      32 / 96 / 160 / 544 (384 for the folded norm), M = 1, 15, 16, grids of 4, 48, 162, 168, 192, 252, 256 workgroups;
  `stream-k<K16>-<plain|gelu|anorm|anorm-gelu|stat|bstat|scat>-m<M>-n<N>-*`  4101 rows (a last tile of 5), `-walk`: waves with a second tile
      (66553 / 67320 rows), `-two-chunks` / `-two-groups`: more than one accumulator chunk per column group / one chunk per group with the sums;
  `nt<1..4>-<f32|bf16f32|bf16>-*`  the generic kernel: ragged M and N, K below one stage, K % 8 != 0, `split4`, `acc`, `one-stage`, and the bf16
      problems a misaligned operand sends there (`a-off2` .. `res-ldodd`) at 4101 rows;  `rank1-*`;  `tn-*` the generic TN kernel with the three
      refusals of the streaming path;  `tnstream-<wm>x<wn>-*`  one split, one reduce group, two, `acc`, `colsum`, `defer`.

Operands: A, B / W, res, aux when read and bs_x come from tests/layouts.py::place_in in the row's layout (NaN all around: a read outside the view
poisons the result); C, aux when written and an_out from place_out (every byte beside the view must survive); the statistics buffers, tn_colsum and
the workspace hold exactly the bytes the library reports, between sentinels, the workspace NaN-filled.  C starts from random values in every mode:
the store modes must overwrite them, `accumulate` is judged against before + product in float64.  References are float64 torch on the very operands the
kernel got; the folded norm also holds bit-equality with miseg_instnorm_apply followed by the plain GEMM; statistics against float64 sums of the stored,
rounded output (rtol 2e-6, atol 1e-3); norm-backward sums against miseg_instnorm_bwd_reduce over the stored gradient (2e-5 of the column's largest
sum); tests/parity.py judges pooled and per element at the bars tests/test_hip_kernels.py uses: 2e-4 for fp32 output (bf16 operands are exact in fp32,
so bf16 -> fp32 is held to the fp32 bar), 2e-2 for bf16 output, twice that for the GELU-derivative epilogue.  The `local_tol` rule of DESIGN.md
section 3 is wired in (a bf16 row beyond the per-element bound: at most twice the local error of torch's own bf16 composition) and reported.  One
exact-integer row per family (`-ints-`) must match bit for bit.  Every row launches twice: rows with a single producer per element repeat bit for
bit, atomic rows (split_k, several reduce groups) are judged by parity only.

NOT launched (pinned on the host in tests/test_gemm_plan_cpu.py): the workload's own shapes (13 824 .. 884 736 rows: tests/test_hip_kernels.py and
scripts/gemm_table.py launch them); the 256-workgroup cap of a weight above 80 KB with a walking wave (M above 32 768 at N = 400, K = 96: the cap
is one `min` in the plan, the walk is the 512-cap rows').  The fused MLP has its rows in tests/test_hip_mlp_forms.py (tests/mlp_cases.py);
miseg_gemm_tn_group, miseg_gemm_tn_reduce_batch and the column sums have theirs in tests/test_hip_step_end_forms.py (tests/step_end_cases.py),
miseg_gemm_tn_stream_group in tests/test_hip_tn_stream_group.py and miseg_permute3 in tests/test_hip_row_op_edges.py: none of them has rows here.
Nothing here searches a kernel's assembly or runs under a sanitizer.

Measured on an MI355X, worst over the rows, pooled / per element (the last test of the file prints this table; no row needed the local_tol rule):
  small, stream, rank-1, generic NT and TN with bf16 output   1.7e-3 / 3.3e-3   (bar 2e-2: one rounding of the output to bf16, 2^-9 at the worst)
  generic NT    fp32 1.1e-7 / 4.6e-7    bf16 -> fp32 6.9e-8 / 2.7e-7    (bar 2e-4)
  generic TN    fp32 1.6e-7 / 5.2e-7    bf16 -> fp32 1.3e-7 / 6.1e-7 .. 6.9e-7 (atomic rows, three runs)    rank-1 fp32 2.5e-8 / 4.6e-8
  TN streaming  bf16 -> fp32 2.7e-7 / 1.5e-6; its column sums 4.8e-8 / 7.1e-8; the deferred partial tiles summed on the host 9.0e-8 / 3.1e-7
  norm(A) of the folded norm against float64 1.7e-3 / 2.6e-3 (bar 5e-3); norm-backward sums at most 2.8e-7 of the column's largest sum (bar 2e-5)
Wall time of the file: 1.8 s for its 142 cases run alone (the slowest, 0.9 s, is the first launch of the process), 0.6 s inside the whole suite.

What the rows exposed.  (a) The documented defect, DESIGN.md 3.3 (4): on the parent's library the four `*-one-stage-*` rows were red, and the
public call returned 30000.0 where the product is 1.3e-4 - fixed in gemm_plan (mode and fill both follow the rounded split).  (b) A TN product
with bf16 OUTPUT and the library's own split (`tn-bf16-auto-k1000-m72-n104`) was planned with two atomic splits and a zero fill: bf16 has no
atomics (the splits would overwrite each other) and the fill counts 4-byte words, twice the bytes of a bf16 C.  The plan assertion caught it before
anything was launched; gemm_plan now keeps one split unless the output is fp32.  No Python caller passes bf16 output to a TN product.
Everything else: no wrong number, no overwritten sentinel, no NaN read.

That the file can fail - seven mutations of gemm.hip, each built from a copy outside the repository and run once; all give wrong numbers from
in-bounds accesses only (loops that do less, dropped terms).  Red rows of this file / of the older tests (tests/test_hip_kernels.py -k "gemm or rank1"):
  1. small kernel, the last wave's k-range dropped: the eleven `small-*` rows whose fourth wave has k-steps (K = 544, K = 384), every epilogue
     among them / old: 13 red (K >= 128);
  2. streaming kernel, a wave stops after its first tile: the four `*-walk-*` rows (folded norm, statistics, norm-backward sums, scatter) / old:
     3 red (the 110 592-row cases of the three folds; the plain streaming test's shapes never walk);
  3. streaming statistics, the last column tile's sums never reach LDS: all three `stream-*-stat-*` and all five `stream-*-bstat-*` rows / old: 9 red;
  4. generic kernel, the bias kept in every split: `nt4-f32-split4-*-bias`, `nt3-f32-split4-acc-*-bias`, `nt3-bf16f32-split4-bias-*` / old: NONE red;
  5. the element-load path drops its last element: 13 `nt*` rows (K % 8 != 0 or K % 4 != 0, `a-off2`, `a-off4`, `b-off8`, `a-ldodd`, `b-ldodd`) and 7
     `tn-*` rows (ragged M or N, `a-off4`, `tn-stream-a-off8`) / old: 5 red;
  6. the TN partial-tile sum starts at split 1: the seven `tnstream-*` rows that run it (not `-defer`, not `-one-split`) / old: 4 red;
  7. rank-1 statistics kernel skips the tail rows: the six `rank1-*-stat-*` rows / old: 8 red.
What the older tests did not observe: WHICH form a case ran, operands that are not contiguous and aligned, split_k and accumulate on the NT
side (mutation 4), and writes beside C, aux, an_out, the statistics, the column sums and the workspace."""
import ctypes as C
import time

import pytest
import torch

import gemm_cases as G
from layouts import SENT, _bits, assert_untouched, place_in, place_out
from parity import assert_parity, local_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
TD = {0: torch.float32, 1: torch.bfloat16}
TOL = {0: 2e-4, 1: 2e-2}      # by output dtype
GUARD = 64
FAMILY = {G.RANK1: "rank1", G.RANK1_STAT: "rank1", G.SMALL: "small", G.STREAM: "stream", G.NT_GENERIC: "nt", G.TN_GENERIC: "tn", G.TN_STREAM: "tnstream"}
WORST = {}             # (family, dtype pair) -> [pooled, local, rows judged by the local_tol rule]
SLOWEST = [0.0, ""]
T0 = [None]


def _ops():
    from mi_seg_amd.hip import ops
    return ops


def _L():
    from mi_seg_amd.hip import lib
    return lib


def rnd(*shape, dtype=torch.float32, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed + 7 * sum(shape))
    return (torch.randn(*shape, generator=g, device=DEV) * scale + shift).to(dtype)


def addr(t):
    return int(t.data_ptr())


class Guarded:
    """n elements of `dtype` between two runs of GUARD sentinels"""

    def __init__(self, n, dtype, fill=0.0):
        self.buf = torch.full((GUARD + n + GUARD,), SENT, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + n]
        self.fill = fill
        assert self.t.data_ptr() % 16 == 0

    def reset(self):
        self.t.copy_(self.fill) if torch.is_tensor(self.fill) else self.t.fill_(self.fill)

    def check(self, what):
        g = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]])
        assert bool((g == SENT).all()), f"{what}: a sentinel beside the buffer was overwritten"


def _slot_at(slot):
    return addr(slot.view), slot.view.stride(-2)


def _check_layout(rid, name, view, kw):
    c, es = G.operand_cols(kw)[name]
    lay = kw.get("lay", {}).get(name, "contig")
    off, ld = G.layout(c, es, lay)
    assert view.stride(-2) == ld and view.data_ptr() % 16 == (off * es) % 16, (rid, name, lay, view.stride(), ld)


def gelu_grad(h):
    return 0.5 * (1.0 + torch.erf(h * 0.7071067811865476)) + h * torch.exp(-0.5 * h * h) * 0.3989422804014327


def gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z * 0.7071067811865476))


def _note(fam, pair, pooled, loc, rule):
    w = WORST.setdefault((fam, pair), [0.0, 0.0, 0])
    w[0], w[1], w[2] = max(w[0], pooled), max(w[1], loc), w[2] + int(rule)


def parity(rid, fam, pair, quantity, got, ref, tol, compose=None):
    """assert_parity at `tol`; a bf16 result beyond the per-element bound is judged by the local_tol rule"""
    what = f"{rid} {quantity}"
    try:
        pooled, loc = assert_parity(got, ref, tol, what)
        rule = False
    except AssertionError:
        if compose is None or got.dtype != torch.bfloat16:
            raise
        lt = max(tol, 2 * local_err(compose().double(), ref)[0])
        pooled, loc = assert_parity(got, ref, tol, what, local_tol=lt)
        rule = True
    print(f"PARITY {what}: pooled {pooled:.3e} local {loc:.3e}{' (local_tol rule)' if rule else ''}")
    _note(fam, pair, pooled, loc, rule)


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


def _inputs(kw, seed):
    """(a, b) values: NT a [M, K], b [N, K]; TN a [K, M], b [K, N]"""
    M, N, K, tn = kw["M"], kw["N"], kw["K"], kw.get("tn", 0)
    dt = TD[G.dtypes(kw)[0]]
    sa, sb = ((K, M), (K, N)) if tn else ((M, K), (N, K))
    if kw.get("ints"):
        return ((torch.arange(sa[0] * sa[1], device=DEV).reshape(sa) % 7 - 3).to(dt), (torch.arange(sb[0] * sb[1], device=DEV).reshape(sb) % 5 - 2).to(dt))
    if kw.get("an"):      # the raw input of an instance norm: off-centre, not unit variance
        return rnd(*sa, seed=seed, scale=1.7, shift=0.4).to(dt), (rnd(*sb, seed=seed + 1) / K ** 0.5).to(dt)
    return rnd(*sa, dtype=dt, seed=seed), (rnd(*sb, seed=seed + 1) / (1.0 if tn else K ** 0.5)).to(dt)


@pytest.mark.parametrize("row", G.FORM_ROWS, ids=lambda r: r[0])
def test_form(row):
    rid, kw, expect = row
    L, ops = _L(), _ops()
    lib = L.load()
    M, N, K, tn = kw["M"], kw["N"], kw["K"], kw.get("tn", 0)
    dti, dto = G.dtypes(kw)
    ti, to = TD[dti], TD[dto]
    lay = kw.get("lay", {})
    ops.begin_step()
    av, bv = _inputs(kw, 501)
    at, ins = {}, {}
    for name, v in (("A", av), ("B", bv)):
        ins[name] = place_in(v, lay.get(name, "contig"))
        _check_layout(rid, name, ins[name], kw)
        at[name] = (addr(ins[name]), ins[name].stride(-2))
    bias = rnd(N, seed=503) if kw.get("bias") else None
    resv = rnd(M, N, dtype=to, seed=504) if kw.get("res") else None
    hv = rnd(M, N, dtype=to, seed=505) if kw.get("epi") == 2 else None      # the pre-activation of the layer in front (GELU-derivative epilogue)
    xv = rnd(M, N, seed=506, scale=1.3, shift=-0.2).to(to) if kw.get("bstat") else None
    for name, v in (("res", resv), ("aux", hv), ("bs_x", xv)):
        if v is not None:
            ins[name] = place_in(v, lay.get(name, "contig"))
            _check_layout(rid, name, ins[name], kw)
            at[name] = (addr(ins[name]), ins[name].stride(-2))
    if bias is not None:
        at["bias"] = addr(bias)

    # ---- outputs: C (random values first), aux when written, an_out - each inside sentinels
    outs = {}
    scat = kw.get("scat")
    if scat:
        d, h, w, co = scat
        Bn = M // (d * h * w)
        c_shape, c_lay = (Bn * 8 * d * h * w, 2 * co), "contig"      # rows of the doubled grid, twice as wide: the store goes to the left half
    else:
        c_shape, c_lay = (M, N), lay.get("C", "contig")
    outs["C"] = place_out(c_shape, to, c_lay)
    if scat:
        outs["C"].index = (slice(None), slice(0, co))
        outs["C"].view = outs["C"].buf[outs["C"].index]
    _check_layout(rid, "C", outs["C"].view, kw)
    c0 = rnd(*outs["C"].view.shape, seed=507).to(to)
    if kw.get("epi") == 1:
        outs["aux"] = place_out((M, N), to, lay.get("aux", "contig"))
        _check_layout(rid, "aux", outs["aux"].view, kw)
    if kw.get("an_out"):
        outs["an_out"] = place_out((M, K), ti, lay.get("an_out", "contig"))
        _check_layout(rid, "an_out", outs["an_out"].view, kw)
    for name, s in outs.items():
        at[name] = _slot_at(s)

    # ---- buffers of exactly the size the library reports, between sentinels
    bufs = {}
    nstat = lib.miseg_instnorm_stat_bytes(1, N) // 8
    if kw.get("stat") or kw.get("bstat"):
        assert nstat >= 16 * N * 2      # [16 replicas][B = 1][N][2], what the kernels index
        bufs["stat"] = Guarded(nstat, torch.float64)
        at["stat"] = addr(bufs["stat"].t)
    nref = None
    if kw.get("bstat"):
        x_stat = ops.instnorm_stats(xv.view(1, M, N), 1, M)
        at["bs_stat"] = addr(x_stat)
    if kw.get("an"):
        ns = kw["an"]
        a_stat = ops.instnorm_stats(av.view(1, M, K), 1, M)
        gam = [rnd(K, seed=510 + i, scale=0.2, shift=1.0) for i in range(ns)] if ns > 1 else None
        bet = [rnd(K, seed=520 + i, scale=0.3) for i in range(ns)] if ns > 1 else None
        styles = torch.tensor([ns - 1], dtype=torch.int32, device=DEV) if ns > 1 else None
        nref = ops.NormRef(a_stat, styles, gam, bet, 1e-5)
        at["an_stat"] = addr(a_stat)
    if kw.get("colsum"):
        bufs["tn_colsum"] = Guarded(M, torch.float32, fill=rnd(M, seed=508))
        at["tn_colsum"] = addr(bufs["tn_colsum"].t)

    p = G.form_params(L, kw, at)
    if nref is not None:
        nref.fill(p.an)
        assert p.an.num_styles == kw["an"]
    # ---- the plan of these very params, before anything is launched
    pl = L.GemmPlan()
    assert lib.miseg_gemm_plan(C.byref(p), C.byref(pl)) == 0, lib.miseg_last_error()
    got = {f: getattr(pl, f) for f in expect}
    assert got == expect, rid
    wsb = lib.miseg_gemm_workspace_bytes(C.byref(p))
    assert wsb == pl.workspace_bytes
    if wsb:
        bufs["workspace"] = Guarded(wsb // 4, torch.float32, fill=float("nan"))
        p.workspace = addr(bufs["workspace"].t)
    fam, pair = FAMILY[pl.kernel], {(0, 0): "f32", (1, 0): "bf16->f32", (1, 1): "bf16"}[(dti, dto)]

    runs = []
    for _ in range(2):
        outs["C"].view.copy_(c0)
        for b in bufs.values():
            b.reset()
        ops._call("miseg_gemm", p)
        for name, s in outs.items():
            assert_untouched(s, f"{rid} {name}")
        for name, b in bufs.items():
            b.check(f"{rid} {name}")
        runs.append({**{n: s.view.clone() for n, s in outs.items()}, **{n: b.t.clone() for n, b in bufs.items()}})
    r0, r1 = runs
    atomic_c = pl.out_mode == G.ATOMIC or (pl.kernel == G.TN_STREAM and pl.reduce_groups > 1)
    if not atomic_c:
        same_bits(r0["C"], r1["C"], rid + " C")
    for name in ("aux", "an_out", "workspace"):      # one producer per element, always
        if name in r0:
            same_bits(r0[name], r1[name], f"{rid} {name}")

    # ---- float64 references on the very operands the kernel got
    tol = TOL[dto]
    if tn:
        prod = av.double().t() @ bv.double()
        if kw.get("defer"):      # the partial tiles wait for a batched sum: C untouched, the tiles add up to the product
            same_bits(r0["C"], c0, rid + " C under defer_reduce")
            parity(rid, fam, pair, "sum of the partial tiles", r0["workspace"].view(pl.splits, M, N).double().sum(0).float(), prod, tol)
        else:
            ref = prod + c0.double() if kw.get("accumulate") else prod
            if kw.get("ints"):
                assert torch.equal(r0["C"].double(), ref.to(to).double()), rid + ": exact integers"
            parity(rid, fam, pair, "C", r0["C"], ref, tol, lambda: (av.t() @ bv).to(to))
        if kw.get("colsum"):
            want = bufs["tn_colsum"].fill.double() + av.double().sum(0)
            parity(rid, fam, pair, "column sums", r0["tn_colsum"], want, tol)
        return

    a_eff = av
    if nref is not None:      # the route the fold replaces: miseg_instnorm_apply, then the plain GEMM - the same bits
        xn0 = ops.instnorm_apply(av.view(1, M, K), 1, M, a_stat, styles, gam, bet).view(M, K)
        pre0 = torch.empty(M, N, dtype=to, device=DEV) if kw.get("epi") == 1 else None
        y0 = ops.gemm_nt(xn0, bv, bias, act=kw.get("act", 0), preact_out=pre0)
        same_bits(r0["C"], y0, rid + " C against instnorm_apply + the plain GEMM")
        if pre0 is not None:
            same_bits(r0["aux"], pre0, rid + " pre-activation against instnorm_apply + the plain GEMM")
        if "an_out" in r0:
            same_bits(r0["an_out"], xn0, rid + " an_out against instnorm_apply")
        xd = av.double()
        mu, var = xd.mean(0, keepdim=True), xd.var(0, unbiased=False, keepdim=True)
        xr = (xd - mu) / torch.sqrt(var + 1e-5) * (gam[-1].double() if gam else 1.0) + (bet[-1].double() if bet else 0.0)
        parity(rid, fam, pair, "norm(A)", xn0, xr, 5e-3)
        a_eff = xn0

    def formula(t):
        z = a_eff.to(t) @ bv.to(t).t()
        if bias is not None:
            z = z + bias.to(t)
        pre = z
        if kw.get("epi") == 2:
            z = z * gelu_grad(hv.to(t))
        if kw.get("act") == G.GELU:
            z = gelu(z)
        if resv is not None:
            z = z + resv.to(t)
        if kw.get("accumulate"):
            z = z + c0.to(t)
        return z, pre

    ref, pre_ref = formula(torch.float64)
    c_got = r0["C"]
    if scat:      # out[b, 2d+jd, 2h+jh, 2w+jw, co] = sum_ci x[b, d, h, w, ci] * w[(j, co), ci]
        ref = ref.reshape(Bn, d, h, w, 2, 2, 2, co).permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(-1, co)
    if kw.get("ints"):
        assert torch.equal(c_got.double(), ref.to(to).double()), rid + ": exact integers"
    parity(rid, fam, pair, "C", c_got, ref, 2 * tol if kw.get("epi") == 2 else tol, None if scat else lambda: formula(to)[0].to(to))
    if kw.get("epi") == 1:
        parity(rid, fam, pair, "pre-activation", r0["aux"], pre_ref, tol, lambda: formula(to)[1].to(to))
    if kw.get("stat"):      # the statistics of the stored, rounded output
        yd = c_got.double()
        want = torch.stack([yd.sum(0), (yd * yd).sum(0)], -1)
        for r in (r0, r1):
            st = r["stat"].view(-1, N, 2).sum(0)
            assert torch.allclose(st, want, rtol=2e-6, atol=1e-3), (rid, float((st - want).abs().max()))
    if kw.get("bstat"):      # against the reduction launch over the stored gradient
        want = ops.instnorm_bwd_reduce(c_got.contiguous().view(1, M, N), xv.view(1, M, N), 1, M, x_stat).sum(0)      # [1, N, 2]
        scale = want.abs().max(dim=1, keepdim=True).values
        for r in (r0, r1):
            st = r["stat"].view(-1, 1, N, 2).sum(0)
            err = float(((st - want).abs() / scale).max())
            print(f"BSTAT {rid}: {err:.3e} of the column's largest sum")
            assert err < 2e-5, (rid, err)


def test_public_gemm_nt_with_split_k_over_one_stage_returns_the_product():
    """ops.gemm_nt(.., out_dtype=float32, split_k=4) at K = 32 allocates its output with torch.empty: one split runs, and it must store - twice
    into a block of the caching allocator that held something else (it used to add to whatever the block held)"""
    ops = _ops()
    a, w = rnd(70, 32, seed=601), rnd(40, 32, seed=602) / 32 ** 0.5
    ref = a.double() @ w.double().t()
    for poison in (3.0e4, float("nan")):
        block = torch.full((70, 40), poison, dtype=torch.float32, device=DEV)
        where = block.data_ptr()
        del block
        y = ops.gemm_nt(a, w, out_dtype=torch.float32, split_k=4)
        assert y.data_ptr() == where      # the poisoned block came back
        assert_parity(y, ref, 2e-4, f"split_k=4 over one stage into a block of {poison}")


def test_zz_report_the_worst_errors():
    """prints the error table of this run (pytest -s): family, dtype pair, worst pooled and per-element error, judgements by the local_tol rule"""
    for (fam, pair), (pooled, loc, rule) in sorted(WORST.items()):
        print(f"WORST {fam:9s} {pair:9s} pooled {pooled:.2e} local {loc:.2e} local_tol-rule judgements {rule}")
    print(f"WALL {time.time() - T0[0]:.1f} s, slowest case {SLOWEST[0]:.2f} s: {SLOWEST[1]}")
    assert WORST
