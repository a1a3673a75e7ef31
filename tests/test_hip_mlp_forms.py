"""Launch forms, row edges and operand layouts of the fused MLP (csrc/mlp.hip): mlp_fwd_kernel<STAT, ANORM, CC> in its 8 instantiations and
mlp_bwd_kernel<BSTAT, CC> in its 4, behind miseg_mlp_fwd / miseg_mlp_bwd.

The rows are ROWS of tests/mlp_cases.py, the table tests/test_mlp_ref_cpu.py pins on the host (grid arithmetic, every instantiation named):
every row goes through `ops._call("miseg_mlp_fwd" | "miseg_mlp_bwd", p)` with its own L.Mlp struct.  Form -> rows:
  `fwd-c<48|96>-<plain|stat|anorm|anorm-stat>-m<4096|4101>`  the four forward forms with all tiles full and with a last tile of 5 rows (the clamped
      load min(row, M - 1)); `-walk-m65589` / `-walk-m32805`: the grid at its cap of 512 / 256 workgroups, 4 / 3 waves with a second tile, the
      last one ragged - `anorm-stat-walk` judges the normalisation of the prefetched tile;
  `-nores`, `-nob1`, `-nob2`, `-nob1-nob2`, `-noanout`  the NULL options; `-styles4-sel<0..3>`: num_styles = 4, the unselected styles' gamma and
      beta rows NaN-filled (a wrong arm of the select chain poisons the output); `-nogamma` / `-nobeta`: the selected style's row NULL;
  `bwd-c<48|96>-<plain|bstat>-m<4096|4101>`, `-walk-*`, `-nodx` (dx NULL: dz and h still written), `-nob1`;
  `-<x|res|y|an_out|dy|dz|h|dx|bs_x>-<slice|off8>`  each row view alone in a 16-byte aligned channel slice of wider rows and 8 bytes into a
      16-byte unit; `-mixed`: every view non-contiguous with an offset and a row stride of its own (a stride applied to the wrong operand);
  `-tails`  x and w1 scaled so that z spans about +-12 (exp(-z^2 / 2) underflows, the cdf saturates);  `-ints`  the exact-integer case.

Operands: x, res, dy and bs_x come from tests/layouts.py::place_in (NaN all around: a read outside the view poisons the result); y, an_out,
dz, h and dx from place_out, re-filled with the sentinel before each launch (an element the kernel skips stays 1536) and checked with
assert_untouched after it; `stat` and `bs_dstat` hold exactly miseg_instnorm_stat_bytes(1, C) between guard sentinels, zero on entry.
References are float64 torch on the very operands the kernel got (mlp_cases.reference; dx from the stored dz), judged by tests/parity.py pooled
and per element at 5e-3, the bar of test_fused_mlp_forward_and_backward; the `local_tol` rule of DESIGN.md section 3 is wired in (beyond the
per-element bound: at most twice the local error of torch's own bf16 composition) and reported.  Bit-equality contracts: every anorm row
equals miseg_instnorm_apply followed by the plain miseg_mlp_fwd (y and an_out); every bstat row equals the plain backward launch (dz, h, dx);
every row launches twice and repeats its outputs bit for bit; the `-ints` rows equal float64 rounded once to bf16.  The atomic sums are judged
by value: forward statistics against float64 sums of the stored, rounded y (rtol 2e-6, atol 1e-3), norm-backward sums against
miseg_instnorm_bwd_reduce over the stored dx (2e-5 of the column's largest sum).  Refusals (mlp_cases.REFUSALS) return before any launch:
the error status, every output buffer still the sentinel, the statistics still zero; their operands are real buffers of the refused layout.
Nothing here searches a kernel's assembly or runs under a sanitizer.

NOT launched: the workload's own shapes (110 592 and 13 824 rows: tests/test_hip_kernels.py); a walking wave under the plain and anorm-only
forward forms (the walk is the loop of the `stat` rows; the forms differ in the epilogue only); `num_styles` 2 and 3.

Measured on an MI355X, worst over the rows, pooled / per element, C = 48 | C = 96 (the last test of the file prints this table; no row needed
the local_tol rule; bar 5e-3 - one rounding of the output to bf16 is 2^-9 at the worst):
  y        1.67e-3 / 2.97e-3 | 1.67e-3 / 2.98e-3        stored norm(x)  1.66e-3 / 3.03e-3 | 1.67e-3 / 3.07e-3
  h        1.67e-3 / 3.31e-3 | 1.66e-3 / 3.32e-3        dz              1.66e-3 / 3.27e-3 | 1.66e-3 / 3.29e-3
  dx       1.84e-3 / 2.89e-3 | 1.69e-3 / 2.91e-3        (the `-tails` rows, z with a standard deviation of 4, are among them)
  forward statistics at most 1.9e-7 relative (bar rtol 2e-6); norm-backward sums at most 3.0e-7 of the column's largest sum (bar 2e-5)
Wall time of the file: 2.3 s for its 184 cases run alone (the slowest, 1.0 s, is the first launch of the process) - the GEMM forms file: 1.8 s
for 142 cases.

What the rows exposed: no wrong number, no overwritten sentinel, no NaN read, no bit that differs between two launches or between a fused form
and the route it replaces.  One missing check: miseg_mlp_fwd / miseg_mlp_bwd tested `ldx >= C` and `ldy >= C` but no other row stride, so a
negative `ldres`, `lddy`, `lddz`, `ldh`, `lddx` or `ld_bs_x` - all multiples of 4 pass the alignment test - sent the kernel to rows before the
operand's base, and a stride between 0 and the row's width made output rows overlap (several producers per element).  The header now states
the contract (stride >= width for every row operand) and both entry points refuse anything else.  Red on the parent's library: the six
refusal rows `fwd-ldres-below-width`, `bwd-lddy-`, `bwd-lddz-`, `bwd-ldh-`, `bwd-lddx-` and `bwd-ldbs_x-below-width` (the call launched; their
stride is width - 4, in bounds); the other 64 refusal rows and every launched row are green there too.

That the file can fail - seven mutations of mlp.hip, each built from a copy outside the repository and run once; all give wrong numbers from
in-bounds accesses only.  Red rows of this file / of the older tests (tests/test_hip_kernels.py -k fused_mlp, 6 cases):
  1. a wave stops after its first tile (both kernels): the eight `-walk-` rows / old: 1 red (the 110 592-row folded-norm case; C = 96 never walked);
  2. the prefetched tile is not normalised (normx skipped in the loop): `fwd-c48-anorm-stat-walk-m65589`, `fwd-c96-anorm-stat-walk-m32805` /
     old: 1 red (110 592 x 48);
  3. C = 96: the transposed W1 read swaps fi >> 2 and fi & 3: all 22 `bwd-c96-*` rows with dx, `-ints` and `-tails` among them, and the wrapper
     case at 96 / old: 2 red;
  4. res read with the smaller of ldy and ldres (ldy itself would leave a contiguous res): the four `fwd-*-res-slice` / `res-off8` rows and both
     wrapper cases / old: NONE red;
  5. the last 16-channel slice left out of the STAT sums: all 40 rows with forward statistics and both wrapper cases / old: 4 red;
  6. gelu' without its z phi(z) term: the 44 backward rows but `-ints` (where the term is exactly 0), and both wrapper cases / old: 4 red;
  7. lb2 indexed without 4 * kg: the 60 forward rows with a b2 (`-nob2`, `-nob1-nob2` stay green) and both wrapper cases / old: 4 red.
What the older tests did not observe: the STAT = false forms, a walking wave at C = 96 or under the plain backward, any operand that is not
contiguous (mutation 4), the NULL options, the style select chain, bytes beside the outputs and the statistics, and the refusals.
"""
import time

import pytest
import torch
import torch.nn.functional as F

import mlp_cases as MC
from layouts import SENT, Slot, _bits, assert_untouched, place_in, place_out
from parity import assert_parity, local_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
GUARD = 64
INPUTS = {"fwd": ("x", "res"), "bwd": ("x", "dy", "bs_x")}
OUTPUTS = {"fwd": ("y", "an_out"), "bwd": ("dz", "h", "dx")}
WORST = {}             # (quantity, C) -> [pooled, local, rows judged by the local_tol rule]
SUMS = {"stat": 0.0, "bstat": 0.0}
SLOWEST = [0.0, ""]
T0 = [None]


def _ops():
    from mi_seg_amd.hip import ops
    return ops


def _L():
    from mi_seg_amd.hip import lib
    return lib


def rnd(*shape, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed + 7 * sum(shape))
    return torch.randn(*shape, generator=g, device=DEV) * scale + shift


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
        self.t.fill_(self.fill)

    def check(self, what):
        g = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]])
        assert bool((g == SENT).all()), f"{what}: a sentinel beside the buffer was overwritten"


def slot(shape, lay, fill):
    """tests/layouts.py::Slot for a layout name; (element offset, row stride): the same construction with the row's own numbers"""
    if not isinstance(lay, tuple):
        return place_out(shape, BF, lay) if fill == SENT else Slot(tuple(shape), BF, lay, fill)
    off, ld = lay
    s = Slot.__new__(Slot)
    s.layout = lay
    s.buf = torch.full((16 + shape[0] + 1, ld), fill, dtype=BF, device=DEV)
    s.index = (slice(16, 16 + shape[0]), slice(off, off + shape[1]))
    s.view = s.buf[s.index]
    assert off + shape[1] <= ld and s.buf.data_ptr() % 16 == 0
    return s


def put_in(values, lay):
    if not isinstance(lay, tuple):
        return place_in(values, lay)
    s = slot(values.shape, lay, float("nan"))
    s.view.copy_(values)
    return s.view


def _at(view):
    return addr(view), view.stride(-2)


def _check_layout(rid, name, view, lay):
    off, ld = MC.layout(view.shape[-1], lay)
    assert view.stride(-2) == ld and view.data_ptr() % 16 == (2 * off) % 16, (rid, name, lay, view.stride(), ld)


def parity(rid, quantity, Cc, got, ref, compose=None):
    """assert_parity at the bar; a result beyond the per-element bound is judged by the local_tol rule"""
    what = f"{rid} {quantity}"
    try:
        pooled, loc = assert_parity(got, ref, MC.TOL, what)
        rule = False
    except AssertionError:
        if compose is None:
            raise
        lt = max(MC.TOL, 2 * local_err(compose().double(), ref)[0])
        pooled, loc = assert_parity(got, ref, MC.TOL, what, local_tol=lt)
        rule = True
    print(f"PARITY {what}: pooled {pooled:.3e} local {loc:.3e}{' (local_tol rule)' if rule else ''}")
    w = WORST.setdefault((quantity, Cc), [0.0, 0.0, 0])
    w[0], w[1], w[2] = max(w[0], pooled), max(w[1], loc), w[2] + int(rule)


def same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous())), f"{what}: not the same bits"


def exact(got, ref64, what):
    same_bits(got, ref64.to(BF), what + ": exact integers, float64 rounded once to bf16")


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


def _values(kw):
    """the operands' values, contiguous: x, res, dy, bs_x [M, C] bf16; w1 [HID, C], w2 [C, HID], their transposes; b1, b2 fp32"""
    Cc, M = kw["C"], kw["M"]
    H = 4 * Cc
    if kw.get("ints"):
        v = {k: t.to(DEV) for k, t in MC.int_case(M, Cc).items()}
    else:
        sx, sw = (2.0, 2.0) if kw.get("tails") else (1.0, 1.0)      # tails: z = x w1 + b1 with a standard deviation of 4
        x = rnd(M, Cc, seed=701, scale=1.5, shift=0.3) if kw.get("an") else rnd(M, Cc, seed=701, scale=sx)      # an: the raw input of a norm
        v = dict(x=x.to(BF), res=rnd(M, Cc, seed=702).to(BF), dy=rnd(M, Cc, seed=703).to(BF), w1=(rnd(H, Cc, seed=704) * sw / Cc ** 0.5).to(BF),
                 b1=rnd(H, seed=705) / 4, w2=(rnd(Cc, H, seed=706) / H ** 0.5).to(BF), b2=rnd(Cc, seed=707) / 4)
    v["bs_x"] = rnd(M, Cc, seed=708, scale=1.3, shift=-0.2).to(BF)
    v["w2t"], v["w1t"] = v["w2"].t().contiguous(), v["w1"].t().contiguous()
    for k in ("b1", "b2", "res"):
        if not kw.get(k, 1):
            v[k] = None
    return v


def _weights_at(v):
    return {k: addr(v[k]) for k in ("w1", "w2", "w2t", "w1t", "b1", "b2") if v[k] is not None}


def _plain(L, ops, kw, v, x):
    """the plain launch of the same problem on contiguous operands: no folded norm, no statistics, no norm-backward sums"""
    Cc, M = kw["C"], kw["M"]
    k0 = {k: kw[k] for k in ("dir", "C", "M", "res", "b1", "b2", "dx") if k in kw}
    at = _weights_at(v)
    at["x"] = _at(x)
    out = {}
    if kw["dir"] == "fwd":
        if v["res"] is not None:
            at["res"] = _at(v["res"])
        names = ("y",)
    else:
        at["dy"] = _at(v["dy"])
        names = ("dz", "h", "dx") if kw.get("dx", 1) else ("dz", "h")
    for n in names:
        out[n] = torch.full((M, MC.view_cols(k0)[n]), SENT, dtype=BF, device=DEV)
        at[n] = _at(out[n])
    ops._call("miseg_mlp_fwd" if kw["dir"] == "fwd" else "miseg_mlp_bwd", MC.params(L, k0, at))
    return out


@pytest.mark.parametrize("row", MC.ROWS, ids=lambda r: r[0])
def test_form(row):
    rid, kw = row
    L, ops = _L(), _ops()
    lib = L.load()
    Cc, M, d = kw["C"], kw["M"], kw["dir"]
    H = 4 * Cc
    lay = kw.get("lay", {})
    cols = MC.view_cols(kw)
    assert lib.miseg_mlp_fused(M, Cc, H, L.BF16) == 1 and MC.walkers(M, Cc) == kw.get("walkers", 0)
    ops.begin_step()
    v = _values(kw)
    at = _weights_at(v)
    ins, outs = {}, {}
    for name in INPUTS[d]:
        if name in cols:
            ins[name] = put_in(v[name], lay.get(name, "contig"))
            _check_layout(rid, name, ins[name], lay.get(name, "contig"))
            at[name] = _at(ins[name])
    for name in OUTPUTS[d]:
        if name in cols:
            outs[name] = slot((M, cols[name]), lay.get(name, "contig"), SENT)
            _check_layout(rid, name, outs[name].view, lay.get(name, "contig"))
            at[name] = _at(outs[name].view)

    # ---- statistics buffers of exactly the size the library reports, between sentinels, zero on entry
    bufs = {}
    nstat = lib.miseg_instnorm_stat_bytes(1, Cc) // 8
    assert nstat >= 16 * Cc * 2      # [16 replicas][B = 1][C][2], what the kernels index
    if kw.get("stat"):
        bufs["stat"] = Guarded(nstat, torch.float64)
        at["stat"] = addr(bufs["stat"].t)
    if kw.get("bstat"):
        bufs["bs_dstat"] = Guarded(nstat, torch.float64)
        x_stat = ops.instnorm_stats(v["bs_x"].view(1, M, Cc), 1, M)
        at["bs_dstat"], at["bs_stat"] = addr(bufs["bs_dstat"].t), addr(x_stat)
    nref = None
    if kw.get("an"):
        ns, sel = kw["an"], kw.get("style", 0)
        a_stat = ops.instnorm_stats(v["x"].view(1, M, Cc), 1, M)
        nan = torch.full((Cc,), float("nan"), device=DEV)
        gam = [rnd(Cc, seed=710 + i, scale=0.2, shift=1.0) if i == sel else nan for i in range(ns)]
        bet = [rnd(Cc, seed=720 + i, scale=0.3) if i == sel else nan for i in range(ns)]
        if kw.get("gamma_null"):
            gam[sel] = None
        if kw.get("beta_null"):
            bet[sel] = None
        styles = torch.tensor([sel], dtype=torch.int32, device=DEV) if ns > 1 else None
        nref = ops.NormRef(a_stat, styles, gam, bet, MC.EPS)
        at["an_stat"] = addr(a_stat)

    p = MC.params(L, kw, at)
    if nref is not None:
        nref.fill(p.an)
        assert p.an.num_styles == kw["an"]
    fn = "miseg_mlp_fwd" if d == "fwd" else "miseg_mlp_bwd"
    runs = []
    for _ in range(2):
        for s in outs.values():
            s.view.fill_(SENT)
        for b in bufs.values():
            b.reset()
        ops._call(fn, p)
        for name, s in outs.items():
            assert_untouched(s, f"{rid} {name}")
        for name, b in bufs.items():
            b.check(f"{rid} {name}")
        runs.append({**{n: s.view.clone() for n, s in outs.items()}, **{n: b.t.clone() for n, b in bufs.items()}})
    r0, r1 = runs
    for name in outs:      # one producer per element
        same_bits(r0[name], r1[name], f"{rid} {name} of two launches")
    w1, w2 = v["w1"], v["w2"]

    if d == "fwd":
        x_eff = v["x"]
        if nref is not None:      # the route the fold replaces: miseg_instnorm_apply, then the plain launch - the same bits
            xn0 = ops.instnorm_apply(v["x"].view(1, M, Cc), 1, M, a_stat, styles, gam, bet).view(M, Cc)
            same_bits(r0["y"], _plain(L, ops, kw, v, xn0)["y"], rid + " y against instnorm_apply + the plain launch")
            if "an_out" in r0:
                same_bits(r0["an_out"], xn0, rid + " an_out against instnorm_apply")
            parity(rid, "norm(x)", Cc, xn0, MC.norm_ref(v["x"], gam[sel], bet[sel]))
            x_eff = xn0
        R = MC.reference(x_eff, w1, v["b1"], w2, v["b2"], v["res"])
        if kw.get("ints"):
            MC.assert_int_ranges(R, w1)
            exact(r0["y"], R["y"], rid + " y")

        def compose():
            z = x_eff @ w1.t()
            y = F.gelu(z + v["b1"].to(BF) if v["b1"] is not None else z) @ w2.t()
            y = y + v["b2"].to(BF) if v["b2"] is not None else y
            return y + v["res"] if v["res"] is not None else y
        parity(rid, "y", Cc, r0["y"], R["y"], compose)
        if kw.get("stat"):      # the statistics of the stored, rounded output
            yd = r0["y"].double()
            want = torch.stack([yd.sum(0), (yd * yd).sum(0)], -1)
            for r in (r0, r1):
                st = r["stat"].view(-1, Cc, 2).sum(0)
                assert torch.allclose(st, want, rtol=2e-6, atol=1e-3), (rid, float((st - want).abs().max()))
                SUMS["stat"] = max(SUMS["stat"], float(((st - want).abs() / want.abs().clamp_min(1.0)).max()))
        return

    R = MC.reference(v["x"], w1, v["b1"], w2, None, None, v["dy"])
    if kw.get("bstat"):
        o0 = _plain(L, ops, kw, v, v["x"])
        for name in ("dz", "h", "dx"):
            same_bits(r0[name], o0[name], f"{rid} {name} against the plain backward launch")
    dxr = r0["dz"].double() @ w1.double()      # from the STORED dz
    if kw.get("ints"):
        dx_int = MC.assert_int_ranges(R, w1)
        exact(r0["h"], R["h"], rid + " h")
        exact(r0["dz"], R["dz"], rid + " dz")
        exact(r0["dx"], dx_int, rid + " dx")

    def zb():
        z = v["x"] @ w1.t()
        return z + v["b1"].to(BF) if v["b1"] is not None else z
    parity(rid, "h", Cc, r0["h"], R["h"], lambda: F.gelu(zb()))
    parity(rid, "dz", Cc, r0["dz"], R["dz"], lambda: (v["dy"] @ w2) * MC.gelu_grad(zb()))
    if "dx" in r0:
        parity(rid, "dx", Cc, r0["dx"], dxr, lambda: r0["dz"] @ w1)
    else:
        assert p.dx is None and p.lddx == 0
    if kw.get("bstat"):      # against the reduction launch over the stored gradient
        want = ops.instnorm_bwd_reduce(r0["dx"].contiguous().view(1, M, Cc), v["bs_x"].view(1, M, Cc), 1, M, x_stat).sum(0)      # [1, C, 2]
        scale = want.abs().max(dim=1, keepdim=True).values
        for r in (r0, r1):
            err = float(((r["bs_dstat"].view(-1, 1, Cc, 2).sum(0) - want).abs() / scale).max())
            print(f"BSTAT {rid}: {err:.3e} of the column's largest sum")
            assert err < 2e-5, (rid, err)
            SUMS["bstat"] = max(SUMS["bstat"], err)


@pytest.mark.parametrize("Cc", [48, 96])
def test_public_wrappers_pass_the_row_strides_on(Cc):
    """ops.mlp_fwd / ops.mlp_bwd with x, res and dy as channel slices of wider buffers: the same bits as on contiguous operands"""
    ops = _ops()
    kw = dict(dir="fwd", C=Cc, M=4101)
    v = _values(kw)
    M = kw["M"]
    xs, rs, gs = place_in(v["x"], "slice"), place_in(v["res"], "off8"), place_in(v["dy"], "slice")
    assert xs.stride(0) != Cc and rs.stride(0) not in (Cc, xs.stride(0))
    ops.begin_step()
    y = ops.mlp_fwd(xs, v["w1"], v["b1"], v["w2"], v["b2"], res=rs, want_stat=True)
    stat = ops.pop_gemm_stat(y)
    same_bits(y, ops.mlp_fwd(v["x"], v["w1"], v["b1"], v["w2"], v["b2"], res=v["res"]), "y from sliced and from contiguous operands")
    R = MC.reference(v["x"], v["w1"], v["b1"], v["w2"], v["b2"], v["res"], v["dy"])
    parity(f"wrappers-c{Cc}", "y", Cc, y, R["y"])
    yd = y.double()
    assert stat is not None and torch.allclose(stat.sum(0)[0], torch.stack([yd.sum(0), (yd * yd).sum(0)], -1), rtol=2e-6, atol=1e-3)
    dz, h, dx = ops.mlp_bwd(xs, gs, v["w1"], v["b1"], v["w2t"], v["w1t"])
    for got, want, name in zip((dz, h, dx), ops.mlp_bwd(v["x"], v["dy"], v["w1"], v["b1"], v["w2t"], v["w1t"]), ("dz", "h", "dx")):
        same_bits(got, want, name + " from sliced and from contiguous operands")
    parity(f"wrappers-c{Cc}", "h", Cc, h, R["h"])
    parity(f"wrappers-c{Cc}", "dz", Cc, dz, R["dz"])
    parity(f"wrappers-c{Cc}", "dx", Cc, dx, dz.double() @ v["w1"].double())
    dz2, h2, none = ops.mlp_bwd(xs, gs, v["w1"], v["b1"], v["w2t"], v["w1t"], need_dx=False)
    assert none is None
    same_bits(dz2, dz, "dz without dx")
    same_bits(h2, h, "h without dx")


def test_mlp_fused_edges():
    lib = _L().load()
    for M, Cc, hid, dt, yes in MC.FUSED_EDGES:
        assert lib.miseg_mlp_fused(M, Cc, hid, dt) == yes, (M, Cc, hid, dt)


@pytest.mark.parametrize("case", MC.REFUSALS, ids=lambda r: r[0])
def test_refusals_return_before_any_launch(case):
    """an error status, every output buffer still the sentinel, the statistics still zero.  Every pointer is a real buffer that holds the view the
    arguments describe (rows at least 768 wide for the refused shapes), so the arguments are wrong only in the way the id names."""
    rid, d, what = case
    L, ops = _L(), _ops()
    M, Cc, H, dt = what[1:] if what[0] == "shape" else (4096, 48, 192, 1)
    kw = dict(dir=d, C=Cc, M=M, HID=H, dtype=dt, an=1, stat=1, bstat=1)
    cols = MC.view_cols(kw)
    wide = (0, 768) if what[0] == "shape" else "contig"
    at, ins, outs = {}, [], []
    for name, c in cols.items():
        lay = what[2] if what[:2] == ("lay", name) else wide
        s = slot((M, c), lay, 1.0 if name in INPUTS[d] else SENT)
        at[name] = _at(s.view)
        if what == ("short", name):
            at[name] = (addr(s.view), c - 4)
        (outs if name in OUTPUTS[d] else ins).append(s)
    weights = {w: torch.ones(H * Cc + 8, dtype=BF, device=DEV) for w in ("w1", "w2", "w2t", "w1t")}
    for w, t in weights.items():
        at[w] = addr(t[4:]) if what == ("woff", w) else addr(t)
    b = torch.zeros(H + Cc, device=DEV)
    stats = [torch.zeros(L.load().miseg_instnorm_stat_bytes(1, 192) // 8, dtype=torch.float64, device=DEV) for _ in range(3)]
    at.update(b1=addr(b), b2=addr(b), stat=addr(stats[0]), bs_dstat=addr(stats[0]), an_stat=addr(stats[1]), bs_stat=addr(stats[2]))
    p = MC.params(L, kw, at)
    if what[0] == "struct":
        p.struct_size += 8
    if what[0] == "styles":
        p.an.num_styles = what[1]
    if what[0] == "nodx":
        p.dx, p.lddx = None, 0
    with pytest.raises(L.MisegHipError if what[0] == "shape" else ValueError):
        ops._call("miseg_mlp_fwd" if d == "fwd" else "miseg_mlp_bwd", p)
    torch.cuda.synchronize()
    for s in outs:
        assert bool((s.buf == SENT).all()), rid + ": a refused call wrote an output"
    assert not any(bool(s.any()) for s in stats), rid + ": a refused call wrote statistics"


def test_zz_report_the_worst_errors():
    """prints the error table of this run (pytest -s): quantity, channels, worst pooled and per-element error, judgements by the local_tol rule"""
    for (q, Cc), (pooled, loc, rule) in sorted(WORST.items()):
        print(f"WORST {q:8s} C={Cc:3d} pooled {pooled:.2e} local {loc:.2e} local_tol-rule judgements {rule}")
    print(f"SUMS forward statistics: worst relative distance {SUMS['stat']:.2e}; norm-backward sums: {SUMS['bstat']:.2e} of the column's largest sum")
    print(f"WALL {time.time() - T0[0]:.1f} s, slowest case {SLOWEST[0]:.2f} s: {SLOWEST[1]}")
    assert WORST
