"""The references of tests/winattn_ref.py, pinned without a GPU:

* ref_window_attention against an independent restatement with explicit loops over windows: the token gather by coordinate arithmetic, the
  shift mask from a region-id grid that is rolled and partitioned like the data (not compute_mask), the bias by explicit (dz, dy, dx)
  lookups under the base-tw decode (not the sliced index table) - at the per-axis-shift and clipped-window geometries of
  tests/test_hip_winattn_forms.py, to float64 rounding, `out` and `lse`;
* the inputs leave the room: the model of the matrix-core kernels' rounding points (winattn_ref.mfma_model) stays below HALF of each bar the
  GPU test holds `out` to, pooled and per element, on every bf16 input set of that test (the 270-unit case is represented by one window pair
  of the same distribution);
* the lse yardsticks: what they measure on these inputs, and that twice a yardstick still tells natural-log units from log2 units.

Measured here (model against float64, worst over the bf16 input sets): pooled 2.7e-3, local 9.4e-3 against 1e-2 (half of 2e-2) - of which
about 9e-3 are the roundings of P and of the output, which no choice of inputs moves (winattn_ref.QK_AMP); the lse yardsticks: fp32 and
fp32 sums on bf16 inputs 2e-7 .. 1.1e-6, the model 1e-4 .. 2e-3 (table amplitude 4)."""
import math

import pytest
import torch

import winattn_ref as W
from conftest import rel_err
from parity import local_err

S = W.Spec


def restated(case):
    """(out [B, D, H, W, C], lse [windows, heads, n]) in float64, window by window"""
    s = case.spec
    B, (D, H, Wd), (wd, wh, ww), (sd, sh, sw) = s.B, s.dims, s.ws, s.ss
    C, heads, hd, n, tw = s.C, s.heads, s.hd, s.n, s.tw
    Dp, Hp, Wp = (-(-d // w) * w for d, w in zip(s.dims, s.ws))
    qkv = case.qkv.double()
    row = case.qb.double() if case.qb is not None else torch.zeros(3 * C, dtype=torch.float64)
    # region ids on the UNROLLED padded grid, then rolled like the data: after the roll by -shift the last `shift` planes of an axis hold the
    # wrapped-around planes 0 .. shift-1 (id 2), the planes of the last window in front of them id 1, everything else id 0
    def axis_ids(P, w, sft):
        ids = torch.zeros(P, dtype=torch.long)
        if sft:
            ids[P - w + sft:] = 1
            ids[:sft] = 2
        return ids
    region = (axis_ids(Dp, wd, sd).view(-1, 1, 1) * 3 + axis_ids(Hp, wh, sh).view(1, -1, 1)) * 3 + axis_ids(Wp, ww, sw).view(1, 1, -1)
    region = torch.roll(region, shifts=(-sd, -sh, -sw), dims=(0, 1, 2))
    grid = row.view(1, 1, 1, 1, -1).repeat(B, Dp, Hp, Wp, 1)
    grid[:, :D, :H, :Wd] = qkv
    grid = torch.roll(grid, shifts=(-sd, -sh, -sw), dims=(1, 2, 3))
    # bias[i][j] = table[(dz + tw - 1, dy + tw - 1, dx + tw - 1)] with token t decoded base tw
    t = torch.arange(n)
    cz, cy, cx = t // (tw * tw), (t // tw) % tw, t % tw
    tb = 2 * tw - 1
    def rel(c):
        return c.view(-1, 1) - c.view(1, -1) + tw - 1
    bias = None
    if case.table is not None:
        tab3 = case.table.double().view(tb, tb, tb, heads)
        bias = tab3[rel(cz), rel(cy), rel(cx)]                       # [n, n, heads]
    out_p = torch.zeros(B, Dp, Hp, Wp, C, dtype=torch.float64)
    lse = torch.zeros(s.windows, heads, n, dtype=torch.float64)
    win = 0
    for b in range(B):
        for wz in range(Dp // wd):
            for wy in range(Hp // wh):
                for wx in range(Wp // ww):
                    sl = (slice(wz * wd, (wz + 1) * wd), slice(wy * wh, (wy + 1) * wh), slice(wx * ww, (wx + 1) * ww))
                    tok = grid[b][sl].reshape(n, 3 * C)
                    rid = region[sl].reshape(n)
                    o = torch.zeros(n, C, dtype=torch.float64)
                    for h in range(heads):
                        q, k, v = (tok[:, i * C + h * hd:i * C + (h + 1) * hd] for i in range(3))
                        sc = s.scale * (q @ k.T)
                        if bias is not None:
                            sc = sc + bias[:, :, h]
                        sc = sc + torch.where(rid.view(-1, 1) != rid.view(1, -1), -100.0, 0.0)
                        m = sc.max(-1, keepdim=True).values
                        e = (sc - m).exp()
                        z = e.sum(-1, keepdim=True)
                        lse[win, h] = (m + z.log()).squeeze(-1)
                        o[:, h * hd:(h + 1) * hd] = (e / z) @ v
                    out_p[b][sl] = o.view(wd, wh, ww, C)
                    win += 1
    out_p = torch.roll(out_p, shifts=(sd, sh, sw), dims=(1, 2, 3))
    return out_p[:, :D, :H, :Wd].contiguous(), lse


RESTATED = [S((14, 14, 7), (7, 7, 7), (3, 3, 0), 2, 32), S((7, 14, 14), (7, 7, 7), (0, 3, 3), 2, 32), S((14, 7, 4), (7, 7, 4), (3, 0, 0), 2, 32),
            S((7, 7, 4), (7, 7, 4), (0, 0, 0), 3, 48), S((4, 7, 7), (4, 7, 7), (0, 0, 0), 3, 48),
            # and: shifted padding with and without a bias row, the base-8 decode, no table
            S((9, 5, 6), (4, 4, 4), (2, 2, 2), 2, 32), S((9, 5, 6), (4, 4, 4), (2, 2, 2), 2, 32, bias=False), S((6, 6, 10), (6, 6, 10), (0, 0, 0), 1, 16, B=1, tw=8),
            S((10, 9, 8), (7, 7, 7), (3, 3, 3), 2, 32, B=1, table=False)]


@pytest.mark.parametrize("spec", RESTATED, ids=str)
def test_the_reference_agrees_with_an_independent_restatement(spec):
    assert spec.B <= 2
    case = W.Case(spec, torch.float32)
    ref = case.reference(backward=False)
    out, lse = restated(case)
    assert ref["lse"].shape == (spec.windows, spec.heads, spec.n) and ref["out"].shape == (spec.B, *spec.dims, spec.C)
    # float64 rounding: scores of magnitude <= ~1e2 (the -100 of the mask) summed over <= 384 keys
    assert float((ref["out"] - out).abs().max()) < 1e-12 * max(1.0, float(out.abs().max()))
    assert float((ref["lse"] - lse).abs().max()) < 1e-11


def test_the_global_reference_is_the_window_reference_of_one_window():
    spec = W.GLOBAL[1]
    case = W.Case(spec, torch.bfloat16)
    q = case.qkv.double()
    out, lse = W.ref_global_attention(q, spec.heads, spec.scale)
    o2, l2 = W.ref_window_attention(q, None, None, spec.heads, spec.ws, spec.ss, 1, spec.scale, with_lse=True)
    assert float((out - o2).abs().max()) < 1e-13 and float((lse - l2).abs().max()) < 1e-12 and lse.shape == (spec.B, spec.heads, spec.n)
    # and its mask multiplies the probabilities behind the softmax
    mask = (torch.rand(spec.B, spec.heads, spec.n, spec.n, generator=torch.Generator().manual_seed(5)) > 0.1).double() / 0.9
    od, ld = W.ref_global_attention(q, spec.heads, spec.scale, drop_mask=mask)
    ow = W.ref_window_attention(q, None, None, spec.heads, spec.ws, spec.ss, 1, spec.scale, drop_mask=mask)
    assert float((od - ow).abs().max()) < 1e-13 and torch.equal(ld, lse)


def _model_specs():
    specs = [s for s in W.all_bf16_specs() if s != W.PRODUCTION]
    # the 270-unit case: two of its windows' worth of the same distribution (same heads, channels, shift, padding on every axis)
    specs.append(S((12, 6, 5), (7, 7, 7), (3, 3, 3), 6, 96, B=1))
    return specs


@pytest.mark.parametrize("spec", _model_specs(), ids=str)
def test_the_inputs_leave_honest_bf16_arithmetic_below_half_of_the_bars(spec):
    """the condition that the inputs, not the kernel, leave the room: a forward with the matrix-core kernels' rounding points lands below half
    of the pooled and of the per-element bar on `out`"""
    case = W.Case(spec, torch.bfloat16)
    ref = case.reference(backward=False)
    out, lse = W.mfma_model(case.qkv, case.qb, case.table, spec.heads, spec.ws, spec.ss, spec.tw, spec.scale)
    pooled, loc = rel_err(out, ref["out"]), local_err(out, ref["out"])[0]
    print(f"{spec}: model pooled {pooled:.2e} local {loc:.2e} lse {float((lse.double() - ref['lse']).abs().max()):.2e}")
    half = W.TOL[torch.bfloat16] / 2
    assert pooled < half and loc < half, (pooled, loc)


def test_sharpening_through_q_and_k_would_not_leave_that_room():
    """why the bf16 cases draw q and k at half the usual amplitude and the sharp-softmax bf16 case sharpens through the fp32 table: on one
    343-token window the table at amplitude 4 leaves the model where it was, q and k at the usual amplitude times 3 (6 x QK_AMP) put it above
    the whole bar"""
    base = dict(dims=(7, 7, 7), ws=(7, 7, 7), ss=(0, 0, 0), heads=1, C=16, B=1)
    errs = {}
    for name, kw in (("plain", {}), ("table", {"table_amp": 4.0}), ("usual", {"qk_gain": 2.0}), ("usual x 3", {"qk_gain": 6.0})):
        spec = S(**base, **kw)
        case = W.Case(spec, torch.bfloat16)
        ref = case.reference(backward=False)
        out, _ = W.mfma_model(case.qkv, case.qb, case.table, spec.heads, spec.ws, spec.ss, spec.tw, spec.scale)
        errs[name] = local_err(out, ref["out"])[0]
    print(errs)
    half = W.TOL[torch.bfloat16] / 2
    assert errs["plain"] < half and errs["table"] < half and errs["usual"] < half and errs["usual x 3"] > 2 * half


LSE_SPECS = [S((7, 7, 7), (7, 7, 7), (0, 0, 0), 1, 16, B=1), S((10, 9, 8), (7, 7, 7), (3, 3, 3), 2, 32), S((10, 9, 8), (7, 7, 7), (3, 3, 3), 2, 32, table_amp=4.0),
             S((4, 4, 4), (2, 2, 2), (1, 1, 1), 1, 16), W.GLOBAL[0]]


@pytest.mark.parametrize("spec", LSE_SPECS, ids=str)
def test_the_lse_yardsticks(spec):
    """each yardstick is small against the quantity, larger than nothing, and twice it still separates natural-log from log2 units (the error
    the allowance exists to catch: lse (log2e - 1) on the largest |lse| of the case)"""
    for dtype, kinds in ((torch.float32, ("fp32",)), (torch.bfloat16, ("fp32", "mfma"))):
        case = W.Case(spec, dtype)
        ref = case.reference(backward=False)
        units = float(ref["lse"].abs().max()) * (W.LOG2E - 1)
        for kind in kinds:
            y = W.lse_yardstick(kind, case.qkv, case.qb, case.table, spec.heads, spec.ws, spec.ss, spec.tw, spec.scale, ref["lse"])
            print(f"{spec} {dtype} {kind}: lse yardstick {y:.2e}, a units error would be {units:.2e}")
            assert 0 < y < (2e-5 if kind == "fp32" else 2e-2)
            assert 2 * y < units / 4


def test_case_draws_are_reproducible_and_rounded_once():
    spec = S((9, 5, 6), (4, 4, 4), (2, 2, 2), 2, 32)
    a, b = W.Case(spec, torch.bfloat16), W.Case(spec, torch.bfloat16)
    assert torch.equal(a.qkv, b.qkv) and torch.equal(a.dout, b.dout) and torch.equal(a.table, b.table) and torch.equal(a.qb, b.qb)
    f = W.Case(spec, torch.float32)
    half = f.qkv.clone()
    half[..., :64] *= W.QK_AMP[torch.bfloat16] / W.QK_AMP[torch.float32]        # a power of two: the same draw, rounded once
    assert torch.equal(half.to(torch.bfloat16), a.qkv) and a.table.dtype == torch.float32 and a.table.shape == (2197, 2)
    assert W.Case(S((9, 5, 6), (4, 4, 4), (2, 2, 2), 2, 32, bias=False, table=False), torch.float32).qb is None
    assert spec.n == 64 and spec.windows == 2 * 3 * 2 * 2 and spec.padded and math.isclose(spec.scale, 0.25)
