"""GPU tests of the loss and Dice metric kernels of csrc/training.hip over their launch forms, class counts and edges: seg_loss_fwd_kernel,
seg_loss_finalize_kernel, seg_loss_bwd_kernel, dice_count_kernel and dice_finalize_kernel against the float64 restatement of
tests/seg_loss_ref.py on the cases of tests/seg_loss_cases.py (tests/test_seg_loss_ref_cpu.py shows that the cases reach every
instantiation the launchers list).

Bars: the project's 1e-5 relative on the loss (and on the sums the forward leaves for the backward) and 1e-4 on d(loss)/d(logits), pooled and per
element (parity.assert_parity).  The judge has no float32 in it and some inputs are extreme: a case named in seg_loss_cases.WIDENED would
take max(bar, 2 x the error of the float32 torch composition - the judge's formulas in float32 on the CPU on the same inputs - against the
judge), computed per case (parity.py local_tol; the pooled d(loss)/d(logits) check keeps its bar).  No case is named
there: every bound is the bar.  Each case prints the kernel's errors with its bounds."""
import ctypes as C
import zlib

import pytest
import torch

import seg_loss_cases as SC
import seg_loss_ref as R
from conftest import rel_err
from parity import assert_parity, local_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mods():
    from mi_seg_amd.hip import lib as L
    from mi_seg_amd.hip import ops
    return L, ops


# ------------------------------------------------------------------------------------------------ inputs
def on_device(x, misaligned=False):
    """a contiguous device copy; misaligned: one that starts 4 bytes into a larger buffer"""
    if not misaligned:
        return x.to(DEV).contiguous()
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=DEV)
    view = buf[1:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def check_against_the_judge(what, j, cfg, loss, sums, dlogits):
    """loss, sums [3 B C + 1] and dlogits of the kernels against SC.judged(); prints one line of measured errors and bounds"""
    B, Cc = dlogits.shape[:2]
    e_loss = abs(float(loss) - float(j["loss"])) / abs(float(j["loss"]))
    e_other = abs(float(sums[-1]) - float(j["other"])) / max(abs(float(j["other"])), 1e-300)
    got_sums = sums[:-1].reshape(B, Cc, 3)
    print(f"seg_loss {what}: loss {e_loss:.3e} (bound {j['loss_bound']:.3e}) other {e_other:.3e} (bound {j['other_bound']:.3e}) "
          f"sums {rel_err(got_sums, j['sums']):.3e} / {local_err(got_sums, j['sums'])[0]:.3e} (bound {j['sums_bound']:.3e}) "
          f"dlogits {rel_err(dlogits, j['grad']):.3e} / {local_err(dlogits, j['grad'])[0]:.3e} "
          f"(bounds {j['grad_pooled_bound']:.3e} / {j['grad_local_bound']:.3e})")
    assert e_loss <= j["loss_bound"], (what, float(loss), float(j["loss"]))
    assert e_other <= j["other_bound"], (what, float(sums[-1]), float(j["other"]))
    assert_parity(got_sums, j["sums"], j["sums_bound"], f"{what}: per-class sums")
    assert_parity(dlogits, j["grad"], j["grad_pooled_bound"], f"{what}: d loss / d logits", local_tol=max(j["grad_pooled_bound"], j["grad_local_bound"]))
    if cfg.kind == "dice_focal" and not cfg.include_background:
        assert torch.equal(dlogits[:, 0], torch.zeros_like(dlogits[:, 0])), f"{what}: channel 0 is outside the softmax support, its gradient is exactly 0"


# ------------------------------------------------------------------------------------------------ the loss cases
@pytest.mark.parametrize("case", SC.CASES, ids=[c.id for c in SC.CASES])
def test_seg_loss_case(case):
    """loss, per-class sums and d(loss)/d(logits) of one case against the float64 judge; a second forward and backward bit-identical"""
    L, ops = _mods()
    lab = SC.make_labels(case)
    x = SC.make_logits(case, lab)
    cfg = case.cfg
    kcfg = SC.criterion(cfg).cfg
    xd = on_device(x, case.misaligned)
    ld = lab.to(SC.LABEL_DTYPES[case.label_dtype]).to(DEV)
    gs = None if case.upstream is None else torch.tensor(case.upstream, dtype=torch.float32, device=DEV)
    loss, sums = ops.seg_loss_fwd(xd, ld, kcfg)
    dlogits = ops.seg_loss_bwd(xd, ld, kcfg, sums, gs)
    assert SC.form(cfg.kind, case.C, case.S, xd.data_ptr() % 16, dlogits.data_ptr() % 16) == case.bwd_form()
    check_against_the_judge(case.id, SC.judged(case.id, x, lab, cfg, case.upstream), cfg, loss, sums, dlogits)
    loss2, sums2 = ops.seg_loss_fwd(xd, ld, kcfg)
    dlogits2 = ops.seg_loss_bwd(xd, ld, kcfg, sums2, gs)
    assert torch.equal(loss2, loss) and torch.equal(sums2, sums) and torch.equal(dlogits2, dlogits)


@pytest.mark.parametrize("kind", R.KINDS)
def test_the_loss_modules_take_the_same_kernels(kind):
    """DiceFocalLoss / DiceCELoss / GeneralizedDiceFocalLoss through autograd, on misaligned logits: the numbers of the two direct calls"""
    L, ops = _mods()
    case = next(c for c in SC.CASES if c.id == f"misaligned-C3-{kind}")
    lab = SC.make_labels(case)
    xd = on_device(SC.make_logits(case, lab), True).requires_grad_(True)
    ld = lab.to(torch.int32).to(DEV)
    crit = SC.criterion(case.cfg)
    loss = crit(xd, ld)
    (loss * case.upstream).backward()
    want, sums = ops.seg_loss_fwd(xd.detach(), ld, crit.cfg)
    assert loss.is_cuda and torch.equal(loss.detach(), want)
    assert torch.equal(xd.grad, ops.seg_loss_bwd(xd.detach(), ld, crit.cfg, sums, torch.tensor(case.upstream, dtype=torch.float32, device=DEV)))


# ------------------------------------------------------------------------------------------------ buffers the test owns
def _guarded(n, dtype, guard):
    """(NaN-filled buffer of guard + n + guard elements, its middle)"""
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[guard:guard + n]


def _guards_untouched(buf, n, guard):
    return bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n:]).all())


# (kind, C, S, label type, guard of dlogits in floats): 65 floats put dlogits 4 bytes off a 16-byte boundary - the scalar backward by the
# gradient pointer alone, behind a vector forward.  S = 1028: two workgroups, the last one of one vector
OWNED = [("dice_focal", 3, 1028, "I32", 64), ("dice_ce", 8, 1028, "U8", 65), ("dice_ce", 9, 1028, "I64", 64),
         ("gdice_focal", 8, 1028, "F32", 64), ("gdice_focal", 3, 1028, "I64", 65), ("gdice_focal", 16, 1027, "U8", 67)]


@pytest.mark.parametrize("kind,Cc,S,dt,dguard", OWNED, ids=[f"{o[0]}-C{o[1]}-S{o[2]}-{o[3]}-g{o[4]}" for o in OWNED])
def test_seg_loss_writes_only_what_it_owns(kind, Cc, S, dt, dguard):
    """the C ABI with workspace (sized by miseg_seg_loss_workspace_bytes), sums and dlogits inside NaN-filled buffers: the guard regions on both
    sides stay NaN, no NaN is left inside, and the numbers are the judge's; one case per backward instantiation"""
    L, ops = _mods()
    lib = L.load()
    B = 2
    case = SC.Case(f"owned-{kind}-C{Cc}-S{S}-{dt}-g{dguard}", SC._BASE[kind], Cc, S, B=B, label_dtype=dt)
    lab = SC.make_labels(case)
    x = SC.make_logits(case, lab)
    xd, ld = on_device(x), lab.to(SC.LABEL_DTYPES[dt]).to(DEV)
    kcfg = SC.criterion(case.cfg).cfg
    nws = lib.miseg_seg_loss_workspace_bytes(B, Cc, S)
    assert nws == B * SC.nblk(S) * (3 * Cc + 1) * 8
    ws_buf, ws = _guarded(nws // 8, torch.float64, 16)
    sums_buf, sums = _guarded(3 * B * Cc + 1, torch.float64, 16)
    dl_buf, dl = _guarded(B * Cc * S, torch.float32, dguard)
    loss = torch.full((3,), float("nan"), dtype=torch.float32, device=DEV)
    gs = torch.tensor(1.7, dtype=torch.float32, device=DEV)
    p, _, _ = ops._seg_loss_params(xd, ld, kcfg, sums, ws)
    p.loss, p.gscale, p.dlogits = C.c_void_p(loss.data_ptr() + 4), C.c_void_p(gs.data_ptr()), C.c_void_p(dl.data_ptr())
    want_form = SC.form(kind, Cc, S, xd.data_ptr() % 16, dl.data_ptr() % 16)
    assert want_form == (8 if Cc <= 8 else 16, 4 if (Cc <= 8 and S % 4 == 0 and dguard % 4 == 0) else 1, kind == "gdice_focal")
    L.check(lib.miseg_seg_loss_fwd(C.byref(p), ops._stream()), "seg_loss_fwd")
    L.check(lib.miseg_seg_loss_bwd(C.byref(p), ops._stream()), "seg_loss_bwd")
    torch.cuda.synchronize()
    assert _guards_untouched(ws_buf, ws.numel(), 16) and not bool(torch.isnan(ws).any())
    assert _guards_untouched(sums_buf, sums.numel(), 16) and not bool(torch.isnan(sums).any())
    assert _guards_untouched(dl_buf, dl.numel(), dguard) and not bool(torch.isnan(dl).any())
    assert bool(torch.isnan(loss[0])) and bool(torch.isnan(loss[2])) and not bool(torch.isnan(loss[1]))
    check_against_the_judge(case.id, SC.judged(case.id, x, lab, case.cfg, 1.7), case.cfg, loss[1], sums, dl.view(B, Cc, S))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("B,Cc", [(65, 3), (2, 1), (2, 17)])
def test_seg_loss_refuses_what_it_has_no_kernel_for(B, Cc):
    """B = 65, C = 1 and C = 17: MISEG_E_UNSUPPORTED from both entry points with nothing written; the loss modules then take forward_torch"""
    L, ops = _mods()
    lib = L.load()
    S = 8
    g = torch.Generator().manual_seed(B * 100 + Cc)
    x = (3.0 * torch.randn(B, Cc, S, generator=g)).to(DEV)
    lab = torch.randint(0, Cc, (B, 1, S), generator=g).to(torch.int32).to(DEV)
    ws = torch.full((B * (3 * Cc + 1),), float("nan"), dtype=torch.float64, device=DEV)
    sums = torch.full((3 * B * Cc + 1,), float("nan"), dtype=torch.float64, device=DEV)
    dl = torch.full((B, Cc, S), float("nan"), dtype=torch.float32, device=DEV)
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=DEV)
    for kind in R.KINDS:
        crit = SC.criterion(SC._BASE[kind])
        p, _, _ = ops._seg_loss_params(x, lab, crit.cfg, sums, ws)
        p.loss, p.dlogits = C.c_void_p(loss.data_ptr()), C.c_void_p(dl.data_ptr())
        assert lib.miseg_seg_loss_fwd(C.byref(p), ops._stream()) == SC.UNSUPPORTED
        assert lib.miseg_seg_loss_bwd(C.byref(p), ops._stream()) == SC.UNSUPPORTED
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in (ws, sums, dl, loss))
        taken, plain = [], crit.forward_torch
        crit.forward_torch = lambda a, b: taken.append(plain(a, b)) or taken[-1]
        got = crit(x, lab)
        crit.forward_torch = plain
        assert got.is_cuda and len(taken) == 1 and got is taken[0]       # what forward() returned is what forward_torch computed
        if kind != "dice_ce":      # F.cross_entropy over [B, C, S] adds its terms with atomics on the device: two calls may differ in the last bit
            assert torch.equal(got, plain(x, lab))
        if Cc > 1:      # and forward_torch on the device is the judge's loss to fp32 precision (a single channel is always kept: not the judge's rule)
            want = R.loss(x.cpu().double(), lab.cpu(), SC._BASE[kind])
            assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want)), (kind, float(got), float(want))
        xin = x.clone().requires_grad_(True)
        crit(xin, lab).backward()
        assert bool(torch.isfinite(xin.grad).all())


# ------------------------------------------------------------------------------------------------ the metric
def make_metric_inputs(case):
    """(fp32 logits [B, C, S], int64 labels [B, 1, S]) on the CPU"""
    g = torch.Generator().manual_seed(zlib.crc32(case.id.encode()))
    B, Cc, S = case.B, case.C, case.S
    x = torch.randn(B, Cc, S, generator=g)
    lab = torch.randint(0, Cc, (B, 1, S), generator=g)
    if case.logits in ("ties", "first_last"):
        x = torch.round(2.0 * x)                          # a handful of integer values: exact ties at the maximum are the rule
        if case.logits == "first_last":
            x[:, 0, ::3] = 50.0
            x[:, Cc - 1, ::3] = 50.0                      # the first and the last channel tie: class 0 wins
    else:
        x = 3.0 * x
        x[:, Cc - 1, ::1000] = x[:, 0, ::1000]
    if case.labels == "never":
        lab[lab == Cc - 1] = 0                            # the last class is never labelled
        x[:, 0] = -100.0                                  # class 0 is never predicted
    elif case.labels == "out_of_range":
        lab[0, 0, ::7] = 255 if case.label_dtype == "U8" else -1
        lab[-1, 0, 3::11] = Cc
        if case.label_dtype in ("I32", "I64"):
            lab[0, 0, 5::13] = 2 ** 31 - 1 if case.label_dtype == "I32" else Cc + 1000
    return x, lab


METRIC_GUARD, METRIC_FILL = 32, -0x0123456789ABCDEF


@pytest.mark.parametrize("case", SC.METRIC_CASES, ids=[c.id for c in SC.METRIC_CASES])
def test_dice_metric_case(case):
    """miseg_dice_metric through the C ABI with a counts buffer the test owns: the integer counts exactly, the per-class Dice (NaN pattern
    included) and the generalized score of every (include_background, weight type) at test_dice_metric_kernel's bars against the judge"""
    L, ops = _mods()
    lib = L.load()
    B, Cc, S = case.B, case.C, case.S
    x, lab = make_metric_inputs(case)
    want_counts = R.metric_counts(x, R.one_hot(lab, Cc, torch.int64))
    if case.labels == "out_of_range":
        assert int(want_counts[..., 2].sum()) < B * S and int(want_counts[..., 1].sum()) == B * S
    if case.labels == "never":
        assert int(want_counts[:, 0, 1].sum()) == 0 and int(want_counts[:, Cc - 1, 2].sum()) == 0
    if case.logits == "first_last":
        assert int(want_counts[:, 0, 1].min()) >= (S + 2) // 3
    want_dice = R.dice_of_counts(want_counts)
    xd, ld = x.to(DEV), lab.to(SC.LABEL_DTYPES[case.label_dtype]).to(DEV)
    n = B * Cc * 3
    buf = torch.full((n + 2 * METRIC_GUARD,), METRIC_FILL, dtype=torch.int64, device=DEV)
    counts = buf[METRIC_GUARD:METRIC_GUARD + n]
    combos = [(inc, w) for inc in (True, False) for w in R.W_TYPES] if S < (1 << 20) else [(False, "square"), (True, "simple")]
    for inc, w_type in combos:
        dice = torch.full((B * Cc + 2,), -7.0, dtype=torch.float32, device=DEV)
        score = torch.full((B + 2,), -7.0, dtype=torch.float32, device=DEV)
        p = L.DiceMetric(C.sizeof(L.DiceMetric), xd.data_ptr(), ld.data_ptr(), ops._label(ld)[1], B, Cc, S, counts.data_ptr(), dice.data_ptr() + 4,
                         score.data_ptr() + 4, int(inc), ops.gdice_weight_type(w_type))
        L.check(lib.miseg_dice_metric(C.byref(p), ops._stream()), "dice_metric")
        torch.cuda.synchronize()
        assert bool((buf[:METRIC_GUARD] == METRIC_FILL).all()) and bool((buf[METRIC_GUARD + n:] == METRIC_FILL).all())
        assert dice[0] == -7.0 and dice[-1] == -7.0 and score[0] == -7.0 and score[-1] == -7.0
        got_counts = counts.cpu().reshape(B, Cc, 3)
        assert torch.equal(got_counts, want_counts), (case.id, (got_counts - want_counts).nonzero()[:8].tolist())
        got = dice[1:-1].cpu().double().reshape(B, Cc)
        assert torch.equal(torch.isnan(got), torch.isnan(want_dice))
        ok = ~torch.isnan(want_dice)
        assert torch.allclose(got[ok], want_dice[ok], rtol=1e-6, atol=0)
        want_score = R.generalized_score_of_counts(want_counts, inc, w_type)
        assert torch.allclose(score[1:-1].cpu().double(), want_score, rtol=1e-6, atol=0), (case.id, inc, w_type, score[1:-1].tolist(), want_score.tolist())
    if case.labels == "never":
        assert bool(torch.isnan(want_dice[:, Cc - 1]).all())
    # the entry point every caller uses: the same Dice, bit for bit
    plain = ops.dice_metric(xd, ld)
    assert torch.equal(torch.nan_to_num(plain, nan=-1.0), torch.nan_to_num(dice[1:-1].reshape(B, Cc), nan=-1.0))
