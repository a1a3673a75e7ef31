"""One host-side plan per 3x3x3 launch (miseg_conv3_fwd_plan / miseg_conv3_wgrad_plan, ABI 13): every distinct conv launch shape of the
bench nets - C-Swin-UNETR fs=48 and C-UNETR at 96^3, the plain UNet - in both directions of the convolution kernel (forward and data
gradient) and the weight gradient, bf16 and fp32, with 16-byte aligned operands.  Kernel, splits and fold answers are what the shape-only
entry points of ABI 12 answered for these shapes; a forward workspace is now exactly the slabs of the plan's splits (ABI 12 sized it from the
split before rounding, up to a third more), a weight-gradient workspace exactly what the chosen kernel writes.  Misaligned operands leave the
kernels and folds that need alignment.  CPU only: the plans touch no device."""
import ctypes as C

import pytest


def _L():
    from mi_seg_amd.hip import lib
    return lib


A = 1 << 12      # an aligned stand-in address: the plans read pointers for NULL and alignment only


def _fwd(dt, S, Cin, Cout, x=A, ldx=None, sc_x=A, ld_sc_x=None, **more):
    L = _L()
    p = L.Conv3(x, ldx or Cin, A, Cout, A, 1, S, S, S, Cin, Cout, dt)
    p.sc_x, p.ld_sc_x, p.sc_w, p.sc_C = sc_x, ld_sc_x or Cin, A, Cin
    p.s2c_out, p.s2c_C = A, Cout // 2
    p.fs_w, p.fs_y, p.ld_fs_y = A, A, Cout
    for k, v in more.items():
        setattr(p, k, v)
    plan = L.Conv3Plan()
    assert L.load().miseg_conv3_fwd_plan(C.byref(p), C.byref(plan)) == 0
    return plan


def _wgrad(dt, S, Cin, Cout, x=A, ldx=None):
    L = _L()
    p = L.Conv3Wgrad(x, ldx or Cin, A, Cout, A, 1, S, S, S, Cin, Cout, dt, 0, None, 0)
    plan = L.Conv3WgradPlan()
    assert L.load().miseg_conv3_wgrad_plan(C.byref(p), C.byref(plan)) == 0
    return plan


class _Consts:
    def __getattr__(self, name):
        return getattr(_L(), name)


L = _Consts()      # (the table names the kernel constants of hip/lib.py; the binding loads when a test runs)

FWD_ROWS = [      # (dtype, S, Cin, Cout, kernel, splits, what miseg_conv3_fwd_workspace_bytes said before, sc, s2c, fs)
    (1, 96, 16, 16, L.CONV3_FWD96, 1, 0, 0, 0, 0),
    (1, 96, 16, 32, L.CONV3_FWD96, 1, 0, 0, 0, 0),
    (1, 96, 32, 16, L.CONV3_FWD96, 1, 0, 0, 0, 0),
    (1, 96, 48, 48, L.CONV3_FWD96, 1, 0, 1, 0, 1),
    (1, 96, 48, 96, L.CONV3_FWD96, 1, 0, 1, 1, 1),
    (1, 96, 96, 48, L.CONV3_FWD96, 1, 0, 1, 0, 1),
    (1, 48, 32, 32, L.CONV3_FWD96, 1, 0, 0, 0, 0),
    (1, 48, 32, 64, L.CONV3_FWD96, 1, 0, 0, 0, 0),
    (1, 48, 48, 48, L.CONV3_FWD96, 1, 0, 1, 0, 1),
    (1, 48, 48, 96, L.CONV3_FWD96, 1, 0, 1, 1, 1),
    (1, 48, 64, 32, L.CONV3_FWD96, 1, 0, 0, 0, 0),
    (1, 48, 96, 48, L.CONV3_FWD96, 1, 0, 1, 0, 1),
    (1, 24, 32, 32, L.CONV3_FWD96, 1, 0, 0, 1, 0),
    (1, 24, 64, 64, L.CONV3_FWD96, 1, 0, 0, 1, 0),
    (1, 24, 64, 128, L.CONV3_FWD96, 1, 0, 0, 1, 0),
    (1, 24, 96, 96, L.CONV3_FWD96, 1, 0, 1, 1, 1),
    (1, 24, 96, 192, L.CONV3_FWD96, 1, 0, 1, 1, 1),
    (1, 24, 128, 64, L.CONV3_FWD96, 1, 0, 0, 1, 0),
    (1, 24, 192, 96, L.CONV3_FWD96, 1, 0, 1, 1, 1),
    (1, 12, 128, 128, L.CONV3_FWD96, 4, 3538944, 0, 0, 0),
    (1, 12, 128, 256, L.CONV3_FWD96, 4, 7077888, 0, 0, 0),
    (1, 12, 192, 192, L.CONV3_FWD96, 4, 5308416, 0, 0, 0),
    (1, 12, 192, 384, L.CONV3_FWD96, 2, 7962624, 0, 0, 0),
    (1, 12, 256, 128, L.CONV3_FWD96, 8, 7077888, 0, 0, 0),
    (1, 12, 256, 256, L.CONV3_FWD96, 4, 7077888, 0, 0, 0),
    (1, 12, 384, 192, L.CONV3_FWD96, 4, 6635520, 0, 0, 0),
    (1, 6, 384, 384, L.CONV3_FWD_TINY, 8, 2654208, 0, 0, 0),
    (1, 6, 384, 768, L.CONV3_FWD_TINY, 8, 5308416, 0, 0, 0),
    (1, 6, 768, 384, L.CONV3_FWD_TINY, 16, 5308416, 0, 0, 0),
    (1, 3, 768, 768, L.CONV3_FWD_TINY, 16, 1327104, 0, 0, 0),
    (0, 96, 16, 16, L.CONV3_FWD96, 1, 0, 0, 0, 0),
    (0, 96, 16, 32, L.CONV3_FWD96, 1, 0, 0, 0, 0),
    (0, 96, 32, 16, L.CONV3_FWD96, 1, 0, 0, 0, 0),
    (0, 96, 48, 48, L.CONV3_FWD96, 1, 0, 0, 0, 0),
    (0, 96, 48, 96, L.CONV3_FWD96, 1, 0, 0, 1, 0),
    (0, 96, 96, 48, L.CONV3_FWD96, 1, 0, 0, 0, 0),
    (0, 48, 32, 32, L.CONV3_FWD96, 1, 0, 0, 0, 0),
    (0, 48, 32, 64, L.CONV3_FWD96, 1, 0, 0, 0, 0),
    (0, 48, 48, 48, L.CONV3_FWD96, 1, 0, 0, 0, 0),
    (0, 48, 48, 96, L.CONV3_FWD96, 1, 0, 0, 1, 0),
    (0, 48, 64, 32, L.CONV3_FWD96, 1, 0, 0, 0, 0),
    (0, 48, 96, 48, L.CONV3_FWD96, 1, 0, 0, 0, 0),
    (0, 24, 32, 32, L.CONV3_FWD96, 2, 3538944, 0, 0, 0),
    (0, 24, 64, 64, L.CONV3_FWD96, 1, 0, 0, 1, 0),
    (0, 24, 64, 128, L.CONV3_FWD96, 1, 0, 0, 1, 0),
    (0, 24, 96, 96, L.CONV3_FWD96, 1, 0, 0, 1, 0),
    (0, 24, 96, 192, L.CONV3_FWD96, 1, 0, 0, 1, 0),
    (0, 24, 128, 64, L.CONV3_FWD96, 1, 0, 0, 1, 0),
    (0, 24, 192, 96, L.CONV3_FWD96, 1, 0, 0, 1, 0),
    (0, 12, 128, 128, L.CONV3_FWD96, 6, 5308416, 0, 0, 0),
    (0, 12, 128, 256, L.CONV3_FWD96, 3, 7077888, 0, 0, 0),
    (0, 12, 192, 192, L.CONV3_FWD96, 4, 6635520, 0, 0, 0),
    (0, 12, 192, 384, L.CONV3_FWD96, 3, 7962624, 0, 0, 0),
    (0, 12, 256, 128, L.CONV3_FWD96, 6, 7077888, 0, 0, 0),
    (0, 12, 256, 256, L.CONV3_FWD96, 4, 7077888, 0, 0, 0),
    (0, 12, 384, 192, L.CONV3_FWD96, 4, 6635520, 0, 0, 0),
    (0, 6, 384, 384, L.CONV3_FWD96, 16, 5308416, 0, 0, 0),
    (0, 6, 384, 768, L.CONV3_FWD96, 16, 10616832, 0, 0, 0),
    (0, 6, 768, 384, L.CONV3_FWD96, 32, 10616832, 0, 0, 0),
    (0, 3, 768, 768, L.CONV3_FWD96, 32, 2654208, 0, 0, 0),
]
WGRAD_ROWS = [      # (dtype, S, Cin, Cout, kernel, workspace bytes, what miseg_conv3_wgrad_workspace_bytes said before: an upper bound)
    (1, 96, 16, 16, L.CONV3_WGRAD_NARROW, 14155776, 63700992),
    (1, 96, 32, 16, L.CONV3_WGRAD_NARROW, 28311552, 63700992),
    (1, 96, 48, 48, L.CONV3_WGRAD_BF16, 63700992, 63700992),
    (1, 96, 96, 48, L.CONV3_WGRAD_BF16, 63700992, 63700992),
    (1, 48, 32, 32, L.CONV3_WGRAD_NARROW, 47775744, 63700992),
    (1, 48, 48, 48, L.CONV3_WGRAD_BF16, 63700992, 63700992),
    (1, 48, 64, 32, L.CONV3_WGRAD_BF16, 63700992, 63700992),
    (1, 48, 96, 48, L.CONV3_WGRAD_BF16, 63700992, 63700992),
    (1, 24, 32, 32, L.CONV3_WGRAD_NARROW, 5971968, 56623104),
    (1, 24, 64, 64, L.CONV3_WGRAD_BF16, 53747712, 63700992),
    (1, 24, 96, 96, L.CONV3_WGRAD_BF16, 53747712, 63700992),
    (1, 24, 128, 64, L.CONV3_WGRAD_BF16, 62705664, 62705664),
    (1, 24, 192, 96, L.CONV3_WGRAD_BF16, 63700992, 63700992),
    (1, 12, 128, 128, L.CONV3_WGRAD_BF16, 26873856, 53747712),
    (1, 12, 128, 256, L.CONV3_WGRAD_BF16, 53747712, 62705664),
    (1, 12, 192, 192, L.CONV3_WGRAD_BF16, 47775744, 63700992),
    (1, 12, 256, 128, L.CONV3_WGRAD_BF16, 53747712, 62705664),
    (1, 12, 256, 256, L.CONV3_WGRAD_BF16, 62705664, 62705664),
    (1, 12, 384, 192, L.CONV3_WGRAD_BF16, 63700992, 63700992),
    (1, 6, 384, 384, L.CONV3_WGRAD_TINY, 0, 47775744),
    (1, 6, 768, 384, L.CONV3_WGRAD_TINY, 0, 63700992),
    (1, 3, 768, 768, L.CONV3_WGRAD_TINY, 0, 63700992),
    (0, 96, 16, 16, L.CONV3_WGRAD_F32, 63700992, 63700992),
    (0, 96, 32, 16, L.CONV3_WGRAD_F32, 63700992, 63700992),
    (0, 96, 48, 48, L.CONV3_WGRAD_F32, 63700992, 63700992),
    (0, 96, 96, 48, L.CONV3_WGRAD_F32, 63700992, 63700992),
    (0, 48, 32, 32, L.CONV3_WGRAD_F32, 63700992, 63700992),
    (0, 48, 48, 48, L.CONV3_WGRAD_F32, 63700992, 63700992),
    (0, 48, 64, 32, L.CONV3_WGRAD_F32, 63700992, 63700992),
    (0, 48, 96, 48, L.CONV3_WGRAD_F32, 63700992, 63700992),
    (0, 24, 32, 32, L.CONV3_WGRAD_F32, 26873856, 56623104),
    (0, 24, 64, 64, L.CONV3_WGRAD_F32, 63700992, 63700992),
    (0, 24, 96, 96, L.CONV3_WGRAD_F32, 63700992, 63700992),
    (0, 24, 128, 64, L.CONV3_WGRAD_F32, 62705664, 62705664),
    (0, 24, 192, 96, L.CONV3_WGRAD_F32, 63700992, 63700992),
    (0, 12, 128, 128, L.CONV3_WGRAD_F32, 53747712, 53747712),
    (0, 12, 128, 256, L.CONV3_WGRAD_F32, 62705664, 62705664),
    (0, 12, 192, 192, L.CONV3_WGRAD_F32, 63700992, 63700992),
    (0, 12, 256, 128, L.CONV3_WGRAD_F32, 62705664, 62705664),
    (0, 12, 256, 256, L.CONV3_WGRAD_F32, 62705664, 62705664),
    (0, 12, 384, 192, L.CONV3_WGRAD_F32, 63700992, 63700992),
    (0, 6, 384, 384, L.CONV3_WGRAD_F32, 47775744, 47775744),
    (0, 6, 768, 384, L.CONV3_WGRAD_F32, 63700992, 63700992),
    (0, 3, 768, 768, L.CONV3_WGRAD_F32, 63700992, 63700992),
]


@pytest.mark.parametrize("row", FWD_ROWS, ids=lambda r: f"{'bf16' if r[0] else 'f32'}-{r[1]}^3-{r[2]}-{r[3]}")
def test_conv3_fwd_plan_of_the_bench_shapes(row):
    dt, S, Cin, Cout, kernel, splits, ws_before, sc, s2c, fs = row
    plan = _fwd(dt, S, Cin, Cout)
    assert (plan.kernel, plan.splits, plan.sc, plan.s2c, plan.fs) == (kernel, splits, sc, s2c, fs)
    assert plan.workspace_bytes == (splits * S ** 3 * Cout * 4 if splits > 1 else 0) and plan.workspace_bytes <= ws_before
    generic = kernel == L.CONV3_GENERIC
    both = _fwd(dt, S, Cin, Cout, res=A, stat=A)      # the fast path serves the residual and the statistics, the row-major kernel neither
    assert (both.res, both.stat) == (int(not generic), int(not generic))
    deferred = _fwd(dt, S, Cin, Cout, stat=A, defer_slabs=1)      # defer_slabs: a split launch only, and then no statistics
    assert (deferred.defer_slabs, deferred.stat) == (int(splits > 1), int(not generic and splits == 1))
    assert _fwd(dt, S, Cin, Cout, res=A, defer_slabs=1).defer_slabs == 0
    assert _fwd(dt, S, Cin, Cout, background=1).kernel == (L.CONV3_FWD96 if kernel == L.CONV3_FWD_TINY else kernel)


@pytest.mark.parametrize("row", WGRAD_ROWS, ids=lambda r: f"{'bf16' if r[0] else 'f32'}-{r[1]}^3-{r[2]}-{r[3]}")
def test_conv3_wgrad_plan_of_the_bench_shapes(row):
    dt, S, Cin, Cout, kernel, ws, ws_before = row
    plan = _wgrad(dt, S, Cin, Cout)
    assert (plan.kernel, plan.workspace_bytes) == (kernel, ws)
    assert (ws == 0) == (kernel == L.CONV3_WGRAD_TINY) and ws <= ws_before


def test_misaligned_operands_take_the_fallback_kernel_or_are_not_served():
    bf = 1
    # tiny forward (3^3 / 6^3): x one bf16 element off, or rows that are no multiple of 8 elements -> the 96-byte-chunk kernel, same splits
    for S, Cin, Cout in [(3, 768, 768), (6, 768, 384)]:
        ok = _fwd(bf, S, Cin, Cout)
        assert ok.kernel == L.CONV3_FWD_TINY
        for bad in (_fwd(bf, S, Cin, Cout, x=A + 2), _fwd(bf, S, Cin, Cout, ldx=Cin + 4)):
            assert (bad.kernel, bad.splits, bad.workspace_bytes) == (L.CONV3_FWD96, ok.splits, ok.workspace_bytes)
    # the shortcut term: sc_x one element off, or its rows no multiple of 8 elements -> not served; the second output needs an aligned x
    assert _fwd(bf, 24, 96, 96).sc == 1 and _fwd(bf, 24, 96, 96).fs == 1
    assert _fwd(bf, 24, 96, 96, sc_x=A + 2).sc == 0 and _fwd(bf, 24, 96, 96, ld_sc_x=100).sc == 0
    assert _fwd(bf, 24, 96, 96, sc_w=A + 2).sc == 0
    assert _fwd(bf, 24, 96, 96, x=A + 2).fs == 0 and _fwd(bf, 24, 96, 96, ldx=100).fs == 0
    assert _fwd(bf, 24, 96, 96, s2c_out=A + 2).s2c == 0
    # tiny and narrow weight gradients -> the bf16 slab kernel
    for S, Cin, Cout in [(3, 768, 768), (6, 384, 384)]:
        assert _wgrad(bf, S, Cin, Cout).kernel == L.CONV3_WGRAD_TINY
        assert _wgrad(bf, S, Cin, Cout, x=A + 2).kernel == L.CONV3_WGRAD_BF16
        assert _wgrad(bf, S, Cin, Cout, ldx=Cin + 4).kernel == L.CONV3_WGRAD_BF16
    for S, Cin, Cout in [(96, 16, 16), (48, 32, 32)]:
        assert _wgrad(bf, S, Cin, Cout).kernel == L.CONV3_WGRAD_NARROW
        bad = _wgrad(bf, S, Cin, Cout, ldx=Cin + 4)
        assert bad.kernel == L.CONV3_WGRAD_BF16 and bad.workspace_bytes > 0


def test_plans_refuse_bad_params():
    Lb = _L()
    plan = Lb.Conv3Plan()
    p = Lb.Conv3(A, 48, A, 48, A, 1, 8, 8, 8, 48, 48, 7)      # unknown dtype
    assert Lb.load().miseg_conv3_fwd_plan(C.byref(p), C.byref(plan)) == Lb.load().miseg_conv3_fwd_plan(None, C.byref(plan)) != 0
    w = Lb.Conv3Wgrad(A, 48, A, 48, A, 1, 0, 8, 8, 48, 48, 1, 0, None, 0)      # empty volume
    assert Lb.load().miseg_conv3_wgrad_plan(C.byref(w), C.byref(Lb.Conv3WgradPlan())) != 0
