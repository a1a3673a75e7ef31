"""The rules of the fused optimiser's gradient clipping, without a GPU: the numpy restatement tests/grad_clip_ref.py (which the GPU tests
hold the kernels to) against torch.nn.utils.clip_grad_norm_ / clip_grad_value_ in float64, the command-line flags and the refusals."""
import argparse

import numpy as np
import pytest
import torch

import grad_clip_ref as R

SHAPES = [(48, 48, 3, 3, 3), (7,), (4097,), (4096,), (4095,), (3, 5), (1,), (96, 33)]
NONE = {1, 5}          # parameters with `grad is None` (an absent modality's norm rows)


def _params(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    ps = []
    for i, s in enumerate(SHAPES):
        p = torch.nn.Parameter(torch.zeros(*s, dtype=torch.float64))
        if i not in NONE:
            p.grad = torch.randn(*s, generator=g, dtype=torch.float64) * scale
        ps.append(p)
    return ps


def _grads(ps):
    return [None if p.grad is None else p.grad.detach().numpy().copy() for p in ps]


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


@pytest.mark.parametrize("max_norm", [0.5, 12.0, 1e6])       # clips hard, clips, does not clip
@pytest.mark.parametrize("scale", [1.0, 1e-3])
def test_norm_clipping_restatement_matches_torch_in_float64(max_norm, scale):
    ps = _params(3, scale)
    grads = _grads(ps)
    want_norm = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
    got, norm, coef = R.clip_by_norm(grads, max_norm, dtype=np.float64)
    assert abs(float(norm) - want_norm) <= 1e-12 * want_norm
    assert (coef < 1) == (want_norm + 1e-6 > max_norm)
    for i, (p, g) in enumerate(zip(ps, got)):
        assert (p.grad is None) == (g is None) == (i in NONE)
        if g is not None:
            assert _rel(g, p.grad.numpy()) <= 1e-12, i
    pn = R.param_norms(grads, dtype=np.float64)
    for i, g in enumerate(grads):
        want = 0.0 if g is None else float(torch.linalg.vector_norm(torch.from_numpy(g)))
        assert abs(float(pn[i]) - want) <= 1e-12 * max(want, 1e-300)


@pytest.mark.parametrize("clip", [0.25, 1.0, 100.0])
def test_value_clipping_restatement_matches_torch_in_float64(clip):
    ps = _params(4)
    grads = _grads(ps)
    torch.nn.utils.clip_grad_value_(ps, clip)
    got = R.clip_by_value(grads, clip, dtype=np.float64)
    for i, (p, g) in enumerate(zip(ps, got)):
        assert (p.grad is None) == (g is None)
        if g is not None:
            assert _rel(g, p.grad.numpy()) <= 1e-12, i
    x = np.array([np.nan, -3.0, 3.0, 0.5, np.inf, -np.inf])
    want = torch.clamp(torch.from_numpy(x), -1.0, 1.0).numpy()
    np.testing.assert_array_equal(R.clip_by_value([x], 1.0, dtype=np.float64)[0], want)          # a NaN stays a NaN


def test_float32_coefficient_is_torchs_float32_arithmetic():
    """clip_grad_norm_'s rule on float32 tensors: max_norm / (norm + 1e-6) clamped to 1, each operation rounded in float32.  The quotient
    is the correctly rounded one (tensor / tensor); torch's `python_scalar / tensor` spelling evaluates reciprocal-then-multiply, which can
    differ from it in the last place - the kernels and the restatement use the quotient."""
    for norm, max_norm in [(3.7, 1.0), (0.0, 1.0), (12.000001, 12.0), (1e30, 1e-3), (0.3, 1.0), (np.inf, 5.0)]:
        t = torch.tensor(norm, dtype=torch.float32)
        want = torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (t + 1e-6), max=1.0)
        got = R.clip_coef(np.float32(norm), max_norm)
        assert got.dtype == np.float32 and got == want.numpy(), (norm, max_norm)
    assert R.clip_coef(np.float32(np.nan), 1.0) == 1.0


def test_record_and_skip_rule():
    g = [np.ones(4, dtype=np.float32) * 3, None, np.array([4.0], dtype=np.float32)]
    r = R.record(g, "norm", 1.0)
    assert r["norm"] == np.float32(np.sqrt(52.0)) and r["coef"] < 1 and r["finite"] == 1 and r["skip"] == 0 and (r["seen"], r["clipped"], r["skipped"]) == (1, 1, 0)
    bad = [np.array([1.0, np.inf], dtype=np.float32)]
    r2 = R.record(bad, "norm", 1.0, skip_nonfinite=True, prev=r)
    assert r2["finite"] == 0 and r2["skip"] == 1 and r2["coef"] == 0 and (r2["seen"], r2["clipped"], r2["skipped"]) == (2, 2, 1)
    r3 = R.record([np.array([np.nan], dtype=np.float32)], "norm", 1.0, skip_nonfinite=False, prev=r2)
    assert r3["finite"] == 0 and r3["skip"] == 0 and r3["coef"] == 1 and r3["skipped"] == 1
    assert R.record([None, None])["norm"] == 0 and R.record([None], "norm", 2.0)["coef"] == 1
    # squares that leave float32's range stay inside float64's
    assert R.total_norm([np.full(5, 1e-30, dtype=np.float32)]) > 0 and np.isfinite(R.total_norm([np.full(5, 1e30, dtype=np.float32)]))


def test_trainer_flags_and_their_defaults():
    from mi_seg_amd.utils import parser as P
    p = P.add_trainer_argparse_args(argparse.ArgumentParser())
    a = p.parse_args([])
    assert a.gradient_clip_val is None and a.gradient_clip_algorithm == "norm" and a.track_grad_norm == -1 and a.skip_nonfinite_steps is False
    a = p.parse_args(["--gradient_clip_val", "12", "--gradient_clip_algorithm", "value", "--track_grad_norm", "2", "--skip_nonfinite_steps"])
    assert a.gradient_clip_val == 12.0 and a.gradient_clip_algorithm == "value" and a.track_grad_norm == 2 and a.skip_nonfinite_steps is True
    for bad in (["--gradient_clip_algorithm", "l1"], ["--track_grad_norm", "1"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    # the other tables do not define them: a script that adds Lightning's own Trainer arguments beside them does not collide
    q = P.add_tune_argparse_args(P.add_data_argparse_args(P.add_model_argparse_args(argparse.ArgumentParser())))
    assert not any(hasattr(q.parse_args([]), k) for k in ("gradient_clip_val", "gradient_clip_algorithm", "track_grad_norm", "skip_nonfinite_steps"))
    P.add_trainer_argparse_args(q)          # ... and can be added beside them


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """every call below is wrong in exactly one way and must come back MISEG_E_BADARG (-1) from the host-side checks: nothing is launched,
    so the stand-in addresses are never read"""
    import ctypes as C
    from mi_seg_amd.hip import lib as L
    so = L.load()
    A = 1 << 20          # a stand-in for device buffers (8-byte aligned)
    assert so.miseg_grad_norm_workspace_bytes(10, 3) == 13 * 8 and so.miseg_grad_norm_workspace_bytes(0, 3) == 0
    assert C.sizeof(L.GradClipRecord) == 32

    def norm_params(**kw):
        d = dict(struct_size=C.sizeof(L.GradNorm), mode=L.CLIP_NORM, descs_dev=A, ndesc=1, total_blocks=1, grad=A, used=A, max_norm=1.0,
                 skip_nonfinite=0, workspace=A, record=A, per_param=None)
        d.update(kw)
        return L.GradNorm(**d)

    bad_norm = [dict(struct_size=C.sizeof(L.GradNorm) - 8), dict(descs_dev=None), dict(grad=None), dict(workspace=None), dict(record=None), dict(ndesc=0),
                dict(total_blocks=0), dict(mode=3), dict(mode=-1), dict(max_norm=0.0), dict(max_norm=-2.0), dict(max_norm=float("inf")),
                dict(max_norm=float("nan"))]
    for kw in bad_norm:
        assert so.miseg_grad_norm(C.byref(norm_params(**kw)), None) == -1, kw
    assert so.miseg_grad_norm(None, None) == -1

    step = L.OptStep(C.sizeof(L.OptStep), L.OPT_ADAMW, A, 1, 1, A, A, A, A, A, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, None, None, None, -1)
    bad_clip = [(A, 3, 1.0), (A, -1, 1.0), (None, L.CLIP_NORM, 1.0), (None, L.CLIP_NONE, 1.0), (A, L.CLIP_VALUE, 0.0), (None, L.CLIP_VALUE, -1.0),
                (A, L.CLIP_VALUE, float("inf")), (None, L.CLIP_VALUE, float("nan"))]
    for rec, mode, val in bad_clip:
        assert so.miseg_opt_step_clipped(C.byref(step), rec, mode, val, None) == -1, (rec, mode, val)
        assert so.miseg_opt_step_pack_conv3_clipped(C.byref(step), A, A, 1, 1, L.F32, None, rec, mode, val, None) == -1, (rec, mode, val)
    short = L.OptStep.from_buffer_copy(bytes(step))
    short.struct_size -= 8
    assert so.miseg_opt_step_clipped(C.byref(short), A, L.CLIP_NORM, 1.0, None) == -1 and b"struct_size" in so.miseg_last_error()
    assert so.miseg_opt_step_pack_conv3_clipped(C.byref(short), A, A, 1, 1, L.F32, None, A, L.CLIP_NORM, 1.0, None) == -1
    assert so.miseg_opt_step_clipped(None, A, L.CLIP_NORM, 1.0, None) == -1
    nograd = L.OptStep.from_buffer_copy(bytes(step))
    nograd.grad = None
    assert so.miseg_opt_step_clipped(C.byref(nograd), A, L.CLIP_NORM, 1.0, None) == -1
    assert so.miseg_opt_step_pack_conv3_clipped(C.byref(nograd), A, A, 1, 1, L.F32, None, A, L.CLIP_NORM, 1.0, None) == -1


def test_optimizer_refuses_bad_clipping_arguments():
    from mi_seg_amd.hip import lib as L
    from mi_seg_amd.training.optim import ArenaOptimizer, clip_options
    for kw in (dict(gradient_clip_algorithm="l1"), dict(gradient_clip_val=0.0), dict(gradient_clip_val=-1.0), dict(gradient_clip_val=float("inf")),
               dict(gradient_clip_val=float("nan")), dict(track_grad_norm=1)):
        with pytest.raises(ValueError):
            clip_options(**kw)
        with pytest.raises(ValueError):
            ArenaOptimizer(None, **kw)          # refused before the arena is looked at
    assert clip_options() == (L.CLIP_NONE, 0.0, False, False)
    assert clip_options(12, "norm", True, 2) == (L.CLIP_NORM, 12.0, True, True)
    assert clip_options(0.5, "value", False, -1) == (L.CLIP_VALUE, 0.5, False, False)
    assert clip_options(None, "value") == (L.CLIP_NONE, 0.0, False, False)
