"""numpy restatement of the gradient-clipping rules of the fused optimiser (include/miseg_hip.h: miseg_grad_norm, miseg_opt_step_clipped),
which restate torch.nn.utils.clip_grad_norm_ / clip_grad_value_ and add the non-finite step guard.

    total_norm(grads)          float32(sqrt(float64 sum of squares)) over the gradients that are not None
    clip_coef(norm, max_norm)  float32 min(1, max_norm / (norm + 1e-6)), every operation rounded in float32 (torch's rule)
    clip_by_norm / clip_by_value   the clipped gradients
    record(...)                what the device record holds after one call

`dtype=np.float64` (the CPU tests) carries every operation out in double, so that the rules themselves can be held against torch on
float64 parameters; the default float32 is what the kernels compute."""
import numpy as np


def sq_sum(grads):
    """float64 sum of squares over the gradients that are not None (a parameter with `grad is None` is left out, like torch does)"""
    s = np.float64(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for g in grads:
            if g is not None:
                s = s + np.sum(np.square(np.asarray(g, dtype=np.float64)), dtype=np.float64)
    return s


def total_norm(grads, dtype=np.float32):
    with np.errstate(over="ignore", invalid="ignore"):
        return dtype(np.sqrt(sq_sum(grads)))


def param_norms(grads, dtype=np.float32):
    """every tensor's own norm, 0 for one without a gradient (Lightning's track_grad_norm logs these)"""
    return np.array([total_norm([g], dtype) for g in grads], dtype=dtype)


def clip_coef(norm, max_norm, dtype=np.float32):
    """min(1, max_norm / (norm + 1e-6)); fminf's rule for a NaN norm: the coefficient is 1 (nothing is scaled; the guard decides about the step)"""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        c = dtype(max_norm) / (dtype(norm) + dtype(1e-6))
    return dtype(1.0) if np.isnan(c) else min(dtype(1.0), dtype(c))


def clip_by_norm(grads, max_norm, dtype=np.float32):
    """(clipped gradients, norm, coefficient): every gradient times the coefficient, one rounding per element"""
    norm = total_norm(grads, dtype)
    c = clip_coef(norm, max_norm, dtype)
    return [None if g is None else np.asarray(g, dtype=dtype) * c for g in grads], norm, c


def clip_by_value(grads, clip_value, dtype=np.float32):
    """g < -v ? -v : (g > v ? v : g): a NaN stays a NaN (torch.clamp)"""
    v = dtype(clip_value)
    out = []
    for g in grads:
        if g is None:
            out.append(None)
            continue
        g = np.asarray(g, dtype=dtype)
        out.append(np.where(g < -v, -v, np.where(g > v, v, g)).astype(dtype))
    return out


def record(grads, mode="none", max_norm=None, skip_nonfinite=False, prev=None):
    """the device record after one miseg_grad_norm call on `grads` (prev: the record before it, for the running counters)"""
    prev = prev or {"seen": 0, "clipped": 0, "skipped": 0}
    norm = total_norm(grads)
    coef = clip_coef(norm, max_norm) if mode == "norm" else np.float32(1.0)
    finite = int(np.isfinite(norm))
    skip = int(bool(skip_nonfinite) and not finite)
    return {"norm": norm, "coef": coef, "finite": finite, "skip": skip, "seen": prev["seen"] + 1, "clipped": prev["clipped"] + int(coef < 1),
            "skipped": prev["skipped"] + skip}
