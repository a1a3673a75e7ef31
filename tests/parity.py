"""Per-element parity of a kernel's output with its reference.

`conftest.rel_err` pools the error over the whole tensor: at the bf16 bar of 2e-2 it lets 4e-4 of a tensor's energy be completely wrong -
a lost tail row of a 5003-row GEMM (pooled 1.40e-2) or a zeroed corner voxel of a 9x13x19 convolution (1.35e-2) pass it.  `local_err`
holds every element to the scale the pooled bound already implies, plus the element's own magnitude:

    max_i |got_i - ref_i| / (|ref_i| + rms(ref))

so it needs no constant of its own: `assert_parity(got, ref, tol)` takes the tolerance the test already used for the pooled number and
asserts both.  An honest bf16 result (one round to nearest, at most 2^-8 of the value) sits near 3e-3; a lost row, voxel or tap group lands at 0.5 - 1.4.
tests/test_parity_metric_cpu.py pins these figures."""
import torch

from conftest import rel_err

_TINY = 1e-300      # keeps an all-zero reference from dividing by zero: 0 / tiny = 0, anything else / tiny fails every tolerance


def _errs(got, ref):
    """(float64 error tensor of ref's shape with non-finite reference entries masked to 0, got as float64, ref as float64) on got's device"""
    if tuple(got.shape) != tuple(ref.shape):
        raise AssertionError(f"shapes differ: got {tuple(got.shape)}, reference {tuple(ref.shape)}")
    g = got.detach().double()
    r = ref.detach().to(g.device).double()
    fin = torch.isfinite(r)
    r0 = torch.where(fin, r, torch.zeros_like(r))
    n = int(fin.numel())
    rms = (r0.square().sum() / max(n, 1)).sqrt()
    e = (g - r0).abs() / (r0.abs() + rms).clamp_min(_TINY)
    # a non-finite `got` against a finite reference is the largest error there is (NaN would lose every max)
    e = torch.where(torch.isfinite(g), e, torch.full_like(e, float("inf")))
    e = torch.where(fin, e, torch.zeros_like(e))
    return e, g, r


def _worst(e, g, r):
    """one device -> host transfer: (max error, flat index, got there, ref there, number of non-finite got where ref is finite)"""
    if e.numel() == 0:
        return 0.0, 0, 0.0, 0.0, 0
    ef = e.reshape(-1)
    val, idx = ef.max(dim=0)
    bad = (torch.isinf(ef)).sum()
    out = torch.stack([val, idx.double(), g.reshape(-1)[idx], r.reshape(-1)[idx], bad.double()]).tolist()
    return out[0], int(out[1]), out[2], out[3], int(out[4])


def _unravel(flat, shape):
    idx = []
    for s in reversed(shape):
        idx.append(flat % s)
        flat //= s
    return tuple(reversed(idx))


def local_err(got, ref):
    """(max_i |got_i - ref_i| / (|ref_i| + rms(ref)), unravelled index of the worst element); float64 on got's device, one synchronisation"""
    e, g, r = _errs(got, ref)
    val, flat, _, _, _ = _worst(e, g, r)
    return val, _unravel(flat, tuple(ref.shape))


def assert_parity(got, ref, tol, what="", local_tol=None):
    """got has no non-finite value where ref is finite, pooled rel_err < tol (as before) and local_err < tol; returns (pooled, local).
    A failure names `what`, both numbers, the worst element's index and the two values there.
    local_tol (never below tol): the bound of the local metric where an honest result exceeds tol there - max(tol, 2 x the local error of the
    torch composition in the compute dtype against the same float64 reference), computed in the test; the pooled check keeps tol."""
    if local_tol is None:
        local_tol = tol
    assert local_tol >= tol, (local_tol, tol)
    e, g, r = _errs(got, ref)
    loc, flat, gv, rv, bad = _worst(e, g, r)
    idx = _unravel(flat, tuple(ref.shape))
    pooled = rel_err(got.detach(), ref.detach())
    where = f"worst element {idx}: got {gv!r}, reference {rv!r}"
    assert bad == 0, f"{what}: {bad} non-finite value(s) where the reference is finite; {where}"
    assert pooled < tol and loc < local_tol, (f"{what}: pooled rel_err {pooled:.3e} (tolerance {tol:.3e}), local_err {loc:.3e} (tolerance {local_tol:.3e}); "
                                              f"{where}")
    return pooled, loc
