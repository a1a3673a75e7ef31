"""The rules of gradient accumulation over micro-batches, without a GPU: the numpy restatement tests/grad_accum_ref.py (which the GPU tests hold
the kernel to) against torch autograd in float64, its float32 bits against the reference's scale-then-sum, the command-line flags and the
refusals of the C entry point."""
import argparse

import numpy as np
import pytest
import torch

import grad_accum_ref as R


class _MLP(torch.nn.Module):
    """two layers with one bias row per style in between: a micro-batch touches the row of its own style only, the other keeps `grad is None`"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.w1 = torch.nn.Parameter(torch.randn(6, 4, generator=g, dtype=torch.float64))
        self.rows = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(6, generator=g, dtype=torch.float64)) for _ in range(3)])
        self.w2 = torch.nn.Parameter(torch.randn(2, 6, generator=g, dtype=torch.float64))

    def forward(self, x, style):
        return torch.tanh(x @ self.w1.t() + self.rows[style]) @ self.w2.t()


def _micro_batches(k, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(5, 4, generator=g, dtype=torch.float64), torch.randn(5, 2, generator=g, dtype=torch.float64)) for _ in range(k)]


# styles per micro-batch: every row used; one only first; only last; only in the middle; style 2 never
@pytest.mark.parametrize("styles", [[0], [0, 0], [0, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0, 0], [1, 0, 0, 1], [0, 1, 1, 0]])
def test_restatement_is_the_mean_gradient_torch_accumulates_in_float64(styles):
    k = len(styles)
    m = _MLP()
    params = list(m.parameters())
    data = _micro_batches(k, 9)
    # the reference's loop (utils/trainer.py:33-78): every loss divided by k, backward() accumulating in p.grad
    for (x, y), s in zip(data, styles):
        (torch.nn.functional.mse_loss(m(x, s), y) / k).backward()
    want = [None if p.grad is None else p.grad.detach().numpy().copy() for p in params]
    # the restatement on every micro-batch's own, unscaled gradient
    grads, used = [], []
    for (x, y), s in zip(data, styles):
        gs = torch.autograd.grad(torch.nn.functional.mse_loss(m(x, s), y), params, allow_unused=True)
        grads.append([None if t is None else t.numpy().copy() for t in gs])
        used.append([t is not None for t in gs])
    mean, union = R.window(grads, used, k, dtype=np.float64)
    assert union == [w is not None for w in want]
    assert params[4] is m.rows[2] and not union[4]          # style 2's row: absent from every window
    for i, (got, w) in enumerate(zip(mean, want)):
        assert (got is None) == (w is None), i
        if w is not None:
            assert got.dtype == np.float64
            assert float(np.max(np.abs(got - w))) <= 1e-12 * float(np.max(np.abs(w))), i


@pytest.mark.parametrize("k", [2, 4])
def test_float32_bits_equal_scale_then_sum_for_a_power_of_two(k):
    """sum-then-scale (the kernel) against the reference's scale-then-sum ((g1/k + g2/k) + ...): dividing by a power of two is exact, so the
    two orders round alike and give equal bits"""
    rng = np.random.default_rng(3)
    grads = [[(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4)).astype(np.float32) for n in (4097, 7, 1)] for _ in range(k)]
    used = [[True, j != 1, j == k - 1] for j in range(k)]          # always; all but micro-batch 1; the last only
    mean, union = R.window(grads, used, k)
    assert union == [True, True, True]
    kk = np.float32(k)
    for i in range(3):
        want = None
        for j in range(k):
            if used[j][i]:
                t = grads[j][i] / kk
                want = t if want is None else (want + t).astype(np.float32)
        assert mean[i].dtype == np.float32
        np.testing.assert_array_equal(mean[i].view(np.int32), want.view(np.int32))


def test_a_short_window_still_divides_by_k():
    g = [[np.array([3.0, -1.5], dtype=np.float32)], [np.array([1.0, 0.25], dtype=np.float32)]]
    mean, _ = R.window(g, [[True], [True]], 3)
    np.testing.assert_array_equal(mean[0], ((g[0][0] + g[1][0]) * (np.float32(1) / np.float32(3))).astype(np.float32))


def test_the_table_of_reads_and_writes():
    """ops 0, 2, 4 touch nothing; 1 and 5 never read acc; 6 never reads the arena; a closing fold writes the arena, another one acc"""
    assert [R.reads(op) for op in range(8)] == [(False, False), (True, False), (False, False), (True, True), (False, False), (True, False), (False, True),
                                                (True, True)]
    assert [R.writes(op) for op in range(8)] == [(False, False), (False, True), (False, False), (False, True), (False, False), (True, False), (True, False),
                                                 (True, False)]
    nan = np.array([np.nan], dtype=np.float32)
    one = np.array([1.0], dtype=np.float32)
    for op in (0, 2, 4):
        acc, g = R.fold([nan], [nan], [op], 0.5)
        assert acc[0] is nan and g[0] is nan
    acc, g = R.fold([nan], [one], [1], 0.5)
    assert acc[0] == 1 and g[0] is one
    acc, g = R.fold([nan], [one], [5], 0.5)
    assert acc[0] is nan and g[0] == 0.5
    acc, g = R.fold([one], [nan], [6], 0.5)
    assert acc[0] is one and g[0] == 0.5
    acc, g = R.fold([one], [one], [7], 0.5)
    assert acc[0] is one and g[0] == 1.0
    acc, g = R.fold([one], [one], [3], 0.5)
    assert acc[0] == 2.0 and g[0] is one
    assert R.op_codes([True, False, True, False], [True, True, False, False], True) == [7, 6, 5, 4]
    assert R.op_codes([True, False, True, False], [True, True, False, False], False) == [3, 2, 1, 0]


def test_flags_and_their_defaults():
    from mi_seg_amd.utils import parser as P
    p = P.add_tune_argparse_args(P.add_trainer_argparse_args(argparse.ArgumentParser()))
    a = p.parse_args([])
    assert a.accumulate_grad_batches == 1 and a.iters_to_accumulate == 1 and P.accumulation_steps(a) == 1
    assert P.accumulation_steps(p.parse_args(["--accumulate_grad_batches", "4"])) == 4
    assert P.accumulation_steps(p.parse_args(["--iters_to_accumulate", "3"])) == 3          # the reference's own flag, when Lightning's is not given
    assert P.accumulation_steps(p.parse_args(["--accumulate_grad_batches", "2", "--iters_to_accumulate", "2"])) == 2
    assert P.accumulation_steps(p.parse_args(["--accumulate_grad_batches", "2", "--iters_to_accumulate", "1"])) == 2
    with pytest.raises(ValueError, match="disagree"):
        P.accumulation_steps(p.parse_args(["--accumulate_grad_batches", "2", "--iters_to_accumulate", "3"]))
    for bad in (["--accumulate_grad_batches", "0"], ["--accumulate_grad_batches", "-2"], ["--accumulate_grad_batches", "1.5"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    # a namespace without either flag, a dict (LitMonai's kwargs), and counts that are no counts
    assert P.accumulation_steps(argparse.Namespace()) == 1 and P.accumulation_steps({"accumulate_grad_batches": 8}) == 8
    assert P.accumulation_steps({"accumulate_grad_batches": None, "iters_to_accumulate": 2}) == 2
    for bad in ({"accumulate_grad_batches": 0}, {"iters_to_accumulate": -1}, {"accumulate_grad_batches": 2.5}, {"accumulate_grad_batches": True}):
        with pytest.raises(ValueError):
            P.accumulation_steps(bad)
    # only the trainer table defines Lightning's flag
    q = P.add_tune_argparse_args(P.add_data_argparse_args(P.add_model_argparse_args(argparse.ArgumentParser())))
    assert not hasattr(q.parse_args([]), "accumulate_grad_batches")


def test_accumulator_refuses_a_count_below_one_and_is_inert_at_one():
    from mi_seg_amd.training.optim import GradAccumulator, accumulation_scale
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            GradAccumulator(None, bad)          # refused before the optimiser is looked at
    acc = GradAccumulator(None, 1)
    assert not acc.active and acc.plan() is True and acc.closes() is True and acc.acc is None and acc.ops is None
    acc.prepare()
    acc.fold()                                   # no buffer, no launch: the optimiser (None here) is never touched
    acc.reset()
    assert acc.acc is None
    for k in (2, 3, 4, 7):
        assert np.float32(accumulation_scale(k)) == R.scale_of(k) and GradAccumulator(None, k).scale == accumulation_scale(k)


def test_lit_monai_resolves_the_count_from_its_kwargs():
    from mi_seg_amd.networks.lightning_monai import LitMonai
    net = torch.nn.Linear(2, 2)
    assert LitMonai(net, 2).accumulation_steps == 1
    assert LitMonai(net, 2, accumulate_grad_batches=4).accumulation_steps == 4
    assert LitMonai(net, 2, iters_to_accumulate=2, accumulate_grad_batches=1).accumulation_steps == 2
    with pytest.raises(ValueError):
        LitMonai(net, 2, iters_to_accumulate=2, accumulate_grad_batches=3).accumulation_steps


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """every call below is wrong in exactly one way and must come back MISEG_E_BADARG (-1) from the host-side checks: nothing is launched,
    so the stand-in addresses are never read"""
    import ctypes as C
    from mi_seg_amd.hip import lib as L
    so = L.load()
    A, B = 1 << 20, 1 << 24          # stand-ins for device buffers (16-byte aligned, 16 MiB apart)
    n = 1 << 20                      # elements: [A, A + 4 MiB) and [B, B + 4 MiB) do not meet
    assert so.miseg_abi_struct_size(b"miseg_grad_fold_params") == C.sizeof(L.GradFold)
    assert (L.FOLD_USED, L.FOLD_EARLIER, L.FOLD_CLOSE) == (R.U, R.A, R.F)

    def params(**kw):
        d = dict(struct_size=C.sizeof(L.GradFold), descs_dev=A, ndesc=1, total_blocks=1, grad=A, acc=B, ops=A, arena_elems=n, scale=0.5)
        d.update(kw)
        return L.GradFold(**d)

    bad = [dict(struct_size=C.sizeof(L.GradFold) - 8), dict(struct_size=0), dict(descs_dev=None), dict(grad=None), dict(acc=None), dict(ops=None),
           dict(ndesc=0), dict(ndesc=-3), dict(total_blocks=0), dict(arena_elems=0),
           dict(scale=0.0), dict(scale=-0.5), dict(scale=float("inf")), dict(scale=float("nan")),
           dict(acc=A), dict(acc=A + 16), dict(acc=A + 4 * n - 16), dict(grad=B + 4 * n - 16),          # the two ranges overlap
           dict(grad=A + 4), dict(acc=B + 8), dict(ops=A + 2)]                                           # misaligned
    for kw in bad:
        assert so.miseg_grad_fold(C.byref(params(**kw)), None) == -1, kw
        assert b"grad_fold" in so.miseg_last_error(), kw
    assert so.miseg_grad_fold(None, None) == -1
    assert so.miseg_grad_fold(C.byref(params(struct_size=C.sizeof(L.GradFold) - 8)), None) == -1 and b"struct_size" in so.miseg_last_error()
    assert so.miseg_grad_fold(C.byref(params(acc=A + 4 * n - 16)), None) == -1 and b"overlap" in so.miseg_last_error()
