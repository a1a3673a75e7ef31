"""The pipelined bf16 loop of the 3x3x3 weight gradient (csrc/conv3d.hip::conv3_wgrad_body, PIPED) on the shapes where a loop that reads its
operands ahead of their MFMAs can go wrong - not the workload's shapes: one brick (nothing to prefetch from), volumes that are ragged in
every dimension (partial bricks whose rows beyond the volume are staged as zeros, the last tap of the last k-step), two input-channel
blocks, workgroups that walk several bricks with the next brick's global loads in flight under the reads, both accumulate modes, the
grouped launch in its normal and its background form, and bit-identical repeats.

Reference: torch.nn.grad.conv3d_weight in float64 on the bf16-rounded operands; helpers and the per-element tolerance are those of the
weight-gradient tests in tests/test_hip_kernels.py (assert_parity at TOL[bf16])."""
import functools

import pytest
import torch

from parity import assert_parity
from test_hip_kernels import DEV, TOL, _ops, rnd

pytestmark = pytest.mark.gpu

DT = torch.bfloat16
ONE_BRICK = (1, 4, 8, 8, 48, 48)
RAGGED = (1, 9, 10, 11, 48, 48)
TWO_CI_BLOCKS = (1, 8, 16, 16, 96, 48)
SEVERAL_BRICKS = (1, 12, 16, 16, 48, 48)      # 3 x 2 x 2 = 12 bricks
GROUP = [(1, 12, 12, 12, 96, 96), (1, 8, 16, 24, 48, 48), (1, 9, 10, 11, 48, 96)]      # 12^3: partial bricks along h and w


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(x, dy, float64 reference) of one layer, made once and shared by the tests that need it (nobody writes to them)"""
    B, D, H, W, Cin, Cout = shape
    x = rnd(B, D, H, W, Cin, dtype=DT, seed=701)
    dy = rnd(B, D, H, W, Cout, dtype=DT, seed=702)
    ref = torch.nn.grad.conv3d_weight(x.double().permute(0, 4, 1, 2, 3), (Cout, Cin, 3, 3, 3), dy.double().permute(0, 4, 1, 2, 3), padding=1)
    return x, dy, ref


def _launch(x, dy, dw, accumulate, max_workgroups=0):
    """the single-layer launch with a workgroup cap (ops.conv3_wgrad sets the cap from the stream it runs on); returns (dw, workspace):
    where the launch splits the bricks, the workspace holds the fp32 slab of every (channel pair, split) as the brick kernel left it"""
    ops = _ops()
    p = ops._conv3_wgrad_params(x, dy, dw, accumulate)
    p.max_workgroups = max_workgroups
    wsb = ops._plan("miseg_conv3_wgrad_plan", p, ops.L.Conv3WgradPlan()).workspace_bytes
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=x.device)
    p.workspace = ops._ptr(ws)
    ops._call("miseg_conv3_wgrad", p)
    return dw, ws


def _is_piped(x, dy):
    return _ops().conv3_wgrad_plan(x, dy).kernel not in (_ops().L.CONV3_WGRAD_TINY, _ops().L.CONV3_WGRAD_NARROW, _ops().L.CONV3_WGRAD_F32)


@pytest.mark.parametrize("shape", [ONE_BRICK, RAGGED, TWO_CI_BLOCKS], ids=["one_brick", "ragged", "two_ci_blocks"])
def test_weight_gradient_of_the_edge_shapes(shape):
    x, dy, ref = _case(shape)
    assert _is_piped(x, dy)
    assert_parity(_ops().conv3_wgrad(x, dy), ref, TOL[DT], f"weight gradient, x {tuple(x.shape)}")


@pytest.mark.parametrize("cap", [1, 2, 3, 0])
def test_workgroups_that_walk_several_bricks(cap):
    x, dy, ref = _case(SEVERAL_BRICKS)
    dw = torch.empty_like(ref, dtype=torch.float32)
    assert_parity(_launch(x, dy, dw, 0, cap)[0], ref, TOL[DT], f"weight gradient on at most {cap or 'any number of'} workgroup(s)")


@pytest.mark.parametrize("mode", [1, 2])
def test_both_accumulate_modes_on_the_ragged_volume(mode):
    ops = _ops()
    x, dy, ref = _case(RAGGED)
    base = rnd(*ref.shape, seed=703) if mode == 1 else torch.zeros(*ref.shape, device=DEV)
    dw = base.clone()
    ops.conv3_wgrad(x, dy, dw=dw, accumulate=(True if mode == 1 else 2))
    # (mode 1 adds to fp32 values of unit scale: the sum is rounded once more, as in test_conv3_fwd_dgrad_wgrad's accumulated check)
    assert_parity(dw - base, ref, (2 if mode == 1 else 1) * TOL[DT], f"weight gradient, accumulate mode {mode}")


@pytest.mark.parametrize("cap", [0, 3], ids=["normal", "background"])
def test_grouped_launch_of_three_layers(cap):
    """three layers of different size in one call; cap 3: fewer workgroups than (layer, channel pair, split) units, the capped grid walks them"""
    ops = _ops()
    L = ops.L
    cases = [_case(s) for s in GROUP]
    bases = [rnd(*ref.shape, seed=710 + i) for i, (_, _, ref) in enumerate(cases)]
    outs = [b.clone() for b in bases]
    descs = (L.Conv3Wgrad * len(cases))()
    for j, ((x, dy, _), dw) in enumerate(zip(cases, outs)):
        assert _is_piped(x, dy)
        (ldx, _, Cin), (lddy, _, Cout) = ops.rows(x), ops.rows(dy)
        descs[j] = L.Conv3Wgrad(ops._ptr(x), ldx, ops._ptr(dy), lddy, ops._ptr(dw), *ops._vol(x), Cin, Cout, ops._dt(x), 1, None, cap if j == 0 else 0)
    lib = L.load()
    wsb = lib.miseg_conv3_wgrad_group_workspace_bytes(descs, len(cases))
    ws = torch.empty(max(wsb // 4, 1), dtype=torch.float32, device=DEV)
    L.check(lib.miseg_conv3_wgrad_group(descs, len(cases), ops._ptr(ws), ops._stream()), "conv3_wgrad_group")
    torch.cuda.synchronize()
    for (x, _, ref), base, dw in zip(cases, bases, outs):
        assert_parity(dw - base, ref, 2 * TOL[DT], f"grouped weight gradient accumulated onto its slot, x {tuple(x.shape)}, cap {cap}")


def test_the_ragged_case_twice_is_bit_identical():
    """What the brick kernel writes is compared, twice over: the slabs of the split launch (12 bricks, 12 splits) and the gradient of the
    single-producer launch (one workgroup, plain stores).  The GRADIENT of the split launch is not reproducible to the bit and was not
    before this loop changed: conv3_wgrad_reduce_kernel adds its split groups into dw with fp32 atomics, in the order they arrive
    (12 groups here; two runs differ in the last bit of some elements, with the parent's library as with this one)."""
    x, dy, ref = _case(RAGGED)
    runs = [_launch(x, dy, torch.empty_like(ref, dtype=torch.float32), 0, 0) for _ in range(2)]
    assert runs[0][1].numel() == 12 * 27 * 48 * 48, "twelve splits of one channel pair"
    assert torch.equal(runs[0][1], runs[1][1])
    assert_parity(runs[0][0], ref, TOL[DT], "weight gradient of the split launch")
    one = [_launch(x, dy, torch.empty_like(ref, dtype=torch.float32), 0, 1)[0] for _ in range(2)]
    assert torch.equal(one[0], one[1])
    assert_parity(one[0], ref, TOL[DT], "weight gradient on one workgroup")
