"""The per-element parity helper (tests/parity.py) on the CPU, at two of the kernel suite's own shapes: inputs rounded to bf16, the honest
result accumulated in fp32 and rounded once to bf16, the reference in float64.  The pooled relative L2 error lets a zeroed corner voxel
(about 1.35e-2) and a lost GEMM tail row (about 1.40e-2) through the bf16 bar of 2e-2; the local metric sees an honest result at about
3e-3 and each defect at 0.5 or more."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from parity import assert_parity, local_err

BF16_TOL, FP32_TOL = 2e-2, 2e-4


def _bf16(t):
    return t.to(torch.bfloat16).float()


@pytest.fixture(scope="module")
def conv_case():
    """1 x 9 x 13 x 19 voxels, 48 -> 48 channels, 3x3x3, zero padding (NCDHW here: voxel (d, h, w) is [0, :, d, h, w])"""
    g = torch.Generator().manual_seed(1)
    x = _bf16(torch.randn(1, 48, 9, 13, 19, generator=g))
    w = _bf16(torch.randn(48, 48, 3, 3, 3, generator=g) / (27 * 48) ** 0.5)
    ref = F.conv3d(x.double(), w.double(), padding=1)
    y32 = F.conv3d(x, w, padding=1)
    w_cut = w.clone()
    w_cut[..., 2] = 0                       # the nine taps of kw = 2
    y_cut = F.conv3d(x, w_cut, padding=1)
    return {"ref": ref, "fp32": y32, "bf16": _bf16(y32), "cut": _bf16(y_cut)}


@pytest.fixture(scope="module")
def gemm_case():
    """5003 x 144 x 48: the streaming GEMM's ragged-tail shape"""
    g = torch.Generator().manual_seed(2)
    a = _bf16(torch.randn(5003, 48, generator=g))
    w = _bf16(torch.randn(144, 48, generator=g) / 48 ** 0.5)
    ref = a.double() @ w.double().t()
    y32 = a @ w.t()
    return {"ref": ref, "fp32": y32, "bf16": _bf16(y32)}


def _caught(got, ref, tol):
    """assert_parity must fail; returns the index it names"""
    with pytest.raises(AssertionError) as ei:
        assert_parity(got, ref, tol, "mutated")
    msg = str(ei.value)
    assert "mutated" in msg and "pooled" in msg and "local_err" in msg and "worst element" in msg, msg
    _, idx = local_err(got, ref)
    assert str(idx) in msg, (idx, msg)
    return idx


def test_honest_bf16_passes(conv_case, gemm_case):
    for case, name in ((conv_case, "conv"), (gemm_case, "gemm")):
        pooled, loc = assert_parity(case["bf16"], case["ref"], BF16_TOL, name)
        print(f"{name}: honest bf16 pooled {pooled:.3e} local {loc:.3e}")
        assert pooled < 2.0 ** -8 and loc < 1.01 * 2.0 ** -8        # one round to nearest of a bf16 (8 significant bits): at most 2^-8 per element


def test_honest_fp32_passes(conv_case, gemm_case):
    for case, name in ((conv_case, "conv"), (gemm_case, "gemm")):
        pooled, loc = assert_parity(case["fp32"], case["ref"], FP32_TOL, name)
        print(f"{name}: honest fp32 pooled {pooled:.3e} local {loc:.3e}")
        assert loc < 2e-5


def test_corner_voxel_zeroed_passes_pooled_and_is_caught(conv_case):
    got = conv_case["bf16"].clone()
    got[0, :, 8, 12, 18] = 0
    assert rel_err(got, conv_case["ref"]) < BF16_TOL          # why the helper exists: the pooled number lets this through
    idx = _caught(got, conv_case["ref"], BF16_TOL)
    assert (idx[0], idx[2], idx[3], idx[4]) == (0, 8, 12, 18)
    assert local_err(got, conv_case["ref"])[0] > 0.3


def test_last_w_line_zeroed_is_caught(conv_case):
    got = conv_case["bf16"].clone()
    got[0, :, 8, 12, :] = 0
    idx = _caught(got, conv_case["ref"], BF16_TOL)
    assert (idx[0], idx[2], idx[3]) == (0, 8, 12)


def test_w_plane_losing_nine_taps_is_caught(conv_case):
    got = conv_case["bf16"].clone()
    got[..., 7] = conv_case["cut"][..., 7]
    idx = _caught(got, conv_case["ref"], BF16_TOL)
    assert idx[4] == 7


def test_tail_row_zeroed_passes_pooled_and_is_caught(gemm_case):
    got = gemm_case["bf16"].clone()
    got[5002] = 0
    assert rel_err(got, gemm_case["ref"]) < BF16_TOL          # pooled: about 1.40e-2 against the 2e-2 bar
    idx = _caught(got, gemm_case["ref"], BF16_TOL)
    assert idx[0] == 5002
    assert local_err(got, gemm_case["ref"])[0] > 0.3


def test_nan_in_got_fails(gemm_case):
    got = gemm_case["bf16"].clone()
    got[17, 3] = float("nan")
    with pytest.raises(AssertionError) as ei:
        assert_parity(got, gemm_case["ref"], BF16_TOL, "nan")
    assert "non-finite" in str(ei.value) and "(17, 3)" in str(ei.value)
    got[17, 3] = float("inf")
    with pytest.raises(AssertionError):
        assert_parity(got, gemm_case["ref"], BF16_TOL, "inf")


def test_all_zero_reference_does_not_divide_by_zero():
    ref = torch.zeros(7, 5)
    val, idx = local_err(torch.zeros(7, 5), ref)
    assert val == 0.0 and idx == (0, 0)
    assert_parity(torch.zeros(7, 5, dtype=torch.bfloat16), ref, FP32_TOL, "zeros")
    got = torch.zeros(7, 5)
    got[3, 2] = 1e-6
    with pytest.raises(AssertionError):
        assert_parity(got, ref, BF16_TOL, "zeros")
    assert local_err(got, ref)[1] == (3, 2)


def test_shapes_must_match_and_index_is_unravelled():
    ref = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4) + 1
    got = ref.clone()
    got[1, 2, 1] += 5
    val, idx = local_err(got, ref)
    assert idx == (1, 2, 1)
    assert val == pytest.approx(5 / (float(ref[1, 2, 1]) + float(ref.square().mean().sqrt())))
    with pytest.raises(AssertionError):
        assert_parity(got.reshape(6, 4), ref, 1.0, "shape")
