"""CPU tests of the weighted window blend (MONAI's sliding_window_inference mode="gaussian", sigma_scale, padding_mode, cval,
roi_weight_map): the importance map against the restatement in tests/gaussian_blend_ref.py, the CPU loop of
training/inferer.py::sliding_window_inference against a window-by-window restatement bit for bit, and the command-line surface.
MONAI is absent from the reference tree: the parity is unpinned, both sides restate its published arithmetic."""
import argparse

import pytest
import torch

import gaussian_blend_ref as G

ROIS = [(96, 96, 96), (32, 24, 16), (16, 24, 16), (7, 5, 3)]


def _inferer():
    from mi_seg_amd.training import inferer
    return inferer


@pytest.mark.parametrize("roi", ROIS)
def test_importance_map_equals_the_convolution_and_the_closed_form(roi):
    I = _inferer()
    m = I.importance_map(roi, "gaussian")
    assert m.dtype == torch.float32 and tuple(m.shape) == roi and m.device.type == "cpu"
    conv, closed = G.conv_map(roi), G.closed_map(roi)
    assert torch.equal(conv, closed)                       # the filter of a one-hot volume is the per-axis product, bit for bit
    assert torch.equal(m, conv)
    centre = tuple(r // 2 for r in roi)
    assert float(m.max()) == 1.0 and float(m[centre]) == 1.0
    assert float(m.min()) == float(torch.tensor(1e-3, dtype=torch.float32))
    for axis, r in enumerate(roi):
        if r % 2 == 1:                                     # an odd axis has its 1 in the middle: the map mirrors there
            assert torch.equal(m, m.flip(axis))
    assert I.importance_map(roi, "gaussian") is m          # cached: built once
    assert torch.equal(I.importance_map(roi, "constant"), torch.ones(roi))


def test_the_default_map_is_not_separable():
    """more than half of the 96^3 map sits on the 1e-3 clamp, which is why the kernel takes the dense map"""
    m = _inferer().importance_map((96, 96, 96), "gaussian")
    share = float((m == m.min()).float().mean())
    assert 0.5 < share < 0.65, share
    assert not torch.equal(m, (m[:, 48, 48, None, None] * m[48, :, 48][None, :, None]) * m[48, 48, :][None, None, :])


def test_per_axis_sigma_scale_and_bad_arguments():
    I = _inferer()
    roi = (32, 24, 16)
    scales = (0.125, 0.25, 0.5)
    m = I.importance_map(roi, "gaussian", sigma_scale=scales)
    assert torch.equal(m, G.conv_map(roi, scales)) and torch.equal(m, G.closed_map(roi, scales))
    assert not torch.equal(m, I.importance_map(roi, "gaussian"))
    assert torch.equal(I.importance_map(roi, "gaussian", sigma_scale=[0.125] * 3), I.importance_map(roi, "gaussian"))
    with pytest.raises(ValueError):
        I.importance_map(roi, "nope")
    with pytest.raises(ValueError):
        I.importance_map(roi, "gaussian", sigma_scale=(0.125, 0.25))
    vol = torch.zeros(1, 1, 40, 30, 20)
    pred = lambda x: x
    for bad in (dict(mode="nope"), dict(padding_mode="nope"), dict(roi_weight_map=torch.ones(32, 24, 15)), dict(roi_weight_map=torch.zeros(roi)),
                dict(roi_weight_map=-torch.ones(roi)), dict(roi_weight_map=torch.full(roi, float("nan"))),
                dict(roi_weight_map=torch.full(roi, float("inf")))):
        with pytest.raises(ValueError):
            I.sliding_window_inference(vol, roi, 2, pred, **bad)


class _Table:
    """predictor that hands out a random table of window logits in the order the windows are asked for"""

    def __init__(self, n, channels, roi, seed):
        self.table = torch.randn(n, channels, *roi, generator=torch.Generator().manual_seed(seed))
        self.at = 0

    def __call__(self, x):
        out = self.table[self.at:self.at + x.shape[0]]
        self.at += x.shape[0]
        return out


CASES = [((70, 41, 33), (32, 24, 16), 0.25, {}),
         ((48, 40, 16), (48, 24, 16), 0.5, {}),                                     # two axes with a single window
         ((20, 30, 12), (32, 24, 16), 0.5, dict(padding_mode="reflect")),            # smaller than the roi on two axes: padded
         ((20, 30, 12), (32, 24, 16), 0.5, dict(padding_mode="constant", cval=-1.0))]


@pytest.mark.parametrize("size,roi,overlap,pad", CASES)
def test_cpu_gaussian_blend_equals_the_window_by_window_restatement(size, roi, overlap, pad):
    I = _inferer()
    from oracle import sliding_window as OSW
    padded = tuple(max(s, r) for s, r in zip(size, roi))
    n = len(OSW.window_origins(padded, roi, overlap))
    vol = torch.randn((1, 1) + size, generator=torch.Generator().manual_seed(3))
    seen = []

    def run(fn, batch, **kw):
        t = _Table(n, 3, roi, 7)

        def predictor(x):
            seen.append(x.clone())
            return t(x)
        out = fn(vol, roi, batch, predictor, overlap=overlap, **kw) if batch else fn(vol, roi, predictor, overlap=overlap, **kw)
        assert t.at == n
        return out

    wmap = G.conv_map(roi)
    want = run(G.weighted_sliding_window_reference, None, wmap=wmap, **pad)
    ref_windows = torch.cat(seen)
    del seen[:]
    got = run(I.sliding_window_inference, 4, mode="gaussian", **pad)
    assert got.shape == (1, 3) + size and torch.equal(got, want)
    assert torch.equal(torch.cat(seen), ref_windows)                       # the same windows of the same padded image, in the same order
    # a caller's map replaces the computed one and is clamped the same way; sw_batch_size does not matter
    mine = torch.rand(roi, generator=torch.Generator().manual_seed(11)) * (torch.rand(roi, generator=torch.Generator().manual_seed(12)) > 0.3)
    want = run(G.weighted_sliding_window_reference, None, wmap=G.clamp_like_the_inferer(mine), **pad)
    assert torch.equal(run(I.sliding_window_inference, 3, mode="gaussian", roi_weight_map=mine, **pad), want)
    # a map of ones is the constant blend, and the constant blend is the restatement the existing tests judge it by
    const = run(I.sliding_window_inference, 4, mode="constant", **pad)
    assert torch.equal(run(I.sliding_window_inference, 4, roi_weight_map=torch.ones(roi), **pad), const)
    assert not torch.equal(const, got)
    if not pad:
        assert torch.equal(const, run(I.sliding_window_inference, 4))
        assert torch.equal(const, run(OSW.sliding_window_reference, None))


def test_padding_modes_reach_the_predictor():
    I = _inferer()
    vol = torch.arange(5 * 6 * 4, dtype=torch.float32).reshape(1, 1, 5, 6, 4)
    for mode, kw in (("constant", dict(cval=-2.0)), ("reflect", {}), ("replicate", {}), ("circular", {})):
        got = []
        I.sliding_window_inference(vol, (8, 6, 6), 1, lambda x: got.append(x.clone()) or x, padding_mode=mode, **kw)
        pp = [1, 1, 0, 0, 1, 2]
        want = torch.nn.functional.pad(vol, pp, value=-2.0) if mode == "constant" else torch.nn.functional.pad(vol, pp, mode=mode)
        assert len(got) == 1 and torch.equal(got[0], want), mode


def _parser():
    from mi_seg_amd.utils.parser import add_data_argparse_args, add_model_argparse_args, add_tune_argparse_args
    p = argparse.ArgumentParser()
    add_tune_argparse_args(add_data_argparse_args(add_model_argparse_args(p)))
    return p


def test_command_line_surface():
    I = _inferer()
    from mi_seg_amd.networks.lightning_monai import LitMonai
    from mi_seg_amd.training import predict
    a = _parser().parse_args([])
    assert (a.infer_mode, a.infer_sigma_scale, a.infer_padding_mode) == ("constant", 0.125, "constant")
    assert (a.infer_overlap, a.sw_batch_size, a.infer_cpu) == (0.5, 1, False)                 # the reference's stay as they are
    b = predict.build_parser().parse_args(["--infer_mode=gaussian", "--infer_sigma_scale", "0.25", "--infer_padding_mode=replicate"])
    assert (b.infer_mode, I.sigma_scale_arg(b.infer_sigma_scale), b.infer_padding_mode) == ("gaussian", 0.25, "replicate")
    assert predict.build_parser().parse_args([]).infer_mode == "constant"
    assert I.sigma_scale_arg([0.1, 0.2, 0.3]) == (0.1, 0.2, 0.3) and I.sigma_scale_arg(0.125) == 0.125
    model = ["--model_name=unet", "--out_channels=3", "--roi_x=32", "--roi_y=24", "--roi_z=16", "--infer_overlap=0.25", "--sw_batch_size=4"]
    lit = LitMonai.from_argparse_args(_parser().parse_args(model + ["--infer_mode=gaussian", "--infer_sigma_scale", "0.125", "0.25", "0.5"]))
    kw = lit.model_inferer.keywords
    assert (kw["mode"], kw["sigma_scale"], kw["padding_mode"]) == ("gaussian", (0.125, 0.25, 0.5), "constant")
    plain = LitMonai.from_argparse_args(_parser().parse_args(model)).model_inferer.keywords
    assert (plain["mode"], plain["sigma_scale"], plain["padding_mode"]) == ("constant", 0.125, "constant")
    # the built inferer blends with the map: swap the network for a table of window logits
    size, roi = (70, 41, 33), (32, 24, 16)
    from oracle import sliding_window as OSW
    n = len(OSW.window_origins(size, roi, 0.25))
    vol = torch.zeros((1, 1) + size)
    got = lit.model_inferer(vol, predictor=_Table(n, 3, roi, 7))
    want = G.weighted_sliding_window_reference(vol, roi, _Table(n, 3, roi, 7), G.conv_map(roi, (0.125, 0.25, 0.5)), overlap=0.25)
    assert torch.equal(got, want)
