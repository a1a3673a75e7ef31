"""GPU tests of the weighted gather stitch (csrc/training.hip::stitch_weighted_kernel): MONAI's mode="gaussian"
blend as ONE gather over the resident window logits.  The kernel adds fl(map * pred) of the covering windows in window-index order and
divides by the weights summed in the same order, so it is held to the bits of the sequential torch loop
(tests/gaussian_blend_ref.py::weighted_loop); the end-to-end run is held to the CPU restatement that runs the oracle network window by window."""
import pytest
import torch

import gaussian_blend_ref as G
from parity import assert_parity

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _starts(size, roi, overlap):
    from mi_seg_amd.training.inferer import _starts as s
    return tuple(s(a, r, overlap) for a, r in zip(size, roi))


@pytest.mark.parametrize("size,roi,overlap,cover", [((70, 41, 33), (32, 24, 16), 0.25, 8),
                                                    ((48, 40, 16), (48, 24, 16), 0.5, 3),          # two axes with a single window
                                                    ((96, 24, 16), (16, 24, 16), 0.75, 4),         # overlap 0.75 along one axis: 4 windows a voxel
                                                    ((41, 40, 16), (16, 16, 16), 0.75, 20),        # more than 8 windows a voxel: the map is re-read
                                                    ((160, 160, 128), (96, 96, 96), 0.5, 18)])     # the real roi: the clamp plateau; pulled-back last
                                                                                                   # windows make 3 x 3 x 2 covers: both paths
def test_weighted_stitch_is_bit_identical_to_the_sequential_loop(size, roi, overlap, cover):
    from mi_seg_amd.hip import ops
    from mi_seg_amd.training.inferer import importance_map
    starts = _starts(size, roi, overlap)
    n = len(starts[0]) * len(starts[1]) * len(starts[2])
    win = torch.randn(n, 3, *roi, generator=torch.Generator().manual_seed(2)).to(DEV)
    wmap = importance_map(roi, "gaussian", device=DEV)
    assert wmap.is_cuda and torch.equal(wmap.cpu(), G.conv_map(roi))
    out = torch.empty((3,) + size, dtype=torch.float32, device=DEV)
    wsum = torch.empty(size, dtype=torch.float32, device=DEV)
    count = torch.empty(size, dtype=torch.int16, device=DEV)
    ops.stitch_windows(win, out, starts, roi, count=count, weight=wmap, wsum=wsum)
    want, ws = G.weighted_loop(win, wmap, starts, roi, size)
    assert int(count.max()) == cover               # <= 8: weights and offsets of a voxel in registers; beyond: the loop that re-reads the map
    assert torch.equal(wsum, ws)
    assert torch.equal(out, want)                      # products rounded before they are added, same order, a true division
    # a map of ones gives the bits of the constant kernel
    plain = torch.empty_like(out)
    ops.stitch_windows(win, plain, starts, roi)
    ones = torch.empty_like(out)
    ops.stitch_windows(win, ones, starts, roi, weight=torch.ones(roi, device=DEV), wsum=wsum)
    assert torch.equal(ones, plain) and torch.equal(wsum, count.float())
    assert not torch.equal(plain, out)


def test_weight_map_validation():
    from mi_seg_amd.hip import ops
    size, roi = (48, 40, 16), (48, 24, 16)
    starts = _starts(size, roi, 0.5)
    win = torch.zeros(len(starts[1]), 2, *roi, device=DEV)
    out = torch.empty((2,) + size, device=DEV)
    good = torch.ones(roi, device=DEV)
    for weight, wsum in ((torch.ones(48, 24, 15, device=DEV), None), (torch.ones(roi, device=DEV, dtype=torch.float64), None),
                         (torch.ones(roi), None), (torch.ones(48, 24, 32, device=DEV)[:, :, ::2], None),
                         (good, torch.empty((2,) + size, device=DEV)), (good, torch.empty(size, device=DEV, dtype=torch.float64)),
                         (None, torch.empty(size, device=DEV))):
        with pytest.raises(ValueError):
            ops.stitch_windows(win, out, starts, roi, weight=weight, wsum=wsum)
    ops.stitch_windows(win, out, starts, roi, weight=good)
    assert torch.equal(out, torch.zeros_like(out))


def test_slab_wise_gaussian_stitching_equals_the_resident_gather(monkeypatch):
    """the sizes and budgets of test_hip_training.py::test_slab_wise_stitching_equals_the_resident_gather with mode="gaussian": the map
    rides through the slab stitcher, every slab is the same gather"""
    from mi_seg_amd.training import inferer
    size, roi, overlap, layers = (200, 40, 33), (32, 24, 16), 0.5, 3
    starts = _starts(size, roi, overlap)
    n = len(starts[0]) * len(starts[1]) * len(starts[2])
    table = torch.randn(n, 3, *roi, generator=torch.Generator().manual_seed(5)).to(DEV)
    vol = torch.zeros((1, 1) + size, device=DEV)
    state = {"i": 0}

    def predictor(x):
        k = x.shape[0]
        out = table[state["i"]:state["i"] + k]
        state["i"] += k
        return out

    wmap = inferer.importance_map(roi, "gaussian", device=DEV)
    want, _ = G.weighted_loop(table, wmap, starts, roi, size)
    per_layer = len(starts[1]) * len(starts[2]) * 3 * roi[0] * roi[1] * roi[2] * 4
    for budget, batch in ((None, 4), (layers * per_layer, 4), (layers * per_layer, 1), (1, 3)):
        monkeypatch.setattr(inferer, "RESIDENT_LIMIT_BYTES", budget)
        state["i"] = 0
        got = inferer.sliding_window_inference(vol, roi, batch, predictor, overlap=overlap, mode="gaussian")
        assert torch.equal(got[0], want), (budget, batch)
    monkeypatch.setattr(inferer, "RESIDENT_LIMIT_BYTES", layers * per_layer)
    state["i"] = 0
    mine = torch.rand(roi, generator=torch.Generator().manual_seed(9))
    got = inferer.sliding_window_inference(vol, roi, 4, predictor, overlap=overlap, roi_weight_map=mine)
    want, _ = G.weighted_loop(table, G.clamp_like_the_inferer(mine), starts, roi, size)
    assert torch.equal(got[0], want)


def test_gaussian_sliding_window_on_the_hip_path_matches_the_oracle():
    """the small fs=12 Swin-UNETR, 8 windows of 64^3 over a 96 x 80 x 72 volume in batches of 4, mode="gaussian": against the CPU restatement
    that runs the oracle network window by window, at the 1e-3 of the constant-mode test of the same model and volume (a convex blend of the
    same window logits is no further off in kind); the hipGraph'd forward gives the bits of the eager one."""
    from mi_seg_amd.networks.nets.swin_unetr import SwinUNETR
    from mi_seg_amd.networks.norms.utils import parse_normalization
    from mi_seg_amd.runtime.graph import GraphedForward
    from mi_seg_amd.training.inferer import sliding_window_inference
    from mi_seg_amd.utils.detfill import det_input, fill_module_
    from oracle import nets as ON
    norm = lambda name: parse_normalization(name, True, 4, 2)
    m = SwinUNETR((64,) * 3, 1, 6, feature_size=12, num_heads=(3, 6, 12, 24), vit_norm_name=norm("instance_cond"),
                  encoder_norm_name=norm("instance_cond"), decoder_norm_name=norm("instance"))
    fill_module_(m)
    m = m.to(DEV).set_compute_dtype(torch.float32)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    cfg = ON.swin_unetr_cfg(feature_size=12)
    vol = det_input(5, (1, 1, 96, 80, 72))
    want = G.weighted_sliding_window_reference(vol, 64, lambda x: ON.swin_unetr_forward(sd, x, [1], cfg), G.conv_map((64,) * 3), overlap=0.5)
    eager = sliding_window_inference(vol.to(DEV), 64, 4, m, overlap=0.5, modalities=torch.tensor([1]), mode="gaussian")
    graphed = sliding_window_inference(vol.to(DEV), 64, 4, GraphedForward(m, (4, 1, 64, 64, 64)), overlap=0.5, modalities=[1], mode="gaussian")
    assert eager.shape == want.shape and eager.is_cuda
    pooled, local = assert_parity(eager, want, 1e-3, "gaussian-blended logits against the oracle")
    print(f"gaussian blend against the oracle: pooled {pooled:.3e}, local {local:.3e}")
    assert torch.equal(eager, graphed)
    constant = sliding_window_inference(vol.to(DEV), 64, 4, m, overlap=0.5, modalities=[1])
    assert not torch.equal(constant, eager)


def test_predict_command_with_gaussian_blend_writes_a_label_map(tmp_path, monkeypatch):
    """predict_whs.py's main with --infer_mode=gaussian: the three options reach the inferer, and the written uint16 label map is the export
    of the Gaussian-blended logits"""
    import json

    import numpy as np
    from mi_seg_amd.data import nifti as N
    from mi_seg_amd.data import preprocess as P
    from mi_seg_amd.data.checkpoint import export_state
    from mi_seg_amd.networks.utils.utils import model_from_argparse_args
    from mi_seg_amd.training import inferer, predict as R
    from mi_seg_amd.utils.detfill import fill_module_
    model_args = ["--model_name", "swin_unetr", "--feature_size", "12", "--num_heads", "3", "--out_channels", "8", "--roi_x", "32", "--roi_y", "32",
                  "--roi_z", "32", "--vit_norm_name", "instance_cond", "--encoder_norm_name", "instance_cond", "--decoder_norm_name", "instance",
                  "--sw_batch_size", "2", "--infer_mode", "gaussian", "--infer_sigma_scale", "0.25", "--infer_padding_mode", "replicate"]
    data = tmp_path / "data"
    (data / "imagesTs").mkdir(parents=True)
    ct = np.random.default_rng(11).normal(0, 300, (41, 37, 23)).astype(np.int16)
    A = np.array([[-0.7 * 0.98, 0.8 * 0.17, 0.0, 120.0], [-0.7 * 0.17, -0.8 * 0.98, 0.0, 95.5], [0.0, 0.0, 1.6, -210.0], [0, 0, 0, 1.0]])
    image = str(data / "imagesTs" / "ct_test_2001_image.nii.gz")
    N.write_nifti(image, ct, A)
    (data / "CT_test.json").write_text(json.dumps({"modality": {"0": "CT"}, "test": [{"image": "imagesTs/ct_test_2001_image.nii.gz"}]}))
    args = R.build_parser().parse_args(model_args)
    args.feature_size = args.feature_size[0]
    model = model_from_argparse_args(args)
    fill_module_(model)
    ck = str(tmp_path / "ck.pt")
    export_state(model, ck)
    seen = []

    def spy(*a, **kw):
        seen.append({k: kw[k] for k in ("mode", "sigma_scale", "padding_mode")})
        return inferer.sliding_window_inference(*a, **kw)

    monkeypatch.setattr(R, "sliding_window_inference", spy)
    paths = R.main(model_args + ["--checkpoint", ck, "--data_dir", str(data), "--json_list", "CT_test.json", "--result_dir", str(tmp_path / "out")])
    assert seen == [dict(mode="gaussian", sigma_scale=0.25, padding_mode="replicate")]
    arr, aff = N.read_nifti(paths[0])
    assert paths[0].endswith("ct_test_2001_label.nii.gz") and arr.dtype == np.uint16 and arr.shape == ct.shape and np.allclose(aff, A, atol=1e-5)
    model = model.to(DEV).eval()
    vol, geom = P.load_image_for_prediction(image, (1.0, 1.0, 1.0), (32, 32, 32), DEV)
    with torch.no_grad():
        logits = inferer.sliding_window_inference(vol, (32, 32, 32), 2, model, overlap=0.5, modalities=torch.tensor([0], device=DEV), mode="gaussian",
                                                  sigma_scale=0.25, padding_mode="replicate")
    assert np.array_equal(arr, R.to_host(R.invert_prediction(logits, geom, R.label_lut(8))))
