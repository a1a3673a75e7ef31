"""GPU tests of the conditional UNet (networks/nets/unet_vanilla.py) and its decoder kernel (csrc/elementwise.hip::miseg_upsample_cat /
miseg_upsample_cat_bwd): the op against the torch composition bit for bit and its adjoint against a float64 box sum, whole-network parity
with the reference module's fixtures (tests/golden/unet_vanilla.npz), the published size, no aten fallback, graph capture, and the prediction
command end to end."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import compare_grads, rel_err, sample
from parity import assert_parity
from test_hip_predict import _host_reference, _mods as _predict_mods

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3
TOL_BF16 = 4e-2


def _norm(name):
    from mi_seg_amd.networks.norms.utils import parse_normalization
    return parse_normalization(name, True, 4, 2)


def _net(channels, strides, num_res_units=2, norm_down="instance", norm_up="instance", out=8):
    from mi_seg_amd.networks.nets.unet_vanilla import UNetVanilla
    return UNetVanilla(3, 1, out, channels=channels, strides=strides, num_res_units=num_res_units, act="prelu", norm_down=_norm(norm_down),
                       norm_up=_norm(norm_up), dropout=0.0, bias=True, adn_ordering="NDA")


def _filled(m, dtype=torch.float32):
    from mi_seg_amd.utils.detfill import fill_module_
    fill_module_(m)
    return m.to(DEV).set_compute_dtype(dtype)


def _row_view(B, grid, C, dtype, pad, seed):
    """[B, *grid, C] channels-last view at channel offset `pad` of a buffer with C + 2 pad channels (ld > C)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    big = torch.randn((B,) + tuple(grid) + (C + 2 * pad,), generator=g, device=DEV).to(dtype)
    return big[..., pad:pad + C]


def _composition(skip, x, f):
    """the reference's nn.Upsample(scale_factor=f) (nearest) + torch.concat((skip, up), dim=1), on NCDHW, back to channels-last"""
    up = F.interpolate(x.permute(0, 4, 1, 2, 3).float(), scale_factor=f, mode="nearest").to(x.dtype)
    return torch.cat((skip.permute(0, 4, 1, 2, 3), up), dim=1).permute(0, 2, 3, 4, 1)


SHAPES = [(3, 5, 0), (3, 5, 3), (16, 32, 0), (16, 32, 8), (8, 24, 16)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("f", [1, 2])
@pytest.mark.parametrize("cs,cu,pad", SHAPES)
def test_upsample_cat_forward_is_the_torch_composition(dtype, f, cs, cu, pad):
    from mi_seg_amd.hip import ops
    fine = (6, 4, 10)
    skip = _row_view(2, fine, cs, dtype, pad, 1)
    x = _row_view(2, tuple(v // f for v in fine), cu, dtype, pad, 2)
    got = ops.upsample_cat(skip, x, f)
    want = _composition(skip, x, f)
    assert got.shape == want.shape and got.dtype == dtype
    assert torch.equal(got, want)


@pytest.mark.parametrize("f", [1, 2])
@pytest.mark.parametrize("cs,cu,pad", SHAPES)
def test_upsample_cat_backward_is_the_box_sum(f, cs, cu, pad):
    from mi_seg_amd.hip import ops
    fine = (8, 6, 12)
    g = torch.Generator(device=DEV).manual_seed(3)
    dcat32 = torch.randn((2,) + fine + (cs + cu + pad,), generator=g, device=DEV)
    want64 = dcat32[..., cs:cs + cu].double()
    box = want64.reshape(2, fine[0] // f, f, fine[1] // f, f, fine[2] // f, f, cu).sum(dim=(2, 4, 6))
    got = ops.upsample_cat_bwd(dcat32[..., cs:cs + cu], f)
    assert got.shape == box.shape and got.dtype == torch.float32
    assert float((got.double() - box).abs().max()) <= 1e-6 * float(box.abs().max())
    # bf16: the fp32 sum of the bf16 children in (dz, dy, dx) order, rounded once
    dcat16 = dcat32.bfloat16()
    right = dcat16[..., cs:cs + cu]
    acc = torch.zeros(box.shape, dtype=torch.float32, device=DEV)
    for dz in range(f):
        for dy in range(f):
            for dx in range(f):
                acc = acc + right[:, dz::f, dy::f, dx::f].float()
    got16 = ops.upsample_cat_bwd(right, f)
    assert got16.dtype == torch.bfloat16 and torch.equal(got16, acc.bfloat16())
    assert torch.equal(ops.upsample_cat_bwd(right, f), got16)              # no atomics: bit-reproducible


@pytest.mark.parametrize("f", [1, 2])
def test_upsample_cat_autograd(f):
    from mi_seg_amd.hip import functional as HF
    skip = _row_view(2, (4, 4, 4), 16, torch.float32, 0, 5).contiguous().requires_grad_(True)
    x = _row_view(2, (4 // f,) * 3, 8, torch.float32, 0, 6).contiguous().requires_grad_(True)
    y = HF.upsample_cat(skip, x, f)
    cot = torch.randn(y.shape, device=DEV)
    y.backward(cot)
    s2, x2 = skip.detach().clone().requires_grad_(True), x.detach().clone().requires_grad_(True)
    _composition(s2, x2, f).backward(cot)
    assert torch.equal(skip.grad, s2.grad)
    assert float((x.grad - x2.grad).abs().max()) <= 1e-5 * float(x2.grad.abs().max())


def _parity(G, tag, dtype):
    from mi_seg_amd.utils.detfill import det_input
    c = G.meta["cases"][tag]
    m = _filled(_net(c["channels"], c["strides"], c["num_res_units"], c["norm_down"], c["norm_up"]), dtype)
    assert list(m.state_dict().keys()) == c["state_keys"]
    x = det_input(1234, c["x"]).to(DEV)
    y = m(x, c["modalities"])
    return m, y


@pytest.mark.parametrize("tag,dtype", [("cond_32", torch.float32), ("pre_s2", torch.float32), ("cond_32", torch.bfloat16),
                                       ("pre_s2", torch.bfloat16)])
def test_unet_vanilla_matches_the_reference(golden, tag, dtype):
    from mi_seg_amd.utils.detfill import det_input
    G = golden("unet_vanilla")
    c = G.meta["cases"][tag]
    m, y = _parity(G, tag, dtype)
    side = c["x"][2] // c["strides"][0]
    assert y.dtype == torch.float32 and list(y.shape) == [c["x"][0], 8, side, side, side]
    tol = TOL if dtype == torch.float32 else TOL_BF16
    whole = G.t(f"{tag}/logits") if G.has(f"{tag}/logits") else G.t(f"{tag}/logits_sub")
    got = y if G.has(f"{tag}/logits") else y[:, :, ::2, ::2, ::4]
    if dtype == torch.float32:
        assert_parity(sample(y), G.t(f"{tag}/logits_samples"), tol, "sampled logits")
        assert_parity(got, whole, tol, "logits")
    else:
        # a whole bf16 network against recorded vectors is a module-level golden comparison and stays on its pooled bar: no torch composition
        # of the same arithmetic is at hand to measure a per-element yardstick with (measured local error 6.5e-2 at pooled 1.1e-2)
        assert rel_err(sample(y), G.t(f"{tag}/logits_samples")) < tol
        assert rel_err(got, whole) < tol
    y.backward(det_input(4321, tuple(y.shape)).to(DEV))
    named = dict(m.named_parameters())
    if dtype == torch.float32:
        compare_grads({k: p.grad for k, p in named.items()}, G.grads(tag), 10 * TOL, sampled=True, vanish_tol=1e-2)
    assert sorted(k for k, p in named.items() if p.grad is None) == sorted(c["grad_none"])
    assert all(torch.isfinite(p.grad).all() for p in named.values() if p.grad is not None)


def test_absent_modality_rows_get_no_gradient(golden):
    """one modality in the batch: the other's conditional-norm rows stay without a gradient, as in the reference's per-sample norm"""
    from mi_seg_amd.utils.detfill import det_input
    m = _filled(_net([8, 16, 32], [1, 2, 2], 2, "instance_cond", "instance"))
    y = m(det_input(7, (1, 1, 32, 32, 32)).to(DEV), [1])
    y.backward(det_input(8, tuple(y.shape)).to(DEV))
    none = sorted(k for k, p in m.named_parameters() if p.grad is None)
    assert none and all(".N.norms.0." in k for k in none), none


def test_published_size_bf16():
    """the README's C-UNet (62.6 M parameters) at one 96^3 patch in bf16, forward and backward"""
    from mi_seg_amd.utils.detfill import det_input
    m = _filled(_net([16, 64, 128, 256, 512], [1, 2, 2, 2, 1], 3, "instance_cond", "instance"), torch.bfloat16)
    y = m(det_input(11, (1, 1, 96, 96, 96)).to(DEV), [0])
    assert list(y.shape) == [1, 8, 96, 96, 96] and bool(torch.isfinite(y).all())
    y.backward(det_input(12, tuple(y.shape)).to(DEV))
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert len(grads) > 100 and all(bool(torch.isfinite(g).all()) for g in grads)


def test_no_torch_fallback_in_a_training_step():
    from torch.profiler import ProfilerActivity, profile
    from mi_seg_amd.utils.detfill import det_input
    m = _filled(_net([8, 16, 32, 64], [1, 2, 2, 1], 2, "instance_cond", "instance"), torch.bfloat16)
    x, cot = det_input(1, (2, 1, 32, 32, 32)).to(DEV), det_input(2, (2, 8, 32, 32, 32)).to(DEV)
    m(x, [0, 1]).backward(cot)                      # warm-up
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        m(x, [0, 1]).backward(cot)
        torch.cuda.synchronize()
    names = {e.name for e in prof.events()}
    bad = sorted(n for n in names if n.startswith("aten::upsample_nearest3d") or n in ("aten::cat", "aten::repeat_interleave"))
    assert not bad, bad


def test_graphed_train_step_matches_the_eager_loop():
    """runtime/graph.py::GraphedTrainStep on a small bf16 C-UNet against the same steps launched eagerly: the bars of
    test_hip_training.py::test_graphed_train_step_matches_the_eager_loop"""
    from mi_seg_amd.runtime.arena import ParamArena
    from mi_seg_amd.runtime.graph import GraphedTrainStep
    from mi_seg_amd.training.losses import DiceFocalLoss
    from mi_seg_amd.training.optim import ArenaOptimizer
    from mi_seg_amd.utils.detfill import det_input

    def small():
        return _filled(_net([8, 16, 32, 64], [1, 2, 2, 2], 2, "instance_cond", "instance", out=6), torch.bfloat16)

    crit = DiceFocalLoss(include_background=False, to_onehot_y=True, softmax=True, squared_pred=True, smooth_nr=0.0, smooth_dr=1e-6)
    xs = [det_input(30 + i, (1, 1, 64, 64, 64)).to(DEV) for i in range(6)]
    ys = [(x.abs() * 3).floor().clamp(0, 5).to(torch.int32) for x in xs]
    mods = [0, 1, 1, 0, 0, 1]
    lrs = [2e-3, 2e-3, 2e-3, 5e-4, 5e-4, 5e-4]
    runs = {}
    for mode in ("eager", "graph"):
        m = small()
        arena = ParamArena([p for p in m.parameters() if p.requires_grad], torch.bfloat16)
        try:
            opt = ArenaOptimizer(arena, "adamw", lr=lrs[0], weight_decay=1e-5)
            losses = []
            if mode == "graph":
                gts = GraphedTrainStep(m, crit, opt, xs[0].shape, ys[0].shape, arena)
            for x, y, md, lr in zip(xs, ys, mods, lrs):
                if mode == "graph":
                    gts.set_lr(lr)
                    losses.append(float(gts(x, y, [md])))
                else:
                    arena.begin_step()
                    loss = crit(m(x, [md]), y)
                    loss.backward()
                    arena.publish()
                    opt.step(lr=lr)
                    losses.append(float(loss))
            torch.cuda.synchronize()
            runs[mode] = (losses, {k: v.detach().clone() for k, v in m.state_dict().items()})
        finally:
            arena.detach()
    le, lg = runs["eager"][0], runs["graph"][0]
    print("C-UNet train step losses: eager", [round(v, 5) for v in le], "graph", [round(v, 5) for v in lg])
    assert all(v == v for v in lg) and lg[-1] < lg[0]
    for i, (a, b) in enumerate(zip(le, lg)):
        assert abs(a - b) < 2e-3 * (1 + i) * abs(a), (i, a, b)
    num = den = 0.0
    for k, v in runs["eager"][1].items():
        w = runs["graph"][1][k]
        if v.is_floating_point():
            assert float((v - w).abs().max()) <= 2.02 * sum(lrs), k
            num += float((v.double() - w.double()).pow(2).sum())
            den += float(v.double().pow(2).sum())
    assert (num / den) ** 0.5 < 2e-2, (num / den) ** 0.5
    sd0 = small().state_dict()
    moved = sum(1 for k, v in runs["graph"][1].items() if v.is_floating_point() and not torch.equal(v, sd0[k]))
    assert moved > 50


VANILLA_ARGS = ["--model=unet_vanilla", "--feature_size", "8", "16", "32", "64", "--strides", "1", "2", "2", "1", "--num_res_units=2",
                "--out_channels", "8", "--roi_x", "32", "--roi_y", "32", "--roi_z", "32", "--encoder_norm_name", "instance_cond",
                "--decoder_norm_name", "instance", "--sw_batch_size", "2"]


def test_predict_end_to_end(tmp_path):
    """predict_whs with the C-UNet: label maps of a synthetic CT volume from a checkpoint written by export_state, equal to the host-side
    composition (sliding window, argmax, numpy inverse, remap), and the modality reaches the conditional norms"""
    N, P, _, _, R = _predict_mods()
    from mi_seg_amd.data.checkpoint import export_state
    from mi_seg_amd.networks.nets.unet_vanilla import UNetVanilla
    from mi_seg_amd.networks.utils.utils import model_from_argparse_args
    from mi_seg_amd.utils.detfill import fill_module_
    data = tmp_path / "data"
    (data / "imagesTs").mkdir(parents=True)
    rng = np.random.default_rng(12)
    ct = rng.normal(0, 300, (41, 37, 23)).astype(np.int16)
    A = np.array([[-0.7 * 0.98, 0.8 * 0.17, 0.0, 120.0], [-0.7 * 0.17, -0.8 * 0.98, 0.0, 95.5], [0.0, 0.0, 1.6, -210.0], [0, 0, 0, 1.0]])
    img = "imagesTs/ct_test_2001_image.nii.gz"
    N.write_nifti(str(data / img), ct, A)
    for name, mod in (("CT_test.json", "CT"), ("MR_test.json", "MR")):
        (data / name).write_text(json.dumps({"modality": {"0": mod}, "test": [{"image": img}]}))
    args = R.build_parser().parse_args(VANILLA_ARGS)
    model = model_from_argparse_args(args)
    assert isinstance(model, UNetVanilla)
    fill_module_(model)
    ck = str(tmp_path / "ck.pt")
    export_state(model, ck)
    model = model.to(DEV).eval()
    a2 = args.__class__(**vars(args))
    a2.device = DEV
    labels = {}
    for json_list, mod in (("CT_test.json", 0), ("MR_test.json", 1)):
        out = tmp_path / f"out{mod}"
        paths = R.main(VANILLA_ARGS + ["--checkpoint", ck, "--data_dir", str(data), "--json_list", json_list, "--result_dir", str(out)])
        assert paths == [str(out / "ct_test_2001_label.nii.gz")]
        arr, aff = N.read_nifti(paths[0])
        assert arr.dtype == np.uint16 and arr.shape == ct.shape and np.allclose(aff, A, atol=1e-5)
        assert np.array_equal(arr, _host_reference(model, {"image": str(data / img)}, a2, mod))
        assert set(np.unique(arr).tolist()) <= {0, 500, 600, 420, 550, 205, 820, 850}
        labels[mod] = arr
    assert not np.array_equal(labels[0], labels[1])           # the same image as CT and as MR: the modality reached the model
