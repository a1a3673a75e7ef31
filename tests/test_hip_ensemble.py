"""GPU tests of flip test-time augmentation and model ensembling (csrc/ensemble.hip::miseg_ensemble_accumulate, training/ensemble.py;
DESIGN.md section 7.10).  The kernel folds fl(w * t) into the accumulator with every operation rounded on its own, so kinds mean_logits and
vote are held to the bits of the torch restatement (hip/ops.py::ensemble_accumulate_torch, itself held to a hand-written float64 computation
in test_ensemble_cpu.py); mean_prob, whose exp is another implementation, to 4x the restatement's own fp32 error against float64.  End to
end the EnsembleInferer is held to the bits of the explicit torch loop over the project's own sliding_window_inference.

Measured (MI355X): mean_prob at [2, 5, 6, 7, 9] x 8 members, randn * 3, seeds 0 / 1 / 2: the restatement's largest error against float64
7.116e-8 / 7.130e-8 / 7.782e-8, the kernel's the same three figures; 0 / 0 / 0.13 % of the voxels lie under the 1e-5 gap."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import ensemble_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NOFLIP = (False, False, False)


def _ops():
    from mi_seg_amd.hip import ops
    return ops


def _aligned(shape, seed, offset=0):
    """a contiguous fp32 device tensor of `shape` whose first element sits `offset` floats behind a 16-byte boundary, and its CPU copy"""
    n = int(np.prod(shape))
    buf = torch.empty(n + 8, device=DEV)
    lead = (offset - buf.data_ptr() // 4) % 4
    t = buf[lead:lead + n].view(shape)
    assert (t.data_ptr() // 4) % 4 == offset and t.is_contiguous()
    host = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    t.copy_(host)
    return t, host


SHAPES = [((2, 3, 5, 6, 7), 0, 0),          # odd everything: the scalar path, B > 1
          ((1, 6, 8, 12, 16), 0, 0),        # the vector path
          ((1, 2, 3, 4, 260), 0, 0),        # 65 quads a row: rows straddle wavefronts and workgroups, W % 4 == 0
          ((1, 1, 4, 4, 6), 0, 0),          # C = 1, a tail quad of two
          ((1, 17, 3, 3, 8), 0, 0),         # beyond the register-resident channel count
          ((1, 64, 2, 2, 4), 0, 0),         # the channel limit
          ((1, 4, 2, 3, 8), 1, 0),          # src rows 4-byte but not 16-byte aligned
          ((1, 4, 2, 3, 8), 0, 1),          # acc rows so
          ((1, 4, 2, 3, 8), 1, 3)]          # both


def _weights(Cc, per_class):
    if not per_class:
        return 0.3, 1.7
    g = torch.Generator().manual_seed(Cc)
    return tuple((torch.rand(Cc, generator=g) + 0.1).tolist()), tuple((torch.rand(Cc, generator=g) + 0.1).tolist())


@pytest.mark.parametrize("shape,src_off,acc_off", SHAPES)
@pytest.mark.parametrize("kind", ["mean_logits", "vote"])
def test_kernel_is_bit_identical_to_the_restatement(kind, shape, src_off, acc_off):
    """all 8 flips x first / add / add + scaled x scalar and per-class weights on every shape at which the kernel takes another path"""
    ops = _ops()
    Cc = shape[1]
    a_dev, a = _aligned(shape, 1, src_off)
    b_dev, b = _aligned(shape, 2, src_off)
    acc_dev, _ = _aligned(shape, 3, acc_off)
    if kind == "vote":                       # exact ties in later channels: the first maximum must win
        from test_hip_predict import tied_logits
        cls = torch.randint(0, Cc, (shape[0],) + shape[2:], generator=torch.Generator().manual_seed(4))
        a = torch.stack([tied_logits(c, Cc, 5 + i) for i, c in enumerate(cls)])
        a_dev.copy_(a)
    for flip in R.FLIPS:
        for per_class in (False, True):
            w0, w1 = _weights(Cc, per_class)
            scale = tuple((1.0 / (np.asarray(w0) + np.asarray(w1)) * np.ones(Cc)).tolist()) if per_class else 1.0 / (w0 + w1)
            acc_dev.fill_(float("nan"))                                   # first never reads the accumulator
            acc = torch.full(shape, float("nan"))
            for src_dev, src, kw in ((a_dev, a, dict(weight=w0, first=True)), (b_dev, b, dict(weight=w1)),
                                     (a_dev, a, dict(weight=w1, out_scale=scale)), (b_dev, b, dict(weight=w0, first=True, out_scale=scale))):
                got = ops.ensemble_accumulate(src_dev, acc_dev, flip=flip, kind=kind, **kw)
                ops.ensemble_accumulate_torch(src, acc, flip=flip, kind=kind, **kw)
                assert got is acc_dev and not bool(torch.isnan(acc_dev).any())
                assert torch.equal(acc_dev.cpu(), acc), (flip, per_class, kw.keys())
            if kind == "vote":
                want = torch.stack([(ops.first_max_argmax(torch.flip(b, [2 + i for i in range(3) if flip[i]])[0]) == c) for c in range(Cc)]).float()
                assert shape[0] > 1 or torch.equal(acc_dev.cpu()[0], want * torch.tensor(scale, dtype=torch.float32).reshape(-1, 1, 1, 1))


def test_eight_members_accumulate_like_the_restatement():
    ops = _ops()
    shape = (2, 5, 6, 7, 9)
    for kind in ("mean_logits", "vote"):
        acc_dev, acc = torch.empty(shape, device=DEV), torch.empty(shape)
        for k in range(8):
            x = torch.randn(shape, generator=torch.Generator().manual_seed(20 + k)) * 3
            kw = dict(flip=R.FLIPS[k], kind=kind, weight=0.5 + 0.25 * k, first=k == 0, out_scale=1.0 / sum(0.5 + 0.25 * j for j in range(8)) if k == 7 else None)
            ops.ensemble_accumulate(x.to(DEV), acc_dev, **kw)
            ops.ensemble_accumulate_torch(x, acc, **kw)
            assert torch.equal(acc_dev.cpu(), acc), (kind, k)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_mean_prob_against_float64(seed):
    """truth: the float64 computation; the kernel may be off by at most 4x the fp32 restatement's own largest error on the same input (two
    exp implementations, each good to an ulp or two; a wrong maximum or a dropped channel is off by 1e-2 or more)"""
    ops = _ops()
    g = torch.Generator().manual_seed(seed)
    shape = (2, 5, 6, 7, 9)
    members = [(torch.randn(shape, generator=g) * 3, R.FLIPS[k], 1.0) for k in range(8)]
    acc_dev, acc = torch.full(shape, float("nan"), device=DEV), torch.empty(shape)
    for k, (x, f, w) in enumerate(members):
        kw = dict(flip=f, kind="mean_prob", weight=w, first=k == 0, out_scale=0.125 if k == 7 else None)
        ops.ensemble_accumulate(x.to(DEV), acc_dev, **kw)
        ops.ensemble_accumulate_torch(x, acc, **kw)
    want, _ = R.fold64([(x.numpy(), f, w) for x, f, w in members], "mean_prob", scale=0.125)
    err_ref = float(np.abs(acc.numpy().astype(np.float64) - want).max())
    err_dev = float(np.abs(acc_dev.cpu().numpy().astype(np.float64) - want).max())
    left_out = R.class_map_agrees(acc_dev, want)
    print(f"mean_prob seed {seed}: largest error against float64: restatement {err_ref:.3e}, kernel {err_dev:.3e}; share under the 1e-5 gap {left_out:.4%}")
    assert err_dev <= 4 * err_ref, (err_dev, err_ref)
    # the other channel paths and a per-class weight, same rule
    for shp in ((1, 17, 3, 3, 8), (1, 64, 2, 2, 4), (1, 3, 5, 6, 7), (1, 8, 4, 6, 16)):
        x, y = torch.randn(shp, generator=g) * 3, torch.randn(shp, generator=g) * 3
        w = tuple((torch.rand(shp[1], generator=g) + 0.1).tolist())
        d, h = torch.empty(shp, device=DEV), torch.empty(shp)
        for fn, (p, q, out) in ((ops.ensemble_accumulate, (x.to(DEV), y.to(DEV), d)), (ops.ensemble_accumulate_torch, (x, y, h))):
            fn(p, out, flip=(True, False, True), kind="mean_prob", weight=w, first=True)
            fn(q, out, flip=(False, True, False), kind="mean_prob", weight=0.5, out_scale=0.25)
        truth, _ = R.fold64([(x.numpy(), (True, False, True), w), (y.numpy(), (False, True, False), 0.5)], "mean_prob", scale=0.25)
        e_ref, e_dev = (float(np.abs(t.cpu().numpy().astype(np.float64) - truth).max()) for t in (h, d))
        assert e_dev <= 4 * e_ref, (shp, e_dev, e_ref)


def test_abi_size_and_refusals():
    """every refused call fails on the host with a message before any launch: the accumulator keeps its bytes"""
    ops = _ops()
    from mi_seg_amd.hip import lib as L
    so = L.load()
    assert so.miseg_abi_struct_size(b"miseg_ensemble_params") == C.sizeof(L.Ensemble)
    assert so.miseg_abi_version() == 16
    shape = (1, 3, 2, 3, 4)
    buf = torch.zeros(2 * 72, device=DEV)
    src, acc = buf[:72].view(shape), buf[72:].view(shape)
    acc.fill_(7.0)

    def params(**kw):
        p = L.Ensemble(C.sizeof(L.Ensemble), src.data_ptr(), acc.data_ptr(), *shape, 0, 0, 1, 0)
        for c in range(64):
            p.weight[c] = 1.0
            p.out_scale[c] = 1.0
        for k, v in kw.items():
            if k in ("weight", "out_scale"):
                getattr(p, k)[v[0]] = v[1]
            else:
                setattr(p, k, v)
        return p

    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad = [dict(src=None), dict(acc=None), dict(C=0), dict(C=65), dict(B=0), dict(D=0), dict(H=-1), dict(W=0), dict(kind=3), dict(kind=-1), dict(flip=8),
           dict(flip=-1), dict(weight=(1, float("nan"))), dict(weight=(0, float("inf"))), dict(weight=(2, -0.5)),
           dict(scaled=1, out_scale=(1, float("nan"))), dict(struct_size=C.sizeof(L.Ensemble) - 4),
           dict(src=acc.data_ptr() + 4 * 8), dict(src=acc.data_ptr() - 4 * 71), dict(src=acc.data_ptr())]
    for kw in bad:
        rc = so.miseg_ensemble_accumulate(C.byref(params(**kw)), stream)
        assert rc < 0 and b"ensemble_accumulate" in so.miseg_last_error(), (kw, rc, so.miseg_last_error())
    torch.cuda.synchronize()
    assert bool((acc == 7.0).all())
    assert so.miseg_ensemble_accumulate(C.byref(params(weight=(3, float("nan")))), stream) == 0      # a weight beyond the C channels is not read
    assert so.miseg_ensemble_accumulate(C.byref(params(src=acc.data_ptr() - 4 * 72)), stream) == 0   # adjacent ranges do not overlap
    torch.cuda.synchronize()
    assert torch.equal(acc, src)
    for a, b in ((src, acc.cpu()), (src.double(), acc.double()), (src, buf[70:142].view(shape))):
        with pytest.raises(ValueError, match="ensemble_accumulate"):
            ops.ensemble_accumulate(a, b)


def test_graph_capture_on_a_side_stream():
    ops = _ops()
    shape = (1, 6, 8, 12, 16)
    a, b = (torch.randn(shape, generator=torch.Generator().manual_seed(s)).to(DEV) for s in (1, 2))
    acc = torch.empty(shape, device=DEV)

    def run():
        ops.ensemble_accumulate(a, acc, flip=(True, False, True), kind="mean_prob", weight=0.75, first=True)
        ops.ensemble_accumulate(b, acc, flip=(False, True, False), kind="mean_prob", weight=1.25, out_scale=0.5)

    run()
    eager = acc.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        run()
    acc.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(acc, eager)
    a.copy_(torch.randn(shape, generator=torch.Generator().manual_seed(3)))      # a replay reads the inputs anew
    g.replay()
    torch.cuda.synchronize()
    replayed = acc.clone()
    run()
    torch.cuda.synchronize()
    assert torch.equal(replayed, acc) and not torch.equal(acc, eager)


# ------------------------------------------------------------------------------------------ end to end
def _tiny(seed=None, C_out=6):
    """the fs=12 Swin-UNETR of test_hip_stitch_gaussian.py at roi 32^3; `seed`: a differently seeded one (the deterministic fill plus noise)"""
    from mi_seg_amd.networks.nets.swin_unetr import SwinUNETR
    from mi_seg_amd.networks.norms.utils import parse_normalization
    from mi_seg_amd.utils.detfill import fill_module_
    norm = lambda name: parse_normalization(name, True, 4, 2)
    m = SwinUNETR((32,) * 3, 1, C_out, feature_size=12, num_heads=(3, 6, 12, 24), vit_norm_name=norm("instance_cond"),
                  encoder_norm_name=norm("instance_cond"), decoder_norm_name=norm("instance"))
    fill_module_(m)
    if seed is not None:
        _perturb(m, seed)
    return m.to(DEV).eval()


def _perturb(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))


@pytest.fixture(scope="module")
def models():
    return _tiny(), _tiny(seed=7)


@pytest.mark.parametrize("blend", ["constant", "gaussian"])
def test_ensemble_inferer_equals_the_explicit_loop(models, blend):
    """flips over axes (0, 2) of a 40 x 36 x 33 volume, roi 32^3, overlap 0.25: bit for bit the torch loop flip -> sliding_window_inference ->
    flip back -> sequential sum; two models: the vote and mean_logits class maps are the torch compositions'"""
    ops = _ops()
    from mi_seg_amd.training.ensemble import EnsembleInferer, tta_flip_sets
    from mi_seg_amd.training.inferer import sliding_window_inference
    from mi_seg_amd.utils.detfill import det_input
    vol = det_input(5, (1, 1, 40, 36, 33)).to(DEV)
    mod = torch.tensor([1], device=DEV)
    flips = tta_flip_sets((0, 2))
    run = lambda x, p: sliding_window_inference(x, 32, 2, p, overlap=0.25, modalities=mod, mode=blend)
    with torch.no_grad():
        plain = run(vol, models[0])
        got = EnsembleInferer(models[0], 32, 2, 0.25, flips=flips, mode="mean_logits", infer_mode=blend)(vol, modalities=mod)
        want = R.loop_reference(vol, models[:1], flips, run)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == plain.shape
        assert torch.equal(got, want) and not torch.equal(got, plain)
        assert torch.equal(EnsembleInferer(models[0], 32, 2, 0.25, infer_mode=blend)(vol, modalities=mod), plain)      # one member: the plain inferer
        for mode in ("mean_logits", "vote"):
            got = EnsembleInferer(list(models), 32, 2, 0.25, flips=flips, mode=mode, infer_mode=blend)(vol, modalities=mod)
            want = R.loop_reference(vol, models, flips, run, mode)
            assert torch.equal(ops.first_max_argmax(got[0]), ops.first_max_argmax(want[0])) and torch.equal(got, want), mode
        assert float(got.sum(1).min()) == float(got.sum(1).max()) == 8.0                                                # vote counts of 8 members


def test_evaluate_with_the_ensemble_inferer(models):
    """evaluate.test takes the ensemble inferer like the plain one: the same result keys, and the Dice of the CPU run of the same loop (the
    members' logits folded by the torch restatement on the host)"""
    ops = _ops()
    from functools import partial
    from mi_seg_amd.training import evaluate as E
    from mi_seg_amd.training import metrics as M
    from mi_seg_amd.training.ensemble import EnsembleInferer, tta_flip_sets
    from mi_seg_amd.training.inferer import sliding_window_inference
    from mi_seg_amd.utils.detfill import det_input
    Cc = 6
    flips = tta_flip_sets((1,))
    loader = [{"image": det_input(i, (1, 1, 40, 36, 32)), "label": torch.randint(0, Cc, (1, 1, 40, 36, 32), generator=torch.Generator().manual_seed(i)).float(),
               "modality": torch.tensor([i % 2])} for i in range(2)]
    kw = dict(roi_size=(32, 32, 32), sw_batch_size=2, overlap=0.5)
    ens = EnsembleInferer(list(models), kw["roi_size"], kw["sw_batch_size"], kw["overlap"], flips=flips, mode="mean_logits")

    def on_host(x, modalities=None):                  # the same loop with the fold on the host
        acc, k = None, 0
        for m in models:
            for f in flips:
                dims = [2 + a for a in range(3) if f[a]]
                logits = sliding_window_inference(torch.flip(x, dims).to(DEV), predictor=m, modalities=modalities, **kw).cpu()
                acc = torch.empty_like(logits) if acc is None else acc
                k += 1
                ops.ensemble_accumulate(logits, acc, flip=f, kind="mean_logits", first=k == 1, out_scale=0.25 if k == 4 else None)
        return acc

    def run(device, inferer):
        res = {}
        ret = E.test(models[0], loader, device, M.DiceMetric(include_background=True, reduction="mean_batch", get_not_nans=True), E.AsDiscrete(to_onehot=Cc),
                     E.AsDiscrete(argmax=True, to_onehot=Cc), model_inferer=inferer, amp=False, results=res)
        return ret, res

    ret_plain, res_plain = run(DEV, partial(sliding_window_inference, predictor=models[0], **kw))
    ret_dev, res_dev = run(DEV, ens)
    ret_cpu, res_cpu = run("cpu", on_host)
    assert res_dev.keys() == res_plain.keys() == res_cpu.keys()
    for part in res_dev:
        assert res_dev[part].keys() == res_plain[part].keys() == res_cpu[part].keys()
        assert list(res_dev[part].values()) == pytest.approx(list(res_cpu[part].values()), rel=1e-6, nan_ok=True), part
    assert ret_dev == pytest.approx(ret_cpu, rel=1e-6)


def test_predict_command_with_an_ensemble_and_flips(tmp_path, capsys):
    """predict_whs.py's main with --ensemble_checkpoints and --infer_tta_flips 0 1 2: the written label map is the export of the torch-composed
    ensemble; without the new flags the file is the plain export's, byte for byte"""
    from mi_seg_amd.data import nifti as N
    from mi_seg_amd.data import preprocess as P
    from mi_seg_amd.data.checkpoint import export_state
    from mi_seg_amd.networks.utils.utils import model_from_argparse_args
    from mi_seg_amd.training import predict as PR
    from mi_seg_amd.training.ensemble import tta_flip_sets
    from mi_seg_amd.training.inferer import sliding_window_inference
    from mi_seg_amd.utils.detfill import fill_module_
    from test_hip_predict import MODEL_ARGS
    data = tmp_path / "data"
    (data / "imagesTs").mkdir(parents=True)
    ct = np.random.default_rng(11).normal(0, 300, (41, 37, 23)).astype(np.int16)
    A = np.array([[-0.7 * 0.98, 0.8 * 0.17, 0.0, 120.0], [-0.7 * 0.17, -0.8 * 0.98, 0.0, 95.5], [0.0, 0.0, 1.6, -210.0], [0, 0, 0, 1.0]])
    image = str(data / "imagesTs" / "ct_test_2001_image.nii.gz")
    N.write_nifti(image, ct, A)
    (data / "CT_test.json").write_text(json.dumps({"modality": {"0": "CT"}, "test": [{"image": "imagesTs/ct_test_2001_image.nii.gz"}]}))
    args = PR.build_parser().parse_args(MODEL_ARGS)
    args.feature_size = args.feature_size[0]
    nets, cks = [], []
    for i in range(2):
        m = model_from_argparse_args(args)
        fill_module_(m)
        if i:
            _perturb(m, 7)
        cks.append(str(tmp_path / f"ck{i}.pt"))
        export_state(m, cks[-1])
        nets.append(m.to(DEV).eval())
    common = MODEL_ARGS + ["--checkpoint", cks[0], "--data_dir", str(data), "--json_list", "CT_test.json"]
    roi = (32, 32, 32)
    vol, geom = P.load_image_for_prediction(image, (1.0, 1.0, 1.0), roi, DEV)
    mod = torch.tensor([0], device=DEV)
    run = lambda x, p: sliding_window_inference(x, roi, args.sw_batch_size, p, overlap=args.infer_overlap, modalities=mod)
    lut = PR.label_lut(8)
    plain = PR.main(common + ["--result_dir", str(tmp_path / "plain")])
    assert "(1 member" in capsys.readouterr().out
    with torch.no_grad():
        want_plain = PR.to_host(PR.invert_prediction(run(vol, nets[0]), geom, lut))
    assert np.array_equal(N.read_nifti(plain[0])[0], want_plain)
    for extra, mode in ((["--ensemble_checkpoints", cks[1], "--infer_tta_flips", "0", "1", "2"], "mean_logits"),
                        (["--ensemble_checkpoints", cks[1], "--infer_tta_flips", "0", "1", "2", "--ensemble_mode", "vote"], "vote")):
        paths = PR.main(common + ["--result_dir", str(tmp_path / mode)] + extra)
        assert "(16 members" in capsys.readouterr().out
        with torch.no_grad():
            want = PR.to_host(PR.invert_prediction(R.loop_reference(vol, nets, tta_flip_sets((0, 1, 2)), run, mode), geom, lut))
        arr, aff = N.read_nifti(paths[0])
        assert arr.dtype == np.uint16 and arr.shape == ct.shape and np.allclose(aff, A, atol=1e-5)
        assert np.array_equal(arr, want) and not np.array_equal(arr, want_plain)
    again = PR.main(common + ["--result_dir", str(tmp_path / "again"), "--ensemble_mode", "vote"])      # a mode without members changes nothing
    assert open(again[0], "rb").read() == open(plain[0], "rb").read()
