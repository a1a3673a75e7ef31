"""GPU tests of the soft prediction export (csrc/export_soft.hip::miseg_soft_export, hip/ops.py::soft_export, training/predict.py's
--invert_mode trilinear / --save_probabilities) against the numpy restatement of tests/soft_export_ref.py: bit identity of labels and fp32
scores without the softmax on every orientation, sampling, channel count, label width, output form and tile edge, the softmax within its
derived tolerance, the all-zero-t case against the nearest export, the ABI refusals, graph capture, the full MM-WHS size and the command end
to end."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import soft_export_ref as ref
from test_hip_predict import MODEL_ARGS, SAMPLING, bits, same
from test_predict_cpu import REF_MAP, make_geom
from test_soft_export_cpu import nan_rule_scores, np_tables, orientation_geom, scores_for

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mods():
    from mi_seg_amd.data import nifti, preprocess
    from mi_seg_amd.hip import lib, ops
    from mi_seg_amd.training import predict
    return nifti, preprocess, ops, lib, predict


def unsigned(t):
    """a label tensor on the host as a numpy array of its own unsigned width"""
    return bits(t).cpu().numpy().view({1: np.uint8, 2: np.uint16, 4: np.uint32}[t.element_size()])


def check_bits(g, x, Cc, dtype=torch.uint16, form="both", tables=None):
    """device labels and fp32 scores of softmax=False equal the restatement bit for bit"""
    _, _, ops, _, R = _mods()
    tables, axes = tables or g.lerp_tables()
    lut = R.label_lut(Cc)
    labels, prob = ops.soft_export(x.to(DEV), tables, axes, lut, dtype, softmax=False, want_labels=form != "scores",
                                   probabilities=None if form == "labels" else torch.float32)
    want = ref.blend(x.numpy(), np_tables(tables), axes)
    assert (labels is None) == (form == "scores") and (prob is None) == (form == "labels")
    if prob is not None:
        assert prob.is_cuda and prob.dtype == torch.float32 and tuple(prob.shape) == (Cc,) + tuple(reversed(g.file_shape)) and prob.is_contiguous()
        assert np.array_equal(prob.cpu().numpy().view(np.uint32), want.view(np.uint32))
    if labels is not None:
        assert labels.is_cuda and labels.dtype == dtype and tuple(labels.shape) == tuple(reversed(g.file_shape)) and labels.is_contiguous()
        assert np.array_equal(unsigned(labels), ref.labels(want, lut.numpy(), labels.element_size()))


@pytest.mark.parametrize("i", range(48))
def test_bits_every_orientation(i):
    g = orientation_geom(i)
    check_bits(g, scores_for(g, 8, i), 8)
    check_bits(g, scores_for(g, 8, i, tied=True), 8)


@pytest.mark.parametrize("case", range(len(SAMPLING)))
@pytest.mark.parametrize("Cc", [2, 8, 14])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16, torch.uint32])
def test_bits_sampling_channels_widths(case, Cc, dtype):
    g = make_geom(*SAMPLING[case])
    check_bits(g, scores_for(g, Cc, 100 * case + Cc), Cc, dtype)


@pytest.mark.parametrize("form", ["labels", "scores", "both"])
@pytest.mark.parametrize("Cc", [1, 64])
def test_bits_channel_limits_and_output_forms(form, Cc):
    g = make_geom(*SAMPLING[2])
    check_bits(g, scores_for(g, Cc, Cc), Cc, form=form)
    if Cc == 64:
        check_bits(g, scores_for(g, Cc, Cc, tied=True), Cc, form=form)


EDGES = [
    # file sides of 65 and 129 in every tile role (X, the tile's second axis, the plane axis): ragged 64-tiles on each
    ((65, 129, 6), (0, 1, 2), (False, True, False), (40, 129, 9), (1, 0, 2), (0, 3, 0)),
    ((129, 6, 65), (2, 0, 1), (True, False, False), (33, 150, 6), (0, 2, 0), (1, 0, 0)),
    ((6, 65, 129), (1, 2, 0), (False, False, True), (65, 70, 3), (0, 0, 1), (0, 0, 1)),
    ((63, 64, 5), (2, 1, 0), (True, True, True), (5, 64, 30), (0, 0, 0), (0, 0, 0)),
    # a strong downsampling: the source span of a tile exceeds the LDS image, the taps are read from memory
    ((20, 6, 21), (0, 1, 2), (False, True, False), (200, 12, 150), (0, 1, 0), (2, 0, 0)),
    ((21, 20, 6), (1, 2, 0), (True, False, False), (200, 12, 150), (0, 0, 3), (0, 0, 0)),
]


@pytest.mark.parametrize("case", range(len(EDGES)))
def test_bits_tile_edges_and_the_unstaged_path(case):
    g = make_geom(*EDGES[case])
    check_bits(g, scores_for(g, 3, case), 3)
    check_bits(g, scores_for(g, 3, case, tied=True), 3, torch.uint8)


def test_uint8_scores_of_a_declared_unit_range():
    """scores the caller declares to lie in [0, 1] (an ensemble's mean probabilities): blended as given, quantised as the restatement does"""
    _, _, ops, _, _ = _mods()
    g = make_geom(*SAMPLING[0])
    x = scores_for(g, 6, 9).sigmoid()
    x[2, 3, 4, 5] = float("nan")                   # a NaN quantises to 0
    tables, axes = g.lerp_tables()
    labels, q = ops.soft_export(x.to(DEV), tables, axes, torch.arange(6), torch.uint8, softmax=False, probabilities=torch.uint8, unit_range=True)
    want = ref.blend(x.numpy(), np_tables(tables), axes)
    assert q.dtype == torch.uint8 and np.array_equal(q.cpu().numpy(), ref.quantize(want))
    assert np.array_equal(labels.cpu().numpy(), ref.labels(want, np.arange(6), 1))
    with pytest.raises(ValueError, match="uint8 probabilities need scores"):
        ops.soft_export(x.to(DEV), tables, axes, torch.arange(6), softmax=False, probabilities=torch.uint8)


def check_softmax(g, x, Cc, coords=None, dev_out=None):
    """device softmax=True against the restatement with numpy's exp: fp32 scores within the derived tolerance, labels equal wherever the
    restatement's top-two margin is at least 1e-5 (at most 0.2 % of the voxels are left out), uint8 scores within half a step more"""
    _, _, ops, _, _ = _mods()
    tables, axes = g.lerp_tables()
    lut = torch.arange(Cc, dtype=torch.int32)
    tol = ref.softmax_tolerance(Cc)
    want = ref.blend(ref.softmax(x.numpy()), np_tables(tables), axes, coords)
    if dev_out is None:
        xd = x.to(DEV)
        labels, prob = ops.soft_export(xd, tables, axes, lut, torch.uint8, softmax=True, probabilities=torch.float32)
        q = ops.soft_export(xd, tables, axes, lut, softmax=True, want_labels=False, probabilities=torch.uint8)[1]
        labels, prob, q = labels.cpu().numpy(), prob.cpu().numpy(), q.cpu().numpy()
    else:
        labels, prob, q = dev_out
    err = float(np.abs(prob - want).max())
    sure = ref.top_two_margin(want) >= 1e-5
    share = float((~sure).mean())
    print(f"softmax C {Cc} file {g.file_shape}: max |p - p_ref| = {err:.3e} (tolerance {tol:.3e}), thin-margin share {share:.2e}")
    assert err <= tol
    assert share <= 2e-3
    assert np.array_equal(labels[sure], ref.labels(want, lut.numpy(), 1)[sure])
    assert (np.abs(q.astype(np.float64) - 255.0 * want.astype(np.float64)) <= 0.5 + 255.0 * tol).all()


@pytest.mark.parametrize("case", range(len(SAMPLING)))
@pytest.mark.parametrize("Cc", [2, 8, 14])
def test_softmax_within_the_derived_tolerance(case, Cc):
    g = make_geom(*SAMPLING[case])
    check_softmax(g, scores_for(g, Cc, 0), Cc)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16, torch.uint32])
def test_all_zero_t_is_the_nearest_export(dtype):
    _, _, ops, _, R = _mods()
    g = make_geom((9, 10, 11), (0, 1, 2), (False, False, False), (9, 10, 11), (0, 0, 0), (0, 0, 0))        # m == n, no pad
    x = nan_rule_scores(g.padded_shape)
    x[3, 4, 5, 6] = float("inf")                   # the hi tap of the voxel before it on every axis: must not leak
    lut = R.label_lut(5)
    xd = x.to(DEV)
    want = R.invert_prediction(xd, g, lut, dtype=dtype)
    got = R.invert_prediction(xd, g, lut, dtype=dtype, mode="trilinear", softmax=False)
    assert same(got, want) and got.permute(2, 1, 0).is_contiguous()
    tables, axes = g.lerp_tables()
    prob = ops.soft_export(xd, tables, axes, lut, softmax=False, want_labels=False, probabilities=torch.float32)[1]
    assert torch.equal(prob.view(torch.int32), xd.permute(0, 3, 2, 1).contiguous().view(torch.int32))
    for case in SAMPLING + EDGES[:2]:              # mode="nearest" tables on resampling geometries
        g = make_geom(*case)
        xd = scores_for(g, 5, 7).to(DEV)
        tables, axes = g.lerp_tables("nearest")
        labels, prob = ops.soft_export(xd, tables, axes, lut, dtype, softmax=False, probabilities=torch.float32)
        assert same(labels.permute(2, 1, 0), R.invert_prediction(xd, g, lut, dtype=dtype))
        gathered = xd
        for a in range(3):
            gathered = gathered.index_select(1 + axes[a], tables[a][0].to(DEV).long())
        assert torch.equal(prob.view(torch.int32), gathered.permute(0, 1 + axes[2], 1 + axes[1], 1 + axes[0]).contiguous().view(torch.int32))


class AbiCall:
    """miseg_soft_export through the C ABI on prepared tensors (nothing is allocated or copied by call())"""

    def __init__(self, x, tables, axes, lut, dtype=torch.uint16, softmax=False, probabilities=None, want_labels=True, unit_range=False):
        _, _, _, L, _ = _mods()
        self.so, self.L = L.load(), L
        self.x = x.to(DEV).contiguous()
        self.host = [tuple(v.contiguous() for v in t) for t in tables]
        self.dev = [tuple(v.to(DEV) for v in t) for t in self.host]
        Cc, dims = self.x.shape[0], tuple(self.x.shape[1:])
        n = [t[0].numel() for t in self.host]
        box = [None] * 3
        for a in range(3):
            lo, hi = int(self.host[a][0].min()), int(self.host[a][1].max())
            box[axes[a]] = (lo, hi - lo + 1)
        self.lut = lut.to(DEV, torch.int32)
        nbytes = int(self.so.miseg_soft_export_workspace_bytes(Cc, box[0][1], box[1][1], box[2][1], int(softmax)))
        self.ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV)
        self.out = torch.zeros(n[2], n[1], n[0], dtype=dtype, device=DEV) if want_labels else None
        self.prob = torch.zeros(Cc, n[2], n[1], n[0], dtype=probabilities, device=DEV) if probabilities is not None else None
        vp3 = C.c_void_p * 3
        self.fields = dict(
            struct_size=C.sizeof(L.SoftExport), scores=self.x.data_ptr(), C=Cc, D=dims[0], H=dims[1], W=dims[2], box_d0=box[0][0], box_h0=box[1][0],
            box_w0=box[2][0], box_nd=box[0][1], box_nh=box[1][1], box_nw=box[2][1], nx=n[0], ny=n[1], nz=n[2], axis_x=axes[0], axis_y=axes[1],
            axis_z=axes[2], lo=vp3(*(t[0].data_ptr() for t in self.dev)), hi=vp3(*(t[1].data_ptr() for t in self.dev)),
            t=vp3(*(t[2].data_ptr() for t in self.dev)), lo_host=vp3(*(t[0].data_ptr() for t in self.host)),
            hi_host=vp3(*(t[1].data_ptr() for t in self.host)), lut=self.lut.data_ptr(), softmax=int(softmax), unit_range=int(unit_range),
            workspace=self.ws.data_ptr() if nbytes else None, out=self.out.data_ptr() if want_labels else None,
            out_bytes=self.out.element_size() if want_labels else 0, prob=self.prob.data_ptr() if self.prob is not None else None,
            prob_bytes=self.prob.element_size() if self.prob is not None else 0)

    def params(self, **kw):
        f = dict(self.fields)
        f.update(kw)
        return self.L.SoftExport(**f)

    def call(self, p=None):
        p = self.params() if p is None else p
        return self.so.miseg_soft_export(C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_abi_argument_checks():
    _, _, _, L, _ = _mods()
    g = make_geom((5, 6, 7), (0, 1, 2), (False, False, False), (6, 7, 8), (0, 0, 0), (0, 0, 0))
    tables, axes = g.lerp_tables()
    x = scores_for(g, 4, 2)
    lut = torch.arange(4, dtype=torch.int32) + 1
    a = AbiCall(x, tables, axes, lut, probabilities=torch.float32)
    assert a.call() == 0
    torch.cuda.synchronize()
    want = ref.blend(x.numpy(), np_tables(tables), axes)
    assert np.array_equal(a.prob.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(unsigned(a.out), ref.labels(want, lut.numpy(), 2))
    a.out.zero_()
    a.prob.zero_()
    BAD, UNSUPPORTED = -1, -2
    vp3 = C.c_void_p * 3

    def table(which, axis, i, v):
        """host copies of lo / hi with one entry changed (kept alive on `a`)"""
        t = [a.host[k][which].clone() for k in range(3)]
        t[axis][i] = v
        a.keep = getattr(a, "keep", []) + [t]
        return vp3(*(v.data_ptr() for v in t))

    hi1 = int(a.host[1][1][2])
    cases = [
        (dict(struct_size=8), BAD, "struct_size"), (dict(out=None, prob=None), BAD, "both outputs are null"), (dict(scores=None), BAD, "null pointer"),
        (dict(lut=None), BAD, "null pointer"), (dict(t=vp3(None, None, None)), BAD, "null table"), (dict(lo_host=vp3(None, None, None)), BAD, "null table"),
        (dict(C=0), BAD, "C 0"), (dict(C=65), BAD, "C 65"), (dict(out_bytes=3), BAD, "out_bytes"), (dict(prob_bytes=2), BAD, "prob_bytes"),
        (dict(prob_bytes=1), UNSUPPORTED, "uint8 scores need values in [0, 1]"), (dict(axis_z=1), BAD, "not a permutation"),
        (dict(box_nw=99), BAD, "leaves the side"), (dict(nx=0), BAD, "sides 1..65535"), (dict(softmax=1, workspace=None), BAD, "needs the workspace"),
        (dict(hi_host=table(1, 1, 2, hi1 + 1)), BAD, "outside [lo, lo + 1]"), (dict(hi_host=table(1, 0, 0, -1)), BAD, "leaves the box"),
        (dict(lo_host=table(0, 2, 3, 8)), BAD, "leaves the box"), (dict(box_d0=1, box_nd=5), BAD, "leaves the box"),
    ]
    assert hi1 == int(a.host[1][0][2]) + 1 and hi1 >= 2
    cases.append((dict(hi_host=table(1, 1, 2, hi1 - 2)), BAD, "outside [lo, lo + 1]"))                 # hi below lo
    for kw, code, text in cases:
        rc = a.call(a.params(**kw))
        assert rc == code, (kw, rc)
        assert text.encode() in a.so.miseg_last_error(), (kw, a.so.miseg_last_error())
    torch.cuda.synchronize()
    assert not bits(a.out).any() and not a.prob.any()           # nothing was launched
    assert a.so.miseg_soft_export_workspace_bytes(4, 3, 4, 5, 1) >= 4 * 60 * 4 and a.so.miseg_soft_export_workspace_bytes(4, 3, 4, 5, 0) == 0


def test_graph_capture_replays_the_same_result():
    g = make_geom(*SAMPLING[0])
    tables, axes = g.lerp_tables()
    x = scores_for(g, 8, 5)
    lut = torch.arange(8, dtype=torch.int32)
    a = AbiCall(x, tables, axes, lut, softmax=True, probabilities=torch.float32)
    assert a.call() == 0
    torch.cuda.synchronize()
    eager = (a.out.clone(), a.prob.clone())
    a.out.zero_()
    a.prob.zero_()
    p = a.params()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            assert a.call(p) == 0
    torch.cuda.synchronize()
    for _ in range(2):
        a.out.zero_()
        a.prob.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same(a.out, eager[0]) and torch.equal(a.prob.view(torch.int32), eager[1].view(torch.int32))


def _timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def test_full_size():
    """512 x 512 x 363 from 180 x 180 x 164 scores, 8 classes, the geometry of test_hip_predict.py::test_full_size: labels and scores at
    200 000 fixed-seed voxels against the restatement at those voxels; the times printed are information only"""
    _, _, ops, L, R = _mods()
    g = make_geom((512, 512, 363), (0, 1, 2), (True, True, False), (180, 180, 164), (0, 0, 2), (0, 0, 3))
    x = torch.randn((8,) + g.padded_shape, generator=torch.Generator().manual_seed(0))
    tables, axes = g.lerp_tables()
    lut = R.label_lut(8)
    rng = np.random.default_rng(0)
    coords = tuple(rng.integers(0, n, 200000) for n in g.file_shape)
    zyx = tuple(torch.from_numpy(coords[k]).to(DEV) for k in (2, 1, 0))

    def pick(t):
        """the sampled voxels of a device [(C,) nz, ny, nx] tensor, on the host"""
        return (bits(t) if not t.dtype.is_floating_point else t)[(..., *zyx)].cpu().numpy()

    a = AbiCall(x, tables, axes, lut, probabilities=torch.float32)
    ms = _timed(a.call)
    want = ref.blend(x.numpy(), np_tables(tables), axes, coords)
    assert np.array_equal(pick(a.prob).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(pick(a.out).view(np.uint16), ref.labels(want, lut.numpy(), 2))
    del a
    ident = torch.arange(8, dtype=torch.int32)
    a = AbiCall(x, tables, axes, ident, torch.uint8, softmax=True, probabilities=torch.float32)
    ms_soft = _timed(a.call)
    labels, prob = pick(a.out), pick(a.prob)
    del a
    a = AbiCall(x, tables, axes, ident, softmax=True, probabilities=torch.uint8, want_labels=False)
    assert a.call() == 0
    torch.cuda.synchronize()
    q = pick(a.prob)
    xd = a.x
    del a
    check_softmax(g, x, 8, coords, dev_out=(labels, prob, q))
    near_tables, near_axes = g.index_tables(DEV)
    ms_near = _timed(lambda: ops.label_export(xd, near_tables, near_axes, lut))
    print(f"full size 512x512x363 from 180x180x169, C 8: soft export labels + fp32 scores {ms:.2f} ms, with softmax {ms_soft:.2f} ms; "
          f"label_export (nearest, wrapper included) {ms_near:.2f} ms")


def test_predict_end_to_end_trilinear_with_probabilities(tmp_path, capsys):
    N, P, _, _, R = _mods()
    from mi_seg_amd.data.checkpoint import export_state
    from mi_seg_amd.networks.utils.utils import model_from_argparse_args
    from mi_seg_amd.training.inferer import sliding_window_inference
    from mi_seg_amd.utils.detfill import fill_module_
    data = tmp_path / "data"
    (data / "imagesTs").mkdir(parents=True)
    rng = np.random.default_rng(11)
    ct = rng.normal(0, 300, (41, 37, 23)).astype(np.int16)
    A = np.array([[-0.7 * 0.98, 0.8 * 0.17, 0.0, 120.0], [-0.7 * 0.17, -0.8 * 0.98, 0.0, 95.5], [0.0, 0.0, 1.6, -210.0], [0, 0, 0, 1.0]])
    image = "imagesTs/ct_test_2001_image.nii.gz"
    N.write_nifti(str(data / image), ct, A)
    (data / "CT_test.json").write_text(json.dumps({"modality": {"0": "CT"}, "test": [{"image": image}]}))
    args = R.build_parser().parse_args(MODEL_ARGS)
    args.feature_size = args.feature_size[0]
    model = model_from_argparse_args(args)
    fill_module_(model)
    ck = str(tmp_path / "ck.pt")
    export_state(model, ck)

    def run(out_dir, *extra):
        paths = R.main(MODEL_ARGS + ["--checkpoint", ck, "--data_dir", str(data), "--json_list", "CT_test.json", "--result_dir", str(out_dir)] + list(extra))
        assert paths == [str(out_dir / "ct_test_2001_label.nii.gz")]
        return paths[0]

    soft = ["--invert_mode", "trilinear", "--save_probabilities", "--probability_dtype", "uint8"]
    filtered = run(tmp_path / "r1", *soft, "--keep_largest")
    arr, aff = N.read_nifti(filtered)
    assert arr.dtype == np.uint16 and arr.shape == ct.shape and np.allclose(aff, A, atol=1e-5)
    assert set(np.unique(arr).tolist()) <= {0} | set(REF_MAP.values())
    printed = capsys.readouterr().out
    assert "inverse (trilinear)" in printed and "probabilities (uint8) device-to-host + write" in printed and "keep-largest" in printed
    prob_path = str(tmp_path / "r1" / "ct_test_2001_label_prob.nii.gz")
    prob, paff = N.read_nifti(prob_path)
    assert prob.shape == ct.shape + (8,) and prob.dtype == np.float32 and np.allclose(paff, A, atol=1e-5)
    q = np.rint(prob * 255.0).astype(np.int64)
    assert np.abs(q / 255.0 - prob).max() < 1e-6 and q.min() >= 0 and q.max() <= 255
    assert (np.abs(prob.astype(np.float64).sum(-1) - 1.0) <= 3.0 / 255.0 + 1e-6).all()
    unfiltered = run(tmp_path / "r2", *soft)
    assert open(prob_path, "rb").read() == open(str(tmp_path / "r2" / "ct_test_2001_label_prob.nii.gz"), "rb").read()
    codes = N.read_nifti(unfiltered)[0]
    inverse = {v: k for k, v in REF_MAP.items()}
    cls = np.vectorize(lambda v: inverse.get(int(v), int(v)))(codes)
    top = np.sort(q, axis=-1)
    clear = top[..., -1] > top[..., -2]
    assert clear.any() and np.array_equal(q.argmax(-1)[clear], cls[clear])
    assert ((arr == codes) | (arr == 0)).all()                 # keep-largest only ever clears voxels
    # the same command without the new options: the bytes invert_prediction(mode="nearest") gives
    plain = run(tmp_path / "r3")
    assert not os.path.exists(str(tmp_path / "r3" / "ct_test_2001_label_prob.nii.gz"))
    # --save_probabilities alone: the nearest export's bytes, and the fp32 softmax under the same gather beside them
    near = run(tmp_path / "r5", "--save_probabilities")
    assert open(near, "rb").read() == open(plain, "rb").read()
    pn, _ = N.read_nifti(str(tmp_path / "r5" / "ct_test_2001_label_prob.nii.gz"))
    assert pn.shape == ct.shape + (8,) and pn.dtype == np.float32 and np.abs(pn.sum(-1) - 1.0).max() < 1e-5
    top = np.sort(pn, axis=-1)
    clear = top[..., -1] > top[..., -2]
    near_cls = np.vectorize(lambda v: inverse.get(int(v), int(v)))(N.read_nifti(near)[0])
    assert clear.any() and np.array_equal(pn.argmax(-1)[clear], near_cls[clear])
    model = model.to(DEV).eval()
    roi = (32, 32, 32)
    vol, g = P.load_image_for_prediction(str(data / image), (1.0, 1.0, 1.0), roi, DEV)
    with torch.no_grad():
        logits = sliding_window_inference(vol, roi, args.sw_batch_size, model, overlap=args.infer_overlap, modalities=torch.tensor([0], device=DEV))
    want = R.to_host(R.invert_prediction(logits, g, R.label_lut(8), mode="nearest"))
    (tmp_path / "r4").mkdir()
    N.write_nifti(str(tmp_path / "r4" / "ct_test_2001_label.nii.gz"), want, g.affine, compresslevel=R.COMPRESSLEVEL, mtime=0)
    assert open(plain, "rb").read() == open(str(tmp_path / "r4" / "ct_test_2001_label.nii.gz"), "rb").read()
