"""Prediction export: the reference's predict_whs.py (35-114).  Each image of a data list's "test" entries goes through the prediction transforms
(data/preprocess.py::load_image_for_prediction), the sliding-window inference with its modality, and then the way back - argmax, the inverse
of the pad, the spacing and the orientation, the MM-WHS label codes - as one miseg_label_export call on the device, into a uint16 NIfTI
label map in the image's own grid and affine.  --keep_largest puts MONAI's KeepLargestConnectedComponent between the
argmax and the way back, on the device (hip/ops.py::keep_largest_component); --fill_holes puts MONAI's FillHoles
there too, after the keep-largest filter when both are given (hip/ops.py::fill_holes).  --invert_mode trilinear
blends the class scores onto the image grid before the argmax and --save_probabilities writes them beside the label map
(hip/ops.py::soft_export); both are off by default."""
import os
import time
from argparse import ArgumentParser

import numpy as np
import torch

from ..data.checkpoint import load_model_state
from ..data.decathlon import load_decathlon_datalist_with_modality, modality_id
from ..data.nifti import write_nifti
from ..data.preprocess import load_image_for_prediction
from ..hip import ops
from ..networks.utils.utils import model_from_argparse_args
from ..utils.parser import add_model_argparse_args
from .ensemble import EnsembleInferer, tta_flip_sets
from .inferer import sigma_scale_arg, sliding_window_inference

LABEL_MAP = {1: 500, 2: 600, 3: 420, 4: 550, 5: 205, 6: 820, 7: 850}      # predict_whs.py:18-26 (_MAP): class -> MM-WHS label code
NO_GPU_MESSAGE = "predict_whs: the model and the label export run on the HIP device only (--no_gpu given, or no device visible)"
COMPRESSLEVEL = 1        # gzip level of a .nii.gz label map (level 9 of a 190 MB volume costs seconds on one core for a few % of size)


def label_lut(C, mapping=LABEL_MAP):
    """int32 [C]: the class code each class index is written as, the reference's remap_tensor (one masked assignment per key, in order)
    restated per class; a class without a key keeps its index"""
    lut = []
    for c in range(C):
        v = c
        for key, value in mapping.items():
            if v == key:
                v = value
        lut.append(v)
    return torch.tensor(lut, dtype=torch.int32)


INVERT_MODES = ("nearest", "trilinear")
INVERT_QUANTITIES = ("probabilities", "logits")
PROBABILITY_DTYPES = {"float32": torch.float32, "uint8": torch.uint8}
VOTE_UINT8_MESSAGE = ("predict_whs: --probability_dtype uint8 needs values in [0, 1]; --ensemble_mode vote leaves vote counts, which are not "
                      "normalised: use --probability_dtype float32, or --ensemble_mode mean_prob")


def invert_prediction(logits, geometry, lut, dtype=torch.uint16, pred=None, mode="nearest", softmax=True):
    """logits [(1,) C, D, H, W] on the padded, resampled RAS grid -> label map in the file's grid: an [X, Y, Z] view of a C-contiguous [Z, Y, X]
    buffer (the file's Fortran order), lut[first-maximum argmax] per voxel.  Device logits take miseg_label_export, CPU logits the same
    arithmetic in torch (hip/ops.py::label_export).  pred= (logits None): a uint8 / int32 class map [(1,) D, H, W] of len(lut) classes on that
    grid instead of the logits' argmax.  mode "trilinear": the scores - the softmax of the logits, or the values as given with softmax=False -
    are blended onto the file's grid before the argmax (hip/ops.py::soft_export); logits only."""
    if mode not in INVERT_MODES:
        raise ValueError(f"invert_prediction: mode {mode!r} is not one of {INVERT_MODES}")
    src = logits if pred is None else pred
    shape = tuple(src.shape[-3:])
    if shape != geometry.padded_shape:
        raise ValueError(f"invert_prediction: logits grid {shape} is not the geometry's padded grid {geometry.padded_shape}")
    if mode == "trilinear":
        if pred is not None:
            raise ValueError("invert_prediction: mode 'trilinear' blends scores, a class map has none")
        tables, axes = geometry.lerp_tables("trilinear")
        return ops.soft_export(logits, tables, axes, lut, dtype, softmax=softmax)[0].permute(2, 1, 0)
    tables, axes = geometry.index_tables(src.device if src.is_cuda else None)
    return ops.label_export(logits, tables, axes, lut, dtype, pred=pred).permute(2, 1, 0)


def score_kind(args):
    """what the inferer's output holds: "logits" (one member, or the mean of logits), "mean_prob" (probabilities) or "vote" (vote counts)"""
    members = (1 + len(getattr(args, "ensemble_checkpoints", None) or [])) * len(tta_flip_sets(getattr(args, "infer_tta_flips", None) or ()))
    mode = getattr(args, "ensemble_mode", "mean_logits")
    return "logits" if members == 1 or mode == "mean_logits" else mode


def export_options(args):
    """the checked export options of the command line: dict(mode, quantity, save, dtype (torch), kind); the default is the reference's way back
    (nearest, no probability file).  Refuses uint8 probabilities of vote counts."""
    opt = dict(mode=getattr(args, "invert_mode", "nearest"), quantity=getattr(args, "invert_quantity", "probabilities"),
               save=bool(getattr(args, "save_probabilities", False)), kind=score_kind(args))
    name = getattr(args, "probability_dtype", "float32")
    if opt["mode"] not in INVERT_MODES or opt["quantity"] not in INVERT_QUANTITIES or name not in PROBABILITY_DTYPES:
        raise SystemExit(f"predict_whs: --invert_mode {opt['mode']} / --invert_quantity {opt['quantity']} / --probability_dtype {name}")
    opt["dtype"] = PROBABILITY_DTYPES[name]
    if opt["save"] and opt["dtype"] == torch.uint8 and opt["kind"] == "vote":
        raise SystemExit(VOTE_UINT8_MESSAGE)
    return opt


def probability_path(label_path):
    """<label name minus extension>_prob.nii.gz beside the label map"""
    for ext in (".nii.gz", ".nii"):
        if label_path.endswith(ext):
            return label_path[:-len(ext)] + "_prob.nii.gz"
    return label_path + "_prob.nii.gz"


def _identity_tables(shape_zyx):
    """tables / axes with which label_export maps a class map [Z, Y, X] on the file's grid onto itself through the lut"""
    return [torch.arange(n, dtype=torch.int32) for n in reversed(shape_zyx)], (2, 1, 0)


def keep_largest_options(args):
    """the keyword arguments of ops.keep_largest_component the command line asks for, None without --keep_largest"""
    if not getattr(args, "keep_largest", False):
        return None
    return dict(applied_labels=getattr(args, "keep_largest_labels", None), independent=not getattr(args, "keep_largest_joint", False),
                connectivity=getattr(args, "keep_largest_connectivity", 3))


def fill_holes_options(args):
    """the keyword arguments of ops.fill_holes the command line asks for, None without --fill_holes"""
    if not getattr(args, "fill_holes", False):
        return None
    return dict(applied_labels=getattr(args, "fill_holes_labels", None), connectivity=getattr(args, "fill_holes_connectivity", 3))


def to_host(label_xyz):
    """device [X, Y, Z] view of a [Z, Y, X] buffer -> numpy [X, Y, Z] in Fortran order, copied as it lies (no transpose on either side)"""
    buf = label_xyz.permute(2, 1, 0)
    if not buf.is_contiguous():
        raise ValueError("to_host: not a view of a C-contiguous [Z, Y, X] buffer")
    host = torch.empty(buf.shape, dtype=buf.dtype, pin_memory=buf.is_cuda)
    host.copy_(buf)
    return host.numpy().transpose(2, 1, 0)


def output_path(image_path, result_dir):
    """the reference's file name: the image's basename with "image" replaced by "label", under result_dir"""
    return os.path.join(result_dir, os.path.basename(image_path).replace("image", "label"))


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)
    return time.perf_counter()


def predict_volume(model, item, args):
    """one data-list item ({"image", "modality"}) -> path of the written label map; prints the time of each stage.  `model`: one model, or a
    list of them (--ensemble_checkpoints); more than one model or any --infer_tta_flips axis goes through an EnsembleInferer (DESIGN.md
    section 7.10), one model without flips makes the call it always made."""
    device = args.device
    roi = (args.roi_x, args.roi_y, args.roi_z)
    models = list(model) if isinstance(model, (list, tuple)) else [model]
    flips = tta_flip_sets(getattr(args, "infer_tta_flips", None) or ())
    t0 = time.perf_counter()
    image, geom = load_image_for_prediction(item["image"], (args.space_x, args.space_y, args.space_z), roi, device)
    t1 = _sync(device)
    modality = torch.tensor([modality_id(item.get("modality", 0))], device=device)
    blend = dict(sigma_scale=sigma_scale_arg(getattr(args, "infer_sigma_scale", 0.125)), padding_mode=getattr(args, "infer_padding_mode", "constant"))
    members = len(models) * len(flips)
    if members > 1:
        inferer = EnsembleInferer(models, roi, args.sw_batch_size, args.infer_overlap, flips=flips, mode=getattr(args, "ensemble_mode", "mean_logits"),
                                  infer_mode=getattr(args, "infer_mode", "constant"), **blend)
        logits = inferer(image, modalities=modality)
    else:
        logits = sliding_window_inference(image, roi, args.sw_batch_size, models[0], overlap=args.infer_overlap, modalities=modality,
                                          mode=getattr(args, "infer_mode", "constant"), **blend)
    del image
    t2 = _sync(device)
    keep, fill = keep_largest_options(args), fill_holes_options(args)
    opt = export_options(args)
    filtered, tk, prob = "", t2, None
    if opt["mode"] == "trilinear":
        label, prob, filtered, tk = _soft_inverse(logits, geom, opt, keep, fill, device, t2)
    elif keep is None and fill is None:
        label = invert_prediction(logits, geom, label_lut(logits.shape[1]))
    else:
        cls = None
        if keep is not None:
            cls, stats = ops.keep_largest_component(logits=logits, stats=True, **keep)
            tk = _sync(device)
            removed = (stats[0, :, 0] - stats[0, :, 1]).tolist()          # (read back after the stage was timed)
            filtered = f"keep-largest {1e3 * (tk - t2):.2f} ms (voxels removed per class: {removed}), "
        if fill is not None:
            tf = tk
            cls, filled = ops.fill_holes(logits=logits if cls is None else None, pred=cls, num_classes=logits.shape[1], stats=True, **fill)
            tk = _sync(device)
            filtered += f"fill-holes {1e3 * (tk - tf):.2f} ms (voxels filled per class: {filled[0].tolist()}), "
        label = invert_prediction(None, geom, label_lut(logits.shape[1]), pred=cls[0])
        del cls
    if opt["mode"] == "nearest" and opt["save"]:  # the scores under the nearest gather: the same tables with t = 0
        tables, axes = geom.lerp_tables("nearest")
        prob = ops.soft_export(logits, tables, axes, label_lut(logits.shape[1]), softmax=opt["kind"] == "logits", want_labels=False,
                               probabilities=opt["dtype"], unit_range=opt["kind"] == "mean_prob")[1]
    del logits                                    # the next volume's inference starts without this one's logits
    t3 = _sync(device)
    host = to_host(label)
    del label
    t4 = time.perf_counter()
    path = output_path(item["image"], args.result_dir)
    write_nifti(path, host, geom.affine, compresslevel=COMPRESSLEVEL, mtime=0)
    t5 = time.perf_counter()
    saved = ""
    if prob is not None:
        scores = prob.cpu().numpy().transpose(3, 2, 1, 0)                 # [C, Z, Y, X] buffer -> [X, Y, Z, C] in Fortran order, as it lies
        del prob
        write_nifti(probability_path(path), scores, geom.affine, compresslevel=COMPRESSLEVEL, mtime=0,
                    scl_slope=1.0 / 255.0 if scores.dtype == np.uint8 else 1.0)
        saved = f", probabilities ({scores.dtype.name}) device-to-host + write {time.perf_counter() - t5:.3f} s"
    print(f"{os.path.basename(path)}: {'x'.join(str(s) for s in host.shape)} read+preprocess {t1 - t0:.3f} s, inference {t2 - t1:.3f} s "
          f"({members} member{'s' if members > 1 else ''}: models {len(models)} x flips {len(flips)}), "
          f"{filtered}inverse ({opt['mode']}) {1e3 * (t3 - tk):.2f} ms, device-to-host {1e3 * (t4 - t3):.2f} ms, write {t5 - t4:.3f} s{saved}", flush=True)
    return path


def _soft_inverse(logits, geom, opt, keep, fill, device, t2):
    """the trilinear way back of predict_volume: (label [X, Y, Z] view, prob [C, Z, Y, X] or None, the filters' part of the timing line, the
    time the last filter ended).  The blended quantity is the softmax of the logits (--invert_quantity probabilities) or the inferer's values
    as given (logits, or an ensemble's probabilities / votes).  The post-filters run on the file's grid: soft_export writes a uint8 class-index
    map [Z, Y, X], the filters take it as pred=, and label_export with identity tables applies the label codes."""
    Cc = logits.shape[1]
    lut, ident = label_lut(Cc), torch.arange(Cc, dtype=torch.int32)
    tables, axes = geom.lerp_tables("trilinear")
    from_logits, unit = opt["kind"] == "logits", opt["kind"] == "mean_prob"
    softmax = from_logits and opt["quantity"] == "probabilities"
    one_pass = opt["save"] and (softmax or not from_logits)       # what is blended for the labels is what the file holds
    post = keep is not None or fill is not None
    label, prob = ops.soft_export(logits, tables, axes, ident if post else lut, torch.uint8 if post else torch.uint16, softmax=softmax,
                                  probabilities=opt["dtype"] if one_pass else None, unit_range=unit)
    if opt["save"] and not one_pass:                              # labels from blended logits; the file holds the blended softmax
        prob = ops.soft_export(logits, tables, axes, lut, softmax=True, want_labels=False, probabilities=opt["dtype"])[1]
    filtered, tk = "", t2
    if post:
        tk = _sync(device)
        filtered = f"soft export {1e3 * (tk - t2):.2f} ms, "
        cls = label[None]
        if keep is not None:
            tf = tk
            cls, stats = ops.keep_largest_component(pred=cls, num_classes=Cc, stats=True, **keep)
            tk = _sync(device)
            removed = (stats[0, :, 0] - stats[0, :, 1]).tolist()
            filtered += f"keep-largest {1e3 * (tk - tf):.2f} ms (voxels removed per class: {removed}), "
        if fill is not None:
            tf = tk
            cls, filled = ops.fill_holes(pred=cls, num_classes=Cc, stats=True, **fill)
            tk = _sync(device)
            filtered += f"fill-holes {1e3 * (tk - tf):.2f} ms (voxels filled per class: {filled[0].tolist()}), "
        id_tables, id_axes = _identity_tables(tuple(cls.shape[1:]))
        label = ops.label_export(None, id_tables, id_axes, lut, torch.uint16, pred=cls[0])
    return label.permute(2, 1, 0), prob, filtered, tk


def predict(model, datalist, args):
    """predict_volume over the data list into args.result_dir (created); returns the written paths.  `model`: one model or a list of them"""
    os.makedirs(args.result_dir, exist_ok=True)
    for m in (model if isinstance(model, (list, tuple)) else [model]):
        m.eval()
    with torch.no_grad():
        return [predict_volume(model, item, args) for item in datalist]


def build_parser():
    """the reference's command line (predict_whs.py:117-127): the model options plus its own, with its defaults (the model options carry
    --infer_mode / --infer_sigma_scale / --infer_padding_mode, the window blend of predict_volume, and --infer_tta_flips / --ensemble_mode;
    --ensemble_checkpoints names the further members of a model ensemble; --use_averaged_weights loads the averaged weights of a checkpoint
    that data/checkpoint.py::export_state wrote with a weight averager)"""
    parser = add_model_argparse_args(ArgumentParser())
    parser.add_argument("--checkpoint", default="", type=str, help="Checkpoint")
    parser.add_argument("--ensemble_checkpoints", default=[], type=str, nargs="*", help="further checkpoints of the same architecture, ensembled with --checkpoint (--ensemble_mode)")
    parser.add_argument("--use_averaged_weights", action="store_true", help="predict with the checkpoints' averaged weights (EMA / SWA: \"averaged_state_dict\")")
    parser.add_argument("--sample", default="", type=str, help="accepted for compatibility, unused")
    parser.add_argument("--space_x", default=1.0, type=float, help="spacing in x direction")
    parser.add_argument("--space_y", default=1.0, type=float, help="spacing in y direction")
    parser.add_argument("--space_z", default=1.0, type=float, help="spacing in z direction")
    parser.add_argument("--no_gpu", action="store_true", help="refused: prediction runs on the HIP device only")
    parser.add_argument("--data_dir", default="dataset/MM-WHS", type=str, help="dataset directory(ies)")
    parser.add_argument("--json_list", default="CT_test.json", help="Json list(s) of input dataset(s)", type=str)
    parser.add_argument("--result_dir", default="dataset/MM_WHS/MM_WHS_test/CT/", help="Directory for results", type=str)
    parser.add_argument("--keep_largest", action="store_true", help="keep only the largest connected component of each class before the export")
    parser.add_argument("--keep_largest_labels", default=None, type=int, nargs="+", help="classes the filter applies to (default: all foreground)")
    parser.add_argument("--keep_largest_joint", action="store_true", help="one largest component of all applied classes together (MONAI independent=False)")
    parser.add_argument("--keep_largest_connectivity", default=3, type=int, choices=(1, 2, 3), help="6 / 18 / 26 neighbourhood")
    parser.add_argument("--fill_holes", action="store_true", help="fill the enclosed holes of each class before the export (after --keep_largest)")
    parser.add_argument("--fill_holes_labels", default=None, type=int, nargs="+", help="classes whose holes are filled (default: all foreground)")
    parser.add_argument("--fill_holes_connectivity", default=3, type=int, choices=(1, 2, 3), help="6 / 18 / 26 neighbourhood of a hole")
    parser.add_argument("--invert_mode", default="nearest", type=str, choices=INVERT_MODES,
                        help="how the scores go back to the image grid: nearest (argmax first, then a nearest gather) | trilinear (blend the scores, then argmax)")
    parser.add_argument("--invert_quantity", default="probabilities", type=str, choices=INVERT_QUANTITIES,
                        help="what --invert_mode trilinear interpolates: the softmax of the logits (nnU-Net's rule) | the logits; an ensemble's probabilities or votes are blended as given")
    parser.add_argument("--save_probabilities", action="store_true",
                        help="also write <label name>_prob.nii.gz: the class probabilities on the image grid, [X, Y, Z, C] (either invert mode)")
    parser.add_argument("--probability_dtype", default="float32", type=str, choices=tuple(PROBABILITY_DTYPES),
                        help="element type of the probability file; uint8 stores floor(p * 255 + 0.5) with scl_slope 1/255 and is refused for "
                             "--ensemble_mode vote, whose vote counts are not normalised to [0, 1]")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    export_options(args)
    if args.no_gpu or not torch.cuda.is_available():
        raise SystemExit(NO_GPU_MESSAGE)
    if len(args.feature_size) == 1:
        args.feature_size = args.feature_size[0]
    args.device = "cuda:0"
    args.distributed = False
    torch.cuda.set_device(args.device)
    models = []
    for checkpoint in [args.checkpoint] + list(args.ensemble_checkpoints or []):
        model = model_from_argparse_args(args)
        load_model_state(model, checkpoint, averaged=args.use_averaged_weights)
        models.append(model.to(args.device).eval())
    datalist = load_decathlon_datalist_with_modality(os.path.join(args.data_dir, args.json_list), True, "test", base_dir=args.data_dir)
    return predict(models[0] if len(models) == 1 else models, datalist, args)
