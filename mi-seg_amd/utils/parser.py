"""Command-line surface of MI-Seg (reference utils/parser.py:5-150): same flags, types and defaults, expressed as tables
(plus --infer_mode / --infer_sigma_scale / --infer_padding_mode, whose defaults are what the reference gets from MONAI, and the
rotation / zoom / gamma / noise flags of the device augmenter, all off by default)."""
from argparse import ArgumentParser

_T = "store_true"


def _positive_int(text):
    """argparse type of a count that must be >= 1"""
    v = int(text)
    if v < 1:
        raise ValueError("{} is not >= 1".format(text))          # (argparse turns a type's ValueError into its usage error)
    return v

MODEL_ARGS = {
    "monai.net": [
        ("--pretrained", dict(type=str, help="path to pre-trained model checkpoint")),
        ("--ckpt_path", dict(type=str, help="path to a training checkpoint to resume")),
        ("--model_name", dict(default="unetr", type=str, help="unet | unet_vanilla | unetr | swin_unetr | pre_swin_unetr")),
        ("--in_channels", dict(default=1, type=int)), ("--out_channels", dict(default=14, type=int)),
        ("--roi_x", dict(default=96, type=int)), ("--roi_y", dict(default=96, type=int)), ("--roi_z", dict(default=96, type=int)),
        ("--feature_size", dict(default=[16], type=int, nargs="+")),
        ("--hidden_size", dict(default=768, type=int)), ("--mlp_dim", dict(default=3072, type=int)),
        ("--num_heads", dict(default=12, type=int)), ("--pos_embed", dict(default="perceptron", type=str)),
        ("--no_conv_block", dict(action=_T)), ("--no_res_block", dict(action=_T)),
        ("--dropout_rate", dict(default=0.0, type=float)), ("--spatial_dims", dict(default=3, type=int)),
        ("--qkv_bias", dict(action=_T)),
        ("--vit_norm_name", dict(type=str, default="layer")), ("--vit_norm_no_affine", dict(action=_T)),
        ("--encoder_norm_name", dict(type=str, default="instance")), ("--encoder_norm_no_affine", dict(action=_T)),
        ("--decoder_norm_name", dict(type=str, default="instance")), ("--decoder_norm_no_affine", dict(action=_T)),
        ("--num_groups", dict(type=int, default=4)), ("--num_styles", dict(type=int, default=2)),
        ("--dropout_path_rate", dict(default=0.0, type=float)), ("--attn_drop_rate", dict(default=0.0, type=float)),
        ("--depth_swin_block", dict(default=[2], type=int, nargs="+")), ("--use_checkpoint", dict(action=_T)),
        ("--downsample", dict(default="merging", type=str)), ("--no_normalize_swin", dict(action=_T)),
        ("--pre_swin", dict(type=str, default="")),
        ("--num_layers", dict(type=int, default=4)), ("--strides", dict(default=[2, 2, 2], nargs="+", type=int)),
        ("--kernel_size", dict(default=3, nargs="+", type=int)), ("--up_kernel_size", dict(default=3, nargs="+", type=int)),
        ("--num_res_units", dict(default=2, type=int)), ("--activation", dict(default="prelu", type=str)),
        ("--no_bias", dict(action=_T)), ("--adn_ordering", dict(default="NDA", type=str)), ("--freeze_encoder", dict(action=_T)),
    ],
    "loss": [
        ("--criterion", dict(default="dice_focal", type=str)), ("--squared_dice", dict(action=_T)),
        ("--smooth_nr", dict(default=0.0, type=float)), ("--smooth_dr", dict(default=1e-6, type=float)),
        ("--no_include_background", dict(action=_T)),
    ],
    "optimizer": [
        ("--lr", dict(default=1e-4, type=float)), ("--optim_name", dict(default="adamw", type=str)),
        ("--reg_weight", dict(default=1e-5, type=float)), ("--momentum", dict(default=0.99, type=float)),
        ("--scheduler", dict(default="reduce_on_plateau", type=str)), ("--warmup_epochs", dict(default=50, type=int)),
        ("--patience_scheduler", dict(default=3, type=int)), ("--t_max", dict(default=200, type=int)),
        ("--cycles", dict(default=0.5, type=float)),
    ],
    "inference": [
        ("--infer_overlap", dict(default=0.5, type=float)), ("--sw_batch_size", dict(default=1, type=int)), ("--infer_cpu", dict(action=_T)),
        # not flags of the reference (it always blends with MONAI's defaults, which these are): MONAI's other blending arguments
        ("--infer_mode", dict(default="constant", type=str, help="constant | gaussian: how overlapping windows are blended")),
        ("--infer_sigma_scale", dict(default=0.125, type=float, nargs="+", help="gaussian mode: sigma = roi * this (one value, or one per axis)")),
        ("--infer_padding_mode", dict(default="constant", type=str, help="constant | reflect | replicate | circular: pad of an image smaller than the roi")),
        # flip test-time augmentation / ensembling (training/ensemble.py): none by default, which leaves the inference as it is
        ("--infer_tta_flips", dict(default=None, type=int, nargs="*", choices=(0, 1, 2), help="spatial axes of the mirror TTA: every flip over them is predicted and averaged")),
        ("--ensemble_mode", dict(default="mean_logits", type=str, choices=("mean_logits", "mean_prob", "vote"), help="what the members of an ensemble / the TTA flips contribute")),
    ],
    "early_stop": [("--patience", dict(default=6, type=int)), ("--min_delta", dict(default=0.001, type=float))],
    "checkpointing": [("--save_top_k", dict(default=3, type=int))],
    "wandb_logger": [
        ("--experiment_name", dict(type=str)), ("--group", dict(type=str)), ("--project", dict(type=str)), ("--entity", dict(type=str)),
        ("--wandb_mode", dict(type=str, default="online")), ("--source", dict(type=int)), ("--alpha_reversal", dict(type=float, default=1.0)),
    ],
}

DATA_ARGS = {
    "dataset(s)": [
        ("--data_dirs", dict(default=["dataset/MM-WHS", "dataset/MM-WHS"], type=str, nargs="+")),
        ("--json_lists", dict(default=["CT_fold1.json", "MR.json"], nargs="+", type=str)),
        ("--space_x", dict(default=1.0, type=float)), ("--space_y", dict(default=1.0, type=float)), ("--space_z", dict(default=1.0, type=float)),
        ("--patches_training_sample", dict(default=1, type=int)),
        ("--randFlipd_prob", dict(default=0.2, type=float)), ("--randRotate90d_prob", dict(default=0.2, type=float)),
        ("--randScaleIntensityd_prob", dict(default=0.1, type=float)), ("--randShiftIntensityd_prob", dict(default=0.1, type=float)),
        # not flags of the reference: free rotation / zoom, gamma contrast and Gaussian noise on the device augmenter (data/augment.py), all off
        ("--randAffined_prob", dict(default=0.0, type=float)),
        ("--rotate_range", dict(default=[0.0, 0.0, 0.0], type=float, nargs="+", help="radians per axis (one value, or one per axis): drawn U(-r, r)")),
        ("--scale_range", dict(default=[0.0, 0.0, 0.0], type=float, nargs="+", help="zoom factor 1 + U(-s, s) per axis")),
        ("--translate_range", dict(default=[0.0, 0.0, 0.0], type=float, nargs="+", help="voxels per axis: drawn U(-t, t)")),
        ("--affine_padding_mode", dict(default="border", type=str, choices=("border", "zeros"), help="what a resampled patch reads outside the volume")),
        ("--randAdjustContrastd_prob", dict(default=0.0, type=float)),
        ("--gamma_range", dict(default=[0.5, 4.5], type=float, nargs=2, help="gamma of RandAdjustContrastd: drawn U(low, high)")),
        ("--randGaussianNoised_prob", dict(default=0.0, type=float)),
        ("--noise_std", dict(default=0.1, type=float, help="RandGaussianNoised: the std of a sample is drawn U(0, noise_std)")),
        ("--randGaussianSmoothd_prob", dict(default=0.0, type=float)),
        ("--smooth_sigma_range", dict(default=[0.25, 1.5], type=float, nargs=2, help="RandGaussianSmoothd: sigma per axis drawn U(low, high), voxels")),
        ("--randGaussianSharpend_prob", dict(default=0.0, type=float)),
        ("--sharpen_sigma1_range", dict(default=[0.5, 1.0], type=float, nargs=2, help="RandGaussianSharpend: the first sigma per axis, U(low, high)")),
        ("--sharpen_sigma2", dict(default=0.5, type=float, help="RandGaussianSharpend: the second sigma of an axis is drawn between this and the first")),
        ("--sharpen_alpha_range", dict(default=[10.0, 30.0], type=float, nargs=2, help="RandGaussianSharpend: alpha drawn U(low, high)")),
        ("--use_normal_dataset", dict(action=_T)), ("--cache_num", dict(default=24, type=int)), ("--loader_workers", dict(default=8, type=int)),
        ("--batch_size", dict(default=1, type=int)), ("--num_workers", dict(default=8, type=int)),
    ],
}

TUNE_ARGS = {
    "tune": [
        ("--study_name", dict(default="experiment", type=str)), ("--n_trials", dict(type=int)), ("--timeout", dict(type=int)),
        ("--max_epochs", dict(default=2, type=int)), ("--check_val_every_n_epoch", dict(default=1, type=int)),
        ("--no_gpu", dict(action=_T)), ("--no_amp", dict(action=_T)), ("--iters_to_accumulate", dict(default=1, type=int)),
        ("--default_root_dir", dict(default="./experiments", type=str)), ("--port", dict(default="23456", type=str)),
        ("--storage_name", dict(default="MI-Seg", type=str)), ("--min_lr", dict(default=1e-5, type=float)), ("--max_lr", dict(default=5e-3, type=float)),
    ],
}

# The reference's train.py takes every pytorch_lightning.Trainer argument (Trainer.add_argparse_args); these are the ones the fused optimiser
# (training/optim.py::ArenaOptimizer) carries out on the device.  A table of its own that no other add_* function adds: a script that also adds
# Lightning's own Trainer arguments would otherwise define them twice.  --skip_nonfinite_steps is the only flag Lightning does not have.
TRAINER_ARGS = {
    "trainer": [
        ("--gradient_clip_val", dict(default=None, type=float, help="clip gradients to this global norm / absolute value (default: no clipping)")),
        ("--gradient_clip_algorithm", dict(default="norm", type=str, choices=("norm", "value"))),
        ("--track_grad_norm", dict(default=-1, type=int, choices=(-1, 2), help="2: compute the gradients' L2 norm every step for logging; -1: off")),
        ("--skip_nonfinite_steps", dict(action=_T, help="an optimisation step whose gradient norm is inf or NaN changes nothing")),
        ("--accumulate_grad_batches", dict(default=1, type=_positive_int, help="micro-batches per optimisation step: the step runs on their mean gradient")),
        # an average of the weights over the optimisation steps, kept on the device (training/optim.py::WeightAverager): Lightning's
        # StochasticWeightAveraging ("swa") and the EMA of the weights that nnU-Net-style and MONAI bundles evaluate and ship; off by default
        ("--weight_averaging", dict(default="none", type=str, choices=("none", "ema", "swa"), help="keep an average of the weights: ema | swa (default: none)")),
        ("--ema_decay", dict(default=0.999, type=float, help="ema: avg += (1 - decay) (w - avg) per averaged step; in [0, 1)")),
        ("--ema_warmup", dict(action=_T, help="ema: the n-th update uses min(decay, (1 + n) / (10 + n))")),
        ("--weight_averaging_start", dict(default=0, type=int, help="the first optimisation step (counted from 0) that is averaged")),
        ("--weight_averaging_every", dict(default=1, type=_positive_int, help="average every this many optimisation steps")),
        ("--no_validate_averaged", dict(action=_T, help="validate on the training weights although an average is kept")),
    ],
}


def accumulation_steps(args):
    """micro-batches per optimisation step (training/optim.py::GradAccumulator): Lightning's --accumulate_grad_batches, else the reference's
    own --iters_to_accumulate (utils/trainer.py:33-78).  `args`: a namespace or a dict; a missing (or None) flag counts as 1.  ValueError for
    a count below 1 and for two counts above 1 that differ."""
    get = args.get if isinstance(args, dict) else (lambda k, d=None: getattr(args, k, d))
    vals = {}
    for k in ("accumulate_grad_batches", "iters_to_accumulate"):
        v = get(k, None)
        v = 1 if v is None else v
        if isinstance(v, bool) or int(v) != v or int(v) < 1:
            raise ValueError("{} {!r} must be an integer >= 1".format(k, v))
        vals[k] = int(v)
    a, b = vals["accumulate_grad_batches"], vals["iters_to_accumulate"]
    if a > 1 and b > 1 and a != b:
        raise ValueError("--accumulate_grad_batches {} and --iters_to_accumulate {} disagree: give one of them".format(a, b))
    return a if a > 1 else b


def _add(parser: ArgumentParser, table):
    for group_name, entries in table.items():
        grp = parser.add_argument_group(group_name)
        for flag, kw in entries:
            grp.add_argument(flag, **kw)
    return parser


def add_model_argparse_args(parser: ArgumentParser):
    return _add(parser, MODEL_ARGS)


def add_data_argparse_args(parser: ArgumentParser):
    return _add(parser, DATA_ARGS)


def add_tune_argparse_args(parser: ArgumentParser):
    return _add(parser, TUNE_ARGS)


def add_trainer_argparse_args(parser: ArgumentParser):
    return _add(parser, TRAINER_ARGS)
