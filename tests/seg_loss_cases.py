"""Cases of the loss and Dice metric kernels (csrc/training.hip) for tests/test_hip_seg_loss_forms.py, with the launchers' choices restated
so that tests/test_seg_loss_ref_cpu.py can say, without a GPU, which kernel instantiation every case reaches:

  miseg_seg_loss_fwd / miseg_seg_loss_bwd:  MAXC = 8 for C <= 8, else 16;  VEC = 4 for MAXC = 8 with S % 4 == 0 and 16-byte aligned logits
    (the backward: and dlogits), else 1;  GD = the gdice_focal kind (backward only);  grid (cdiv(S, 1024), B);  one label type of four.
  miseg_dice_metric:  grid (min(cdiv(S, 2048), 2048), B) of 256 threads, a grid-stride loop.

Volumes are flat ([B, C, S] logits, [B, 1, S] labels): the kernels see nothing but S."""
import os
import re
import zlib
from dataclasses import dataclass, replace

import torch

from seg_loss_ref import Cfg, KINDS, W_TYPES

LOSS_VPB = 1024                      # voxels per workgroup of the loss kernels
FWD_FORMS = {(8, 4), (8, 1), (16, 1)}                                      # <L, MAXC, VEC>
BWD_FORMS = {(m, v, gd) for m, v in FWD_FORMS for gd in (False, True)}     # <L, MAXC, VEC, GD>
LABEL_DTYPES = {"F32": torch.float32, "I32": torch.int32, "I64": torch.int64, "U8": torch.uint8}      # MISEG_LABEL_*
UNSUPPORTED = -2                     # MISEG_E_UNSUPPORTED


def cdiv(a, b):
    return -(-a // b)


def fwd_form(C, S, logits_align):
    """(MAXC, VEC) of miseg_seg_loss_fwd; logits_align: the logits address modulo 16"""
    if C > 8:
        return 16, 1
    return 8, 4 if (S % 4 == 0 and logits_align % 16 == 0) else 1


def form(kind, C, S, logits_align=0, dlogits_align=0):
    """(MAXC, VEC, GD) of miseg_seg_loss_bwd"""
    maxc, vec = fwd_form(C, S, logits_align)
    if dlogits_align % 16:
        vec = 1
    return maxc, vec, kind == "gdice_focal"


def nblk(S):
    return cdiv(S, LOSS_VPB)


def metric_grid_x(S):
    return min(cdiv(S, 2048), 2048)


def metric_trips(S):
    """trips of the metric's grid-stride loop made by the first thread"""
    return cdiv(S, metric_grid_x(S) * 256)


def criterion(cfg):
    """the training/losses.py module of a Cfg, built the way LitMonai builds it (to_onehot_y, softmax)"""
    from mi_seg_amd.training.losses import DiceCELoss, DiceFocalLoss, GeneralizedDiceFocalLoss
    kw = dict(include_background=cfg.include_background, to_onehot_y=True, softmax=True, smooth_nr=cfg.smooth_nr, smooth_dr=cfg.smooth_dr)
    if cfg.kind == "dice_focal":
        return DiceFocalLoss(squared_pred=cfg.squared_pred, gamma=cfg.gamma, lambda_dice=cfg.lambda_dice, lambda_focal=cfg.lambda_other, **kw)
    if cfg.kind == "dice_ce":
        return DiceCELoss(squared_pred=cfg.squared_pred, lambda_dice=cfg.lambda_dice, lambda_ce=cfg.lambda_other, **kw)
    return GeneralizedDiceFocalLoss(w_type=cfg.w_type, gamma=cfg.gamma, lambda_gdl=cfg.lambda_dice, lambda_focal=cfg.lambda_other, **kw)


def launcher_forms():
    """(forward forms, backward forms, label types) as the launchers of csrc/training.hip list them, read from the source"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mi-seg_amd", "csrc", "training.hip")
    src = open(path).read()
    val = {"LOSS_MAXC": int(re.search(r"constexpr int LOSS_MAXC = (\d+);", src).group(1)),
           "LOSS_VEC": int(re.search(r"#define MISEG_LOSS_VEC (\d+)", src).group(1)), "true": True, "false": False}

    def body(name):
        at = src.index('extern "C" int %s(' % name)
        return src[at:src.index('\nextern "C"', at + 1)]

    def num(tok):
        tok = tok.strip()
        return val[tok] if tok in val else int(tok)

    fwd = [tuple(num(t) for t in m) for m in re.findall(r"seg_loss_fwd_kernel<L,([^,>]+),([^,>]+)><<<", body("miseg_seg_loss_fwd"))]
    calls = re.findall(r"MISEG_LB\(([^,()]+),([^,()]+),([^,()]+)\)", body("miseg_seg_loss_bwd"))
    bwd = [tuple(num(t) for t in m) for m in calls if m[0].strip() != "MAXC"]      # the macro's own parameter list is no call
    at = src.index("static int dispatch_label(")
    labels = re.findall(r"case MISEG_LABEL_(\w+):", src[at:src.index("\n}", at)])
    return fwd, bwd, labels


# ================================================================================================ the loss cases
@dataclass(frozen=True)
class Case:
    id: str
    cfg: Cfg
    C: int
    S: int
    B: int = 2
    label_dtype: str = "I32"
    labels: str = "absent_one"       # see test_hip_seg_loss_forms.make_labels
    logits: str = "randn3"           # see test_hip_seg_loss_forms.make_logits
    upstream: object = 1.7           # None: the backward runs without a gscale pointer
    misaligned: bool = False         # the logits start 4 bytes into a larger buffer

    def fwd_form(self):
        return fwd_form(self.C, self.S, 4 if self.misaligned else 0)

    def bwd_form(self):
        return form(self.cfg.kind, self.C, self.S, 4 if self.misaligned else 0, 0)


CASES = []
_BASE = {k: Cfg(kind=k, include_background=False, squared_pred=(k == "dice_focal"), smooth_nr=0.0, smooth_dr=1e-6) for k in KINDS}      # as LitMonai builds them


def _add(id_, cfg, C, S, **kw):
    CASES.append(Case(id_, cfg, C, S, **kw))


def _tag(cfg):
    return f"{cfg.kind}{'-' + cfg.w_type if cfg.kind == 'gdice_focal' else ''}-bg{int(cfg.include_background)}-sq{int(cfg.squared_pred)}"


# ---- class counts: where the register arrays are exactly full (8, 16) and where the instantiation changes (8 | 9); S = 500 is the vector
# form for C <= 8, S = 501 below is not
for _C in (2, 3, 8, 9, 16):
    for _bg in (False, True):
        for _kind in ("dice_focal", "dice_ce"):
            for _sq in (False, True):
                _c = replace(_BASE[_kind], include_background=_bg, squared_pred=_sq)
                _add(f"classes-C{_C}-{_tag(_c)}", _c, _C, 500)
        for _w in (W_TYPES if _C in (3, 9) else ("square",)):
            _c = replace(_BASE["gdice_focal"], include_background=_bg, w_type=_w)
            _add(f"classes-C{_C}-{_tag(_c)}", _c, _C, 500)

# ---- spatial edges: one voxel, less than and exactly one vector, LOSS_VPB and one voxel / one vector either side of it, a last workgroup
# of one vector; 65 workgroups (+ one vector | + three voxels): a lane of the finalize kernel adds a second partial
for _C in (3, 9):
    for _S in (1, 3, 4, 1020, 1023, 1024, 1025, 1028, 2048 + 4):
        for _kind in KINDS:
            _add(f"edge-C{_C}-S{_S}-{_kind}", _BASE[_kind], _C, _S)
for _S in (65 * 1024 + 4, 65 * 1024 + 3):
    for _kind in KINDS:
        _add(f"wrap-S{_S}-{_kind}", _BASE[_kind], 3, _S, B=1)

# ---- logits 4 bytes off a 16-byte boundary with S % 4 == 0: the scalar form by the pointer alone
for _C in (3, 8):
    for _kind in KINDS:
        _add(f"misaligned-C{_C}-{_kind}", _BASE[_kind], _C, 500, misaligned=True)

# ---- batch: the finalize kernel's wave-per-job loop (16 waves, B (3 C + 1) jobs) and its other[64]
for _B in (1, 3, 17, 64):
    for _kind in KINDS:
        _add(f"batch-B{_B}-{_kind}", _BASE[_kind], 4, 36, B=_B)

# ---- hyper-parameters
for _kind in ("dice_focal", "gdice_focal"):
    for _g in (0.0, 0.5, 2.0, 3.5):
        _add(f"gamma-{_g}-{_kind}", replace(_BASE[_kind], gamma=_g), 3, 500)
for _kind in KINDS:
    for _nr, _dr in ((1e-5, 1e-5), (1.0, 1.0)):      # MONAI's defaults; a smoothing that matters
        _add(f"smooth-{_nr}-{_dr}-{_kind}", replace(_BASE[_kind], smooth_nr=_nr, smooth_dr=_dr), 3, 500)
    for _ld, _lo in ((0.0, 1.0), (1.0, 0.0), (0.3, 2.5)):
        _add(f"lambda-{_ld}-{_lo}-{_kind}", replace(_BASE[_kind], lambda_dice=_ld, lambda_other=_lo), 3, 500)
    for _up in (1.0, -2.5, 0.0, None):
        _add(f"upstream-{_up}-{_kind}", _BASE[_kind], 3, 500, upstream=_up)

# ---- label content
for _kind in KINDS:
    for _bg in (False, True):
        for _lab in ("absent_one", "absent_all", "background_only", "single_class"):
            _add(f"labels-{_lab}-bg{int(_bg)}-{_kind}", replace(_BASE[_kind], include_background=_bg), 3, 500, labels=_lab)
# every label type through every forward and backward form
for _dt in LABEL_DTYPES:
    for _C, _S in ((3, 500), (3, 501), (9, 500)):
        for _kind in KINDS:
            _add(f"dtype-{_dt}-C{_C}-S{_S}-{_kind}", _BASE[_kind], _C, _S, label_dtype=_dt)

# ---- logit range (fp32 inputs that the float64 judge sees exactly)
for _kind in KINDS:
    for _C in (3, 9):
        for _lg in ("equal", "times30", "times100", "focal_corner", "voxel_1e4"):
            _add(f"logits-{_lg}-C{_C}-{_kind}", replace(_BASE[_kind], include_background=True), _C, 500, logits=_lg)

assert len({c.id for c in CASES}) == len(CASES)


# ---- inputs, the judge's answers and the bounds
LOSS_BAR, GRAD_BAR = 1e-5, 1e-4      # the project's bars: relative on the loss (and the sums), pooled and per element on d(loss)/d(logits)
# ids of the cases whose bounds are max(bar, 2 x the error of the float32 torch composition against the float64 judge) instead of the bar
# (parity.py, local_tol; the pooled dlogits check keeps its bar).  Empty: tests/test_seg_loss_ref_cpu.py shows that no case needs it, and a
# case that comes to need it fails there until it is named here
WIDENED = frozenset()


def make_labels(case):
    """int64 [B, 1, S] on the CPU.  absent_one: the last class is missing from the last sample; absent_all: from every sample;
    background_only: sample 0 holds class 0 alone; single_class: sample 0 holds class 1 alone"""
    g = torch.Generator().manual_seed(zlib.crc32(case.id.encode()) ^ 0x5EED)
    lab = torch.randint(0, case.C, (case.B, 1, case.S), generator=g)
    if case.labels == "absent_one":
        lab[-1][lab[-1] == case.C - 1] = 0
    elif case.labels == "absent_all":
        lab[lab == case.C - 1] = 0
    elif case.labels == "background_only":
        lab[0] = 0
    elif case.labels == "single_class":
        lab[0] = 1
    else:
        raise KeyError(case.labels)
    return lab


def make_logits(case, lab):
    """fp32 [B, C, S] on the CPU: the float64 judge reads exactly these numbers"""
    g = torch.Generator().manual_seed(zlib.crc32(case.id.encode()))
    x = torch.randn(case.B, case.C, case.S, generator=g)
    if case.logits == "equal":
        return torch.full_like(x, 0.75)
    if case.logits in ("times30", "times100"):
        return x * (30.0 if case.logits == "times30" else 100.0)
    x = 3.0 * x
    if case.logits == "focal_corner":      # the focal term's large-loss corner: -80 under the label, +80 under a wrong class
        n = min(40, case.S)
        for b in range(case.B):
            c = lab[b, 0, :n]
            x[b, :, :n].scatter_(0, c[None], torch.full((1, n), -80.0))
            x[b, :, :n].scatter_(0, ((c + 1) % case.C)[None], torch.full((1, n), 80.0))
    elif case.logits == "voxel_1e4":
        x[0, :, min(7, case.S - 1)] = torch.tensor([1e4 if c % 2 == 0 else -1e4 for c in range(case.C)])
    elif case.logits != "randn3":
        raise KeyError(case.logits)
    return x


def composition_errors(x, lab, cfg, upstream):
    """errors of the float32 torch composition (the judge's formulas on the fp32 logits themselves) against the float64 judge:
    dict of loss, other (relative), sums, grad_local (parity.local_err; sums: the larger of pooled and local)"""
    from conftest import rel_err
    from parity import local_err
    import seg_loss_ref as R
    up = 1.0 if upstream is None else upstream
    loss64, grad64 = R.loss_and_grad(x.double(), lab, cfg, up)
    loss32, grad32 = R.loss_and_grad(x, lab, cfg, up)
    sums64, other64 = R.kernel_sums(x.double(), lab, cfg)
    sums32, other32 = R.kernel_sums(x, lab, cfg)
    rel = lambda a, b: abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)
    return dict(loss=rel(loss32, loss64), other=rel(other32, other64), sums=max(rel_err(sums32, sums64), local_err(sums32, sums64)[0]),
                grad_local=local_err(grad32, grad64)[0])


def judged(case_id, x, lab, cfg, upstream):
    """the judge's answers for fp32 logits x and int64 labels, with the bounds: the bars, or the rule above for a case named in WIDENED"""
    import seg_loss_ref as R
    up = 1.0 if upstream is None else upstream
    loss, grad = R.loss_and_grad(x.double(), lab, cfg, up)
    sums, other = R.kernel_sums(x.double(), lab, cfg)
    e = composition_errors(x, lab, cfg, upstream) if case_id in WIDENED else dict(loss=0.0, other=0.0, sums=0.0, grad_local=0.0)
    return dict(loss=loss, grad=grad, sums=sums, other=other, loss_bound=max(LOSS_BAR, 2 * e["loss"]), other_bound=max(LOSS_BAR, 2 * e["other"]),
                sums_bound=max(LOSS_BAR, 2 * e["sums"]), grad_pooled_bound=GRAD_BAR, grad_local_bound=max(GRAD_BAR, 2 * e["grad_local"]))


# ================================================================================================ the metric cases
@dataclass(frozen=True)
class MetricCase:
    id: str
    C: int
    B: int
    S: int
    label_dtype: str = "I32"
    labels: str = "random"           # "random" | "out_of_range" | "never" (one class never labelled, one never predicted)
    logits: str = "ties"             # "ties": small integers, many exact ties | "randn" | "first_last" (first and last channel tie at the maximum)


METRIC_CASES = []
_dts = list(LABEL_DTYPES)
for _i, _C in enumerate((1, 2, 9, 33, 64)):
    for _B in (1, 3):
        for _j, _S in enumerate((1, 255, 256, 257, 2049)):
            METRIC_CASES.append(MetricCase(f"grid-C{_C}-B{_B}-S{_S}", _C, _B, _S, label_dtype=_dts[(_i + _j) % 4]))
METRIC_CASES.append(MetricCase("capped-grid", 2, 1, 2048 * 2048 + 5, label_dtype="U8", logits="randn"))
for _C in (2, 9, 64):
    METRIC_CASES.append(MetricCase(f"tie-first-last-C{_C}", _C, 2, 700, logits="first_last"))
    METRIC_CASES.append(MetricCase(f"never-C{_C}", _C, 2, 700, labels="never", logits="randn"))
for _dt in ("U8", "I64", "I32", "F32"):
    METRIC_CASES.append(MetricCase(f"out-of-range-{_dt}", 9, 2, 700, label_dtype=_dt, labels="out_of_range"))
