"""Float64 references, input cases and launch helpers of the attention kernels (csrc/attention.hip, csrc/attention_global.hip), shared by
tests/test_hip_kernels.py, tests/test_hip_winattn_forms.py (GPU) and tests/test_winattn_ref_cpu.py, which pins the references on the CPU
against an independent restatement and shows that the inputs drawn here leave honest bf16 arithmetic below half of every bar of the GPU tests.

* ref_window_attention: pad with the bias row, roll, partition, softmax(q scale k^T + bias + mask) v, reverse, roll back, crop - in the dtype
  of its arguments (the tests hand it float64); with_lse also returns the log-sum-exp [windows, heads, n] in the kernels' window order
  (b, wz, wy, wx), natural-log units, rows of padded queries included.
* ref_global_attention: softmax(q k^T scale) [o mask] v over the whole token grid and its log-sum-exp [B, heads, n].
* mfma_model: the rounding points of the bf16 matrix-core forward - Q' = bf16(q scale log2e), fp32 score sums, P rounded to bf16 in front of
  PV, the output rounded once - as the yardstick of that kernel's `out` and `lse`.
* Spec / Case: one geometry and the tensors drawn for it from seeded CPU generators (the CPU and the GPU test see the same numbers).
* fwd_params / bwd_params / new_output: the C structs for caller-supplied views and prefilled outputs."""
import collections
import math

import torch

from parity import local_err

TOL = {torch.float32: 2e-4, torch.bfloat16: 2e-2}
LOG2E = 1.4426950408889634


# ----------------------------------------------------------------------------------------------------------------- references
def _pad_roll(qkv, qkv_bias, ws, ss):
    """(the padded and rolled grid, the shift mask [nW, n, n] or None)"""
    from oracle.functional import compute_mask
    B, D, H, W, C3 = qkv.shape
    pd, ph, pw = (-D) % ws[0], (-H) % ws[1], (-W) % ws[2]
    x = qkv
    if pd or ph or pw:
        if qkv_bias is not None:
            full = qkv_bias.view(1, 1, 1, 1, C3).expand(B, D + pd, H + ph, W + pw, C3).clone()
        else:
            full = qkv.new_zeros(B, D + pd, H + ph, W + pw, C3)
        full[:, :D, :H, :W] = qkv
        x = full
    mask = None
    if any(ss):
        x = torch.roll(x, shifts=tuple(-s for s in ss), dims=(1, 2, 3))
        mask = compute_mask(tuple(x.shape[1:4]), ws, ss).to(qkv.device)
    return x, mask


def _scores(q, k, table, mask, tw, scale):
    """q scale k^T + bias + mask of [b, heads, n, hd] operands, [b, heads, n, n]"""
    from oracle.functional import relative_position_index
    b, heads, n, _ = q.shape
    attn = (q * scale) @ k.transpose(-2, -1)
    if table is not None:
        idx = relative_position_index((tw, tw, tw)).to(q.device)[:n, :n].reshape(-1)
        attn = attn + table[idx].reshape(n, n, -1).permute(2, 0, 1).unsqueeze(0)
    if mask is not None:
        nw = mask.shape[0]
        mask = mask.to(attn.dtype)
        attn = (attn.view(b // nw, nw, heads, n, n) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, n, n)
    return attn


def _unwindow(o, ws, ss, dims, padded):
    """[b, heads, n, hd] per-window outputs -> [B, D, H, W, C] (reverse, roll back, crop)"""
    from oracle.functional import window_reverse
    B, D, H, W = dims
    b, heads, n, hd = o.shape
    o = o.transpose(1, 2).reshape(b, n, heads * hd)
    o = window_reverse(o.view(-1, *ws, heads * hd), ws, (B, *padded))
    if any(ss):
        o = torch.roll(o, shifts=tuple(ss), dims=(1, 2, 3))
    return o[:, :D, :H, :W].contiguous()


def ref_window_attention(qkv, qkv_bias, table, heads, ws, ss, tw, scale, drop_mask=None, with_lse=False):
    """plain PyTorch reference (in the dtype of its arguments: the tests hand it float64) of the fused attention core (pad with the bias row,
    roll, partition, softmax(QK^T+bias+mask)V, reverse, roll back, crop) built from the oracle's helpers.  qkv_bias None: padded tokens are
    zeros; table None: no bias.  drop_mask: [windows, heads, n, n] of 0 or 1 / (1 - p) (attn_drop, window_attention.py:114).
    with_lse: also the log-sum-exp of the scores, [windows, heads, n], natural-log units, padded query rows included."""
    from oracle.functional import window_partition
    B, D, H, W, C3 = qkv.shape
    hd = C3 // 3 // heads
    x, mask = _pad_roll(qkv, qkv_bias, ws, ss)
    win = window_partition(x, ws)
    b, n, _ = win.shape
    q, k, v = win.reshape(b, n, 3, heads, hd).permute(2, 0, 3, 1, 4)
    attn = _scores(q, k, table, mask, tw, scale)
    prob = attn.softmax(-1)
    if drop_mask is not None:
        prob = (prob * drop_mask).to(v.dtype)
    o = _unwindow(prob @ v, ws, ss, (B, D, H, W), tuple(x.shape[1:4]))
    return (o, torch.logsumexp(attn, -1)) if with_lse else o


def ref_global_attention(qkv, heads, scale, drop_mask=None):
    """softmax((q k^T) scale) [o drop_mask] v over the whole token grid (MONAI SABlock on "b h (qkv l d)" channels) and the log-sum-exp of
    the scaled scores [B, heads, n]; qkv [B, D, H, W, 3C]."""
    B, C = qkv.shape[0], qkv.shape[-1] // 3
    n, hd = math.prod(qkv.shape[1:4]), C // heads
    q, k, v = qkv.reshape(B, n, 3, heads, hd).permute(2, 0, 3, 1, 4)
    attn = (q @ k.transpose(-2, -1)) * scale
    prob = attn.softmax(-1)
    if drop_mask is not None:
        prob = prob * drop_mask
    return (prob @ v).transpose(1, 2).reshape(*qkv.shape[:4], C), torch.logsumexp(attn, -1)


def _bf(t):
    return t.to(torch.bfloat16).float()


def mfma_model(qkv, qkv_bias, table, heads, ws, ss, tw, scale, drop_mask=None):
    """(out as bf16, lse as fp32) of a model of the bf16 matrix-core forward's rounding points on bf16 qkv and fp32 bias row / table:
    Q' = bf16(q scale log2e) and K, V = bf16 (the bias row of a padded token rounded like a loaded one), scores summed in fp32 in the log2
    domain with the fp32 table and mask added, p = exp2(s - max) in fp32, the denominator from the unrounded p, P rounded to bf16 in front
    of PV (after the dropout factor), fp32 PV sums, one rounding of the quotient.  Not the kernel's tile order (its running maximum rescales
    per key tile): the places where precision is lost."""
    from oracle.functional import window_partition
    assert qkv.dtype == torch.bfloat16
    B, D, H, W, C3 = qkv.shape
    hd = C3 // 3 // heads
    x, mask = _pad_roll(qkv.float(), None if qkv_bias is None else qkv_bias.float(), ws, ss)
    win = window_partition(x, ws)
    b, n, _ = win.shape
    q, k, v = win.reshape(b, n, 3, heads, hd).permute(2, 0, 3, 1, 4)
    qs = _bf(q * (scale * LOG2E))
    s = _scores(qs, _bf(k), None if table is None else table.float() * LOG2E, None if mask is None else mask * LOG2E, tw, 1.0)
    m = s.max(-1, keepdim=True).values
    p = torch.exp2(s - m)
    l = p.sum(-1, keepdim=True)
    if drop_mask is not None:
        p = p * drop_mask.float()
    o = (_bf(p) @ _bf(v)) / l
    out = _unwindow(o, ws, ss, (B, D, H, W), tuple(x.shape[1:4])).to(torch.bfloat16)
    return out, ((m + torch.log2(l)) * math.log(2.0)).squeeze(-1)


def lse_yardstick(kind, qkv, qkv_bias, table, heads, ws, ss, tw, scale, lse_ref):
    """max |lse - float64 lse| of the arithmetic a kernel family is measured by (the GPU test allows a kernel twice this):
    "fp32"  torch's fp32 logsumexp of fp32 scores (the fp32 kernels; for bf16 qkv the same on the bf16-rounded inputs: fp32 sums, what the
            bf16 query-lane kernels compute);
    "mfma"  mfma_model's (the bf16 matrix-core kernels, window and global)."""
    f = lambda t: None if t is None else t.float()
    if kind == "mfma":
        got = mfma_model(qkv, qkv_bias, table, heads, ws, ss, tw, scale)[1]
    else:
        got = ref_window_attention(qkv.float(), f(qkv_bias), f(table), heads, ws, ss, tw, scale, with_lse=True)[1]
    return float((got.double() - lse_ref.double()).abs().max())


def dqkv_local_tol(tol, qkv, qb, table, g, heads, ws, ss, scale, want, drop_mask=None, tw=7):
    """bound of the local metric for the bf16 data gradient of the attention core: max(tol, 2 x yardstick), the yardstick being the local error of
    the SAME composition run by torch in bf16 (bias row and table rounded to bf16 too) against the float64 gradient `want`.  A window that is
    mostly padding holds hundreds of identical tokens (the bias row): their rounding errors add coherently instead of averaging out, so single
    elements of dk stand 15 times above the pooled error - in torch's bf16 arithmetic as in the kernel's.  fp32: tol.
    Measured, B = 2, [dims, heads, C]: yardstick 6.5e-2 / 5.8e-2 / 4.3e-2 / 3.8e-2 / 5.5e-2 for the five shapes of test_window_attention_core (kernel
    2.8e-2 / 4.06e-2 / 2.0e-2 / 1.5e-2 / 9.6e-3 against tol 4e-2); with dropout 6.1e-2 / 4.1e-2 / 5.6e-2 (kernel 2.8e-2 / 2.1e-2 / 2.2e-2)."""
    if qkv.dtype != torch.bfloat16:
        return tol
    qy = qkv.clone().requires_grad_(True)
    c = lambda t: None if t is None else t.to(qkv.dtype)
    ref_window_attention(qy, c(qb), c(table), heads, ws, ss, tw, scale, drop_mask=drop_mask).backward(g)
    return max(tol, 2 * local_err(qy.grad, want)[0])


# ----------------------------------------------------------------------------------------------------------------- cases
class Spec(collections.namedtuple("Spec", "dims ws ss heads C B tw table_amp qk_gain bias table")):
    """one geometry: grid dims, window, shift, heads, channels, batch, the table's window `tw`; the amplitude the table is drawn at, a gain on
    the q and k thirds of qkv (sharp softmax), whether there is a qkv bias row and a bias table"""
    __slots__ = ()

    def __new__(cls, dims, ws, ss, heads, C, B=2, tw=7, table_amp=0.5, qk_gain=1.0, bias=True, table=True):
        return super().__new__(cls, tuple(dims), tuple(ws), tuple(ss), heads, C, B, tw if table else 1, table_amp, qk_gain, bias, table)

    @property
    def n(self):
        return math.prod(self.ws)

    @property
    def windows(self):
        return self.B * math.prod(-(-d // w) for d, w in zip(self.dims, self.ws))

    @property
    def hd(self):
        return self.C // self.heads

    @property
    def scale(self):
        return self.hd ** -0.5

    @property
    def padded(self):
        return any((-d) % w for d, w in zip(self.dims, self.ws))

    def __str__(self):
        x = lambda t: "x".join(map(str, t))
        s = f"B{self.B}-{x(self.dims)}-w{x(self.ws)}-s{x(self.ss)}-h{self.heads}c{self.C}"
        s += "" if self.tw in (1, 7) else f"-tw{self.tw}"
        s += "" if self.table_amp == 0.5 else f"-amp{self.table_amp:g}"
        s += "" if self.qk_gain == 1.0 else f"-qk{self.qk_gain:g}"
        return s + ("" if self.bias else "-nobias") + ("" if self.table else "-notable")


def _draw(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


# amplitude of the q and k thirds of qkv.  bf16: the matrix-core forward rounds Q' = q scale log2e to bf16, a score error that grows with
# |q| |k|; over the 1e5 outputs of the larger cases the worst element of the rounding model (mfma_model) then stands at 1.85e-2 of the
# per-element metric for standard-normal q and k - an honest kernel would be left no room under the 2e-2 bar.  At 0.5 the model stays below
# half the bar on every case (tests/test_winattn_ref_cpu.py; 9.4e-3 worst, of which ~9e-3 are the roundings of P and of the output, which no
# amplitude moves).  The bias row and the table keep the softmax far from flat.  fp32 has no such rounding: the usual amplitude.
QK_AMP = {torch.float32: 1.0, torch.bfloat16: 0.5}


class Case:
    """the tensors of a Spec, drawn on the CPU as test_hip_kernels.rnd draws (seeded generator, standard normal), then moved: qkv and dout
    in `dtype` (q and k thirds times QK_AMP[dtype] qk_gain), the bias row (x 0.3) and the table (x table_amp) in fp32 or None."""

    def __init__(self, spec, dtype, device="cpu", seed=181):
        s = self.spec = spec
        self.dtype, self.device = dtype, device
        qkv = _draw((s.B, *s.dims, 3 * s.C), seed)
        qkv[..., :2 * s.C] *= QK_AMP[dtype] * s.qk_gain
        self.qkv = qkv.to(device).to(dtype)
        self.qb = (_draw((3 * s.C,), seed + 1) * 0.3).to(device) if s.bias else None
        self.table = _draw(((2 * s.tw - 1) ** 3, s.heads), seed + 2, s.table_amp).to(device) if s.table else None
        self.dout = _draw((s.B, *s.dims, s.C), seed + 3).to(device).to(dtype)

    def reference(self, drop_mask=None, backward=True):
        """float64 on the case's device: dict(out, lse, dqkv, dtable, dqb) - the last two None where the case has no table / bias row"""
        s = self.spec
        d = lambda t: None if t is None else t.double().clone().requires_grad_(backward)
        q, qb, tab = d(self.qkv), d(self.qb), d(self.table)
        if s.table is False and s.ws == s.dims and not any(s.ss):
            out, lse = ref_global_attention(q, s.heads, s.scale, drop_mask=drop_mask)
        else:
            out, lse = ref_window_attention(q, qb, tab, s.heads, s.ws, s.ss, s.tw, s.scale, drop_mask=drop_mask, with_lse=True)
        r = {"out": out.detach(), "lse": lse.detach(), "dqkv": None, "dtable": None, "dqb": None}
        if backward:
            out.backward(self.dout.double())
            g = lambda t: None if t is None else (t.grad if t.grad is not None else torch.zeros_like(t))
            r.update(dqkv=q.grad, dtable=g(tab), dqb=g(qb))
        return r


# ----------------------------------------------------------------------------------------------------------------- launches
def new_output(shape, dtype, layout="contig"):
    """an output operand that shows what the kernel left alone: NaN-filled when contiguous (a row the kernel skipped stays NaN), a view in a
    sentinel-filled buffer (layouts.place_out) otherwise - there layouts.assert_untouched looks for stores outside the view"""
    from layouts import Slot, place_out
    return Slot(tuple(shape), dtype, "contig", float("nan")) if layout == "contig" else place_out(shape, dtype, layout)


def fwd_params(ops, spec, qkv, out, qb, table, lse, drop=None):
    """miseg_winattn_params for caller-supplied views (qkv, out: uniformly strided channels-last rows)"""
    return ops.winattn_params(qkv, out, qb, table, lse, spec.heads, spec.ws, spec.ss, spec.tw, spec.scale, drop)


def bwd_params(ops, L, spec, qkv, out, qb, table, lse, dout, dqkv, dqb, dtable, drop=None):
    f = fwd_params(ops, spec, qkv, out, qb, table, lse, drop)
    return L.WinattnBwd(f, ops._ptr(dout), ops.rows(dout)[0], ops._ptr(dqkv), ops.rows(dqkv)[0], ops._ptr(dqb), ops._ptr(dtable))


# ----------------------------------------------------------------------------------------------------------------- the cases of the GPU test
S = Spec
BOTH = (torch.float32, torch.bfloat16)
BF16 = (torch.bfloat16,)
FP32 = (torch.float32,)
OPTION_SPECS = [S((10, 9, 8), (7, 7, 7), (3, 3, 3), 2, 32), S((6, 6, 6), (6, 6, 6), (0, 0, 0), 3, 48)]
LAYOUT_SPEC = OPTION_SPECS[0]
PRODUCTION = S((33, 20, 19), (7, 7, 7), (3, 3, 3), 6, 96, B=1)        # 45 windows x 6 heads = 270 units
# (spec, dtypes), grouped as the table of the GPU test's docstring
GEOMETRY = [
    # shift on two axes, on one
    (S((14, 14, 7), (7, 7, 7), (3, 3, 0), 2, 32), BOTH), (S((7, 14, 14), (7, 7, 7), (0, 3, 3), 2, 32), BOTH), (S((14, 7, 4), (7, 7, 4), (3, 0, 0), 2, 32), BOTH),
    # clipped anisotropic windows under the base-7 decode
    (S((7, 7, 4), (7, 7, 4), (0, 0, 0), 3, 48), BOTH), (S((4, 7, 7), (4, 7, 7), (0, 0, 0), 3, 48), BOTH),
    # n % 32 == 0: the forward without a ragged tile
    (S((8, 8, 8), (4, 4, 4), (2, 2, 2), 4, 64), BOTH), (S((8, 8, 8), (4, 4, 4), (0, 0, 0), 4, 64), BOTH), (S((4, 4, 2), (4, 4, 2), (0, 0, 0), 1, 16), BOTH),
    (S((8, 8, 5), (8, 8, 5), (0, 0, 0), 1, 16), BOTH),
    # n % 16 == 0, n % 32 != 0
    (S((8, 8, 6), (4, 4, 3), (2, 2, 1), 2, 32), BOTH),
    # tiny windows
    (S((3, 3, 3), (3, 3, 3), (0, 0, 0), 2, 32), BOTH), (S((6, 6, 6), (3, 3, 3), (1, 1, 1), 2, 32), BOTH), (S((4, 4, 4), (2, 2, 2), (1, 1, 1), 1, 16), BOTH),
    # padding on one axis only, mostly-padding windows under a shift; the same without a bias row
    (S((8, 7, 7), (7, 7, 7), (0, 0, 0), 3, 48), BOTH), (S((9, 5, 6), (4, 4, 4), (2, 2, 2), 2, 32), BOTH),
    (S((8, 7, 7), (7, 7, 7), (0, 0, 0), 3, 48, bias=False), BOTH), (S((9, 5, 6), (4, 4, 4), (2, 2, 2), 2, 32, bias=False), BOTH),
    # capacity edges (tw = 8: a table of 15^3 entries)
    (S((11, 8, 4), (11, 8, 4), (0, 0, 0), 1, 16, tw=8), BOTH), (S((6, 8, 8), (6, 8, 8), (0, 0, 0), 1, 16, tw=8), BOTH), (S((6, 6, 10), (6, 6, 10), (0, 0, 0), 1, 16, tw=8), BOTH),
    # unit mapping: 1, 27 and 9 units
    (S((7, 7, 7), (7, 7, 7), (0, 0, 0), 1, 16, B=1), BOTH), (S((21, 21, 21), (7, 7, 7), (3, 3, 3), 1, 16, B=1), BOTH), (S((7, 7, 7), (7, 7, 7), (0, 0, 0), 3, 48, B=3), BOTH),
    # the production form: >= 256 units with a remainder, padded, masked
    (PRODUCTION, BF16),
    # the 256-unit boundary at n = 64: 256 units (8 waves, 6 of them without a tile) and 192 (11 waves)
    (S((16, 16, 16), (4, 4, 4), (2, 2, 2), 4, 64, B=1), BOTH), (S((16, 16, 12), (4, 4, 4), (2, 2, 2), 4, 64, B=1), BOTH),
    # sharp softmax: through the fp32 table; fp32 also through q and k (the running-maximum rescale of the query-lane kernels)
    (S((10, 9, 8), (7, 7, 7), (3, 3, 3), 2, 32, table_amp=4.0), BOTH), (S((10, 9, 8), (7, 7, 7), (3, 3, 3), 2, 32, qk_gain=3.0), FP32),
]
# head dims of the query-lane kernels (a table keeps the global kernels away at head_dim 64); bf16 head_dim 16 without a table
HEAD_DIMS = [(S((10, 9, 8), (7, 7, 7), (3, 3, 3), 2, 2 * hd), BOTH) for hd in (8, 12, 32)] + [(S((6, 6, 6), (6, 6, 6), (0, 0, 0), 2, 128), BOTH),
                                                                                              (S((10, 9, 8), (7, 7, 7), (3, 3, 3), 2, 32, table=False), BF16)]
# global head_dim-64 kernels (bf16, no table, one window = the grid): NP / 16 = 6, 10, 12; n = 1, 2; B = 1 and 3; above GA_MAXN = 256
GLOBAL = [S(d, d, (0, 0, 0), 1, 64, B=B, bias=False, table=False) for d, B in (((4, 4, 5), 1), ((5, 5, 6), 3), ((5, 6, 6), 1), ((1, 1, 1), 3), ((1, 1, 2), 1))]
GLOBAL_ABOVE = S((6, 6, 8), (6, 6, 8), (0, 0, 0), 1, 64, B=1, bias=False, table=False)       # n = 288 > 256: the query-lane head_dim-64 kernels
GLOBAL_LAYOUT = GLOBAL[0]


def all_bf16_specs():
    """every Spec the GPU test runs in bf16, once"""
    seen = []
    for s, dts in GEOMETRY + HEAD_DIMS:
        if torch.bfloat16 in dts:
            seen.append(s)
    for s in OPTION_SPECS + GLOBAL + [GLOBAL_ABOVE]:
        seen.append(s)
    return list(dict.fromkeys(seen))
