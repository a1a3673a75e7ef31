"""Plain torch references of the (conditional) instance-norm family of csrc/norm.hip, one function per operation, and the inputs, case matrix
and tolerances that tests/test_instnorm_ref_cpu.py (CPU) and tests/test_hip_instnorm_forms.py (GPU) share.

    forward     y = act(norm(x; styles, gamma, beta) [+ res | + norm_b(res)])      biased variance, eps inside the root
    backward    autograd of that composition: dx (+ gadd), dres, dgamma / dbeta per style
    pair        y = LeakyReLU(norm_a(xa) + norm_b(xb)): dxa, dxb and the four affine gradients

Tensors are channels-last [B, S, C]; `styles` is a list of B style ids or None (every sample takes row 0); `gammas` / `betas` are lists of
[C] rows (one per style) or None.  Every function computes in `work` (float64: the reference) on whatever device its inputs live on.

The yardstick for honest arithmetic (`*_yardstick`) runs the same composition in fp32 on the dtype-rounded inputs and rounds y / dx / dres
ONCE to the compute dtype: that is what a correct kernel does.  torch's own bf16 run is no yardstick here: its intermediate roundings flip
LeakyReLU signs and put single dx elements 0.5 .. 3 away."""
import torch
import torch.nn.functional as F

EPS = 1e-5
SLOPE = 0.01
TOL = {torch.float32: 2e-4, torch.bfloat16: 2e-2}
FUSED_MAX_ROWS = 2048          # miseg_instnorm_fused_max_rows(): the register-resident one-launch kernels up to here, the streaming pairs above


def nvec(dtype):
    """V: elements of one 16-byte vector (8 bf16, 4 fp32)"""
    return 16 // torch.empty(0, dtype=dtype).element_size()


def fwd_tol(dtype):
    return TOL[dtype]


def bwd_tol(dtype, S):
    """the bars the existing tests of the same calls use: streaming backward TOL (fp32) / 3 TOL (bf16) (test_instnorm_fwd_bwd), fused backward
    4 TOL (test_instnorm_fused_small)"""
    if S <= FUSED_MAX_ROWS:
        return 4 * TOL[dtype]
    return TOL[dtype] * (3 if dtype == torch.bfloat16 else 1)


# ----------------------------------------------------------------------------------------------------------------- the case matrix
STREAM_S = FUSED_MAX_ROWS + 1      # 2049: 65 chunks of 32 rows with 32 columns (more than the 16 replicas), 3 chunks with one column (the last: one
#                                    row) - the rows `*-S2049-C*-onetile` / `-scalar1` of tests/instnorm_cases.py hold these figures
FUSED_ROWS = (2, 8, 16, 17, 27, 256, 257, 512, 513, 1024, 1025, 2047, 2048)
LONG_S = 1024 * 1024 + 1029        # the 1024-row cap of rows per workgroup with more chunks than any launcher's target grid (rows `*-rowcap`: 1026 chunks)


def stream_channels(dtype):
    """(id, C): tx = 3 (ty = 85, one idle thread); one full tile; two tiles with 8 of 32 columns live in the second; the scalar instantiation with
    one column; scalar, two tiles, 18 live.  Each id is the tag of the rows of tests/instnorm_cases.py (section a) that hold these figures as
    literal numbers, asserted on the calls' plans (tests/test_instnorm_plan_cpu.py, and beside the launches of the GPU cases)."""
    V = nvec(dtype)
    return [("tx3", 3 * V), ("onetile", 32 * V), ("twotiles", 40 * V), ("scalar1", 1), ("scalar50", 50)]


def fused_shapes(dtype):
    """(S, C): one vector and three scalar columns at every row count; dead channel columns in the last workgroup: tx = 8 with 5 columns, two
    workgroups with one live column in the second, scalar 8 + 5.  Held by the rows `-tyfloor` / `-ty32` / `-ty256` / `-lane4` / `-lane2` /
    `-dead3of8` / `-dead15of16` of tests/instnorm_cases.py (section b)."""
    V = nvec(dtype)
    return [(S, C) for S in FUSED_ROWS for C in (V, 3)] + [(27, 5 * V), (16, 17 * V), (27, 13)]


def option_shapes(dtype):
    V = nvec(dtype)
    return [(STREAM_S, 3 * V), (STREAM_S, 50), (27, 5 * V), (27, 13)]


# option -> what it changes of the network's combination (styles [1, 0], both affine rows, LeakyReLU, residual, dres wanted, no gadd, y given)
OPTIONS = {
    "network": {},
    "nostyles": {"styles": None},
    "noaffine": {"affine": "none"},
    "gammaonly": {"affine": "gamma"},
    "nullgrads1": {"null_style": 1},
    "actnone": {"act": False},
    "nores": {"res": False},
    "nores_gammaonly": {"res": False, "affine": "gamma"},
    "nodres": {"want_dres": False},
    "gadd": {"gadd": True},
    "network_gadd_nodres": {"gadd": True, "want_dres": False},
    "nores_gadd_actnone": {"res": False, "gadd": True, "act": False},
}


class Case:
    """deterministic inputs of one (B, S, C, dtype): every channel and sample has its own mean and spread, so statistics, affine rows or styles
    taken from a neighbour show; drawn on the CPU (or on `device` for the long rows) and rounded to `dtype`"""

    def __init__(self, B, S, C, dtype, device="cpu", seed=0, on_device=False):
        self.B, self.S, self.C, self.dtype = B, S, C, dtype
        g = torch.Generator(device=device if on_device else "cpu").manual_seed(1000 * seed + 7 * S + C)
        draw_on = device if on_device else "cpu"

        def rn(*shape):
            return torch.randn(*shape, generator=g, device=draw_on).to(device)
        ch = torch.arange(C, dtype=torch.float32, device=device)
        smp = torch.arange(B, dtype=torch.float32, device=device)[:, None, None]
        spread = 0.5 + 1.5 * ((ch * 0.37) % 1.0)
        spread_b = 0.5 + 1.5 * ((ch * 0.53 + 0.2) % 1.0)
        shift = ((ch * 0.61) % 1.0) * 2 - 1 + 0.25 * smp
        amp = 1.0
        if S == 2:
            # Two rows: xhat = +-(1 - d) with d = eps / (2 var), and the input gradient is the fraction 2 d of its own terms - at inputs of
            # amplitude 1 (var ~ 1, d ~ 5e-6) that is 1e-5 of them, which fp32 arithmetic (u = 6e-8) resolves to 1e-2 .. 1e-3 at best: measured
            # on the CPU, the fp32-compute yardstick stood between 3e-7 and 3.8e-3 from one draw to the next, around the fp32 bar of 8e-4.
            # Inputs of a sixteenth of the amplitude (var ~ 4e-3, d ~ 1e-3; the ratio of mean to spread stays what it is at every other S)
            # leave a gradient that fp32 resolves to 1e-4 or better, so the bar can tell a wrong kernel from rounding.  What the case is
            # for - the ty floor, 14 of 16 row lanes idle - does not depend on the amplitude.
            amp = 1.0 / 16
        spread, spread_b, shift = spread * amp, spread_b * amp, shift * amp
        self.x = (rn(B, S, C) * spread + shift).to(dtype)
        self.xb = (rn(B, S, C) * spread_b - 0.5 * shift).to(dtype)      # the second norm's input of the pair form
        self.res = rn(B, S, C).to(dtype)
        self.dy = rn(B, S, C).to(dtype)
        self.gadd = rn(B, S, C).to(dtype)
        # distinct affine rows per style (and per norm of the pair)
        self.gam = [rn(C) * 0.2 + 1 + 0.3 * s for s in range(2)]
        self.bet = [rn(C) * 0.2 - 0.1 * s for s in range(2)]
        self.gam_b = [rn(C) * 0.2 + 0.8 - 0.2 * s for s in range(2)]
        self.bet_b = [rn(C) * 0.2 + 0.1 * s for s in range(2)]

    def config(self, styles="default", affine="both", act=True, res=True, want_dres=True, gadd=False, null_style=None):
        """the operands of one option combination: dict(styles, gam, bet, res, gadd, act, want_dres, null_style)"""
        if styles == "default":
            styles = [(i + 1) % 2 for i in range(self.B)]
        ns = 2 if styles is not None else 1
        return {"styles": styles, "gam": self.gam[:ns] if affine != "none" else None, "bet": self.bet[:ns] if affine == "both" else None,
                "res": self.res if res else None, "gadd": self.gadd if gadd else None, "act": act, "want_dres": want_dres and res, "null_style": null_style}


# ----------------------------------------------------------------------------------------------------------------- the composition
def norm(x, styles, gammas, betas, eps=EPS, moments=None):
    """(x - mean) / sqrt(var + eps) * gamma[style] + beta[style] over the S rows of every (sample, channel); moments = (mean, var) [B, 1, C]
    replaces the statistics (the mutation checks)"""
    B = x.shape[0]
    if moments is None:
        mu = x.mean(1, keepdim=True)
        var = ((x - mu) ** 2).mean(1, keepdim=True)
    else:
        mu, var = moments
    out = (x - mu) / torch.sqrt(var + eps)
    idx = styles if styles is not None else [0] * B
    if gammas is not None:
        out = out * torch.stack([gammas[s] for s in idx])[:, None]
    if betas is not None:
        out = out + torch.stack([betas[s] for s in idx])[:, None]
    return out


def forward(x, styles, gammas, betas, res=None, res_norm=None, act=True, slope=SLOPE, eps=EPS, work=torch.float64, moments=None, unsure=None):
    """y in `work`.  unsure (a list): receives the mask of the elements whose activation sign fp32 cannot determine (SIGN_EPS).  res_norm = (gammas_b, betas_b): `res` is the raw input of a second norm with these affine rows (the pair form)"""
    c = lambda t: None if t is None else t.to(work)      # noqa: E731
    cl = lambda ts: None if ts is None else [t.to(work) for t in ts]      # noqa: E731
    y = norm(c(x), styles, cl(gammas), cl(betas), eps, moments)
    scale = y.detach().abs()
    if res is not None:
        r = norm(c(res), styles, cl(res_norm[0]), cl(res_norm[1]), eps) if res_norm is not None else c(res)
        y, scale = y + r, scale + r.detach().abs()
    if unsure is not None and act:
        unsure.append(y.detach().abs() < SIGN_EPS * (1 + scale))
    return F.leaky_relu(y, slope) if act else y


# A LeakyReLU multiplies the gradient by 1 or by `slope` according to the sign of a pre-activation that the kernels (and the yardstick) form in
# fp32 from statistics summed in fp32 partials: where the exact pre-activation lies within 2e-5 of zero (relative to 1 + the magnitudes of its
# terms; fp32 arithmetic reaches about 1e-6 there) no finite-precision run determines that sign, and the element's gradient is 100 times as
# large on one side as on the other.  The float64 reference marks these elements of dx / dres (about 1 in 50 000) NaN and the
# tests compare the rest (determined()); their weight in the sums behind the other outputs is 1 / S.
SIGN_EPS = 2e-5


def determined(got, ref):
    """(got, ref) with the elements the reference marks NaN (SIGN_EPS) set to zero in both: what the parity metrics are taken over"""
    m = torch.isnan(ref)
    return torch.where(m.to(got.device), torch.zeros_like(got), got), torch.where(m, torch.zeros_like(ref), ref)


def _mask(t, unsure):
    if t is None or not unsure:
        return t
    return torch.where(unsure[0], torch.full_like(t, float("nan")), t)


def _leaves(ts, work):
    return None if ts is None else [t.detach().to(work).requires_grad_(True) for t in ts]


def _grads(leaves, n):
    if leaves is None:
        return [None] * n
    return [l.grad if l.grad is not None else torch.zeros_like(l) for l in leaves]


def backward(dy, x, styles, gammas, betas, res=None, act=True, gadd=None, slope=SLOPE, eps=EPS, work=torch.float64):
    """autograd of forward(): dict(y, dx, dres, dgamma [per style], dbeta [per style]) in `work`; dx includes gadd when given.  A style no
    sample uses has a zero gradient.  In float64 the elements of dx / dres behind an undeterminable activation sign are NaN (SIGN_EPS)."""
    xl = x.detach().to(work).requires_grad_(True)
    rl = res.detach().to(work).requires_grad_(True) if res is not None else None
    gl, bl = _leaves(gammas, work), _leaves(betas, work)
    unsure = [] if work == torch.float64 else None
    y = forward(xl, styles, gl, bl, res=rl, act=act, slope=slope, eps=eps, work=work, unsure=unsure)
    y.backward(dy.to(work))
    ns = len(gammas) if gammas is not None else (len(betas) if betas is not None else 0)
    dx = xl.grad if gadd is None else xl.grad + gadd.to(work)
    return {"y": y.detach(), "dx": _mask(dx, unsure), "dres": _mask(rl.grad, unsure) if rl is not None else None, "dgamma": _grads(gl, ns), "dbeta": _grads(bl, ns)}


def pair_backward(dy, xa, xb, styles, gammas_a, betas_a, gammas_b, betas_b, slope=SLOPE, eps=EPS, work=torch.float64, mark=True):
    """y = LeakyReLU(norm_a(xa) + norm_b(xb)): dict(y, dxa, dxb, dgamma_a, dbeta_a, dgamma_b, dbeta_b).  mark = False: no element is marked
    NaN - for inputs whose dy is zero wherever the sign is undeterminable (rank1_case), so that either sign gives the same gradients"""
    al = xa.detach().to(work).requires_grad_(True)
    bl = xb.detach().to(work).requires_grad_(True)
    ga, ba, gb, bb = _leaves(gammas_a, work), _leaves(betas_a, work), _leaves(gammas_b, work), _leaves(betas_b, work)
    unsure = [] if (work == torch.float64 and mark) else None
    y = forward(al, styles, ga, ba, res=bl, res_norm=(gb, bb), act=True, slope=slope, eps=eps, work=work, unsure=unsure)
    y.backward(dy.to(work))
    n = lambda ts: len(ts) if ts is not None else 0      # noqa: E731
    return {"y": y.detach(), "dxa": _mask(al.grad, unsure), "dxb": _mask(bl.grad, unsure), "dgamma_a": _grads(ga, n(gammas_a)), "dbeta_a": _grads(ba, n(betas_a)),
            "dgamma_b": _grads(gb, n(gammas_b)), "dbeta_b": _grads(bb, n(betas_b))}


# ----------------------------------------------------------------------------------------------------------------- the rank-1 pair
def rank1_channels(dtype):
    """C of the rank-1 pair cases at STREAM_S rows: two channel tiles with one live column in the second; scalar lanes, 18 live in the second"""
    return [33 * nvec(dtype), 50]


class Rank1Case:
    """the pair backward whose second input is the unstored product xb[row][c] = round(r1x[row] * r1w[c]) (the stem block's one-channel 1x1x1
    shortcut), B = 2, S = STREAM_S.  xa, gradient and affine rows are those of Case; three things are shaped for the weight gradient
    dW[c] = sum over rows of round(dxb[row][c]) * r1x[row] (the rounding is the kernels' definition: csrc/norm.hip, instnorm_pair_bwd_apply_kernel):

    * r1x and r1w have amplitude 0.03, so the product's variance (1e-6) lies below eps: a norm in front of which the convolution's scale
      survives.  At amplitude 1 the norm removes that scale and dW is what is left of terms that cancel 20 000-fold (measured: |dW| 0.06 of
      summed |terms| 1256), which no fp32 run resolves to the bar;
    * dy carries the sign of r1x, so the terms of dW add up (measured: |dW| 7600 of summed |terms| 8200) instead of cancelling like a random
      walk (1 / 64 at 4098 rows) - one bf16 ulp of one term, where fp32 and float64 round dxb to different neighbours, is then 1e-6 of dW
      and not 6e-5, 3 of which in one channel would stand above the bar;
    * dy is zero wherever float64 cannot sign the pre-activation (SIGN_EPS; 4 to 25 elements): either sign gives the same gradients, so no
      element has to be left out of sums that no test can take apart again.

    What the cases are for - the rank-1 epilogue with a ragged last channel tile and with scalar lanes - depends on none of it."""

    def __init__(self, dtype, C, device="cpu"):
        c = Case(2, STREAM_S, C, dtype, device=device)
        g = torch.Generator().manual_seed(99 + C)
        self.B, self.S, self.C, self.dtype = 2, STREAM_S, C, dtype
        self.styles = [1, 0]
        self.xa, self.gam, self.bet, self.gam_b, self.bet_b = c.x, c.gam, c.bet, c.gam_b, c.bet_b
        self.r1x = (torch.randn(2, STREAM_S, 1, generator=g) * 0.03).to(device).to(dtype)
        self.r1w = ((torch.randn(C, generator=g) * 0.3 + 1) * 0.03).to(device).to(dtype)
        self.xb = (self.r1x.float() * self.r1w.float()).to(dtype)      # one rounding of the fp32 product, as the kernels form it
        unsure = []
        forward(self.xa, self.styles, self.gam, self.bet, res=self.xb, res_norm=(self.gam_b, self.bet_b), unsure=unsure)
        sign = torch.where(self.r1x < 0, -1.0, 1.0).to(dtype)
        self.dy = torch.where(unsure[0], torch.zeros_like(c.dy), c.dy.abs() * sign)
        self.n_unsure = int(unsure[0].sum())

    def backward(self, work=torch.float64):
        """pair_backward on the materialised product plus dw: the row sum of dxb, rounded once to the compute dtype, times r1x, in float64"""
        r = pair_backward(self.dy, self.xa, self.xb, self.styles, self.gam, self.bet, self.gam_b, self.bet_b, work=work, mark=False)
        r["dw_terms"] = r["dxb"].to(self.dtype).double() * self.r1x.double()
        r["dw"] = r["dw_terms"].sum((0, 1))
        return r


# ----------------------------------------------------------------------------------------------------------------- the yardstick
def _once(t, dtype):
    return None if t is None else t.to(dtype)


def backward_yardstick(dtype, dy, x, styles, gammas, betas, res=None, act=True, gadd=None, slope=SLOPE, eps=EPS):
    """the same composition in fp32 on the (already dtype-rounded) inputs; y / dx / dres rounded once to `dtype`, the affine gradients stay fp32"""
    r = backward(dy, x, styles, gammas, betas, res=res, act=act, gadd=gadd, slope=slope, eps=eps, work=torch.float32)
    for k in ("y", "dx", "dres"):
        r[k] = _once(r[k], dtype)
    return r


def pair_backward_yardstick(dtype, dy, xa, xb, styles, gammas_a, betas_a, gammas_b, betas_b, slope=SLOPE, eps=EPS):
    r = pair_backward(dy, xa, xb, styles, gammas_a, betas_a, gammas_b, betas_b, slope=slope, eps=eps, work=torch.float32)
    for k in ("y", "dxa", "dxb"):
        r[k] = _once(r[k], dtype)
    return r
