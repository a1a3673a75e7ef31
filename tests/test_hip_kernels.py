"""GPU parity tests, kernel level: every C-ABI entry point against a plain PyTorch float64 reference of the same op on the same (fp32 or
bf16-rounded) inputs, run on the device -- tolerances: fp32 path 2e-4 (north_star asks 1e-3), bf16 path 2e-2, each held both by the pooled
relative L2 error and by the per-element metric of tests/parity.py (assert_parity)."""
import math
import os
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from parity import assert_parity, local_err
from winattn_ref import dqkv_local_tol as _dqkv_local_tol, ref_window_attention as _ref_window_attention

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {torch.float32: 2e-4, torch.bfloat16: 2e-2}


def _ops():
    from mi_seg_amd.hip import ops
    return ops


def _L():
    from mi_seg_amd.hip import lib
    return lib


def _gemm_plan(M, N, K, **fields):
    """the plan miseg_gemm dispatches on for a contiguous, aligned problem of this shape (gemm_cases.params keywords)"""
    import ctypes
    import gemm_cases
    plan = _L().GemmPlan()
    assert _L().load().miseg_gemm_plan(ctypes.byref(gemm_cases.params(_L(), M, N, K, **fields)), ctypes.byref(plan)) == 0
    return plan


def rnd(*shape, dtype=torch.float32, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


def test_library_loads_and_reports_arch():
    import ctypes
    L = _L()
    lib = L.load()
    assert lib.miseg_abi_version() == L.ABI_VERSION
    buf = ctypes.create_string_buffer(16)
    assert lib.miseg_device_arch(buf, 16) == 0 and buf.value == b"gfx950"
    L.check_device(0)          # the card really is what the embedded code objects were built for


def test_integration_md_stub_runs():
    """the per-op binding shown in INTEGRATION.md, executed verbatim, against the reference's per-sample loop
    (networks/norms/conditional_instance_norm.py:59-60) restated with F.instance_norm"""
    import os
    import re
    from conftest import ROOT
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    code = re.search(r"```python\n(import ctypes as C, torch\n.*?)```", md, flags=re.S).group(1)
    ns = {}
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        exec(compile(code, "INTEGRATION.md", "exec"), ns)
    finally:
        os.chdir(cwd)
    norms = torch.nn.ModuleList([torch.nn.InstanceNorm3d(24, affine=True) for _ in range(2)]).to(DEV)
    for i, n in enumerate(norms):
        torch.nn.init.normal_(n.weight, 1.0, 0.3)
        torch.nn.init.normal_(n.bias, 0.0, 0.3)
    x = rnd(3, 5, 6, 7, 24)
    styles = [1, 0, 1]
    y = ns["cond_instance_norm_ndhwc"](x, torch.tensor(styles, dtype=torch.int32, device=DEV), norms)
    xc = x.permute(0, 4, 1, 2, 3)
    xc = xc.double()
    want = torch.stack([F.instance_norm(xc[i:i + 1], weight=norms[s].weight.double(), bias=norms[s].bias.double())[0] for i, s in enumerate(styles)]).permute(0, 2, 3, 4, 1)
    assert_parity(y, want, 2e-5, "INTEGRATION.md stub against float64")


def test_bad_args_raise_value_error():
    ops = _ops()
    with pytest.raises((ValueError, RuntimeError)):
        ops.gemm_nt(rnd(4, 8), rnd(3, 9))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,S,C", [(2, 210, 6), (1, 4096 + 17, 48), (3, 27, 3072), (2, 1000, 96)])
def test_instnorm_fwd_bwd(dtype, B, S, C):
    ops, L = _ops(), _L()
    x = rnd(B, S, C, dtype=dtype, seed=1) * 1.5 + 0.3
    res = rnd(B, S, C, dtype=dtype, seed=2)
    gam = [rnd(C, seed=3) * 0.2 + 1, rnd(C, seed=4) * 0.2 + 1]
    bet = [rnd(C, seed=5) * 0.1, rnd(C, seed=6) * 0.1]
    styles_h = [(i + 1) % 2 for i in range(B)]
    styles = torch.tensor(styles_h, dtype=torch.int32, device=DEV)
    stat = ops.instnorm_stats(x, B, S)
    mean = (stat.sum(0)[..., 0] / S).float()
    y = ops.instnorm_apply(x, B, S, stat, styles, gam, bet, res=res, act=L.ACT_LEAKY, slope=0.01)
    # reference (fp32 on device)
    xf = x.double().requires_grad_(True)
    rf = res.double().requires_grad_(True)
    gp = [g.double().requires_grad_(True) for g in gam]
    bp = [b.double().requires_grad_(True) for b in bet]
    outs = []
    for i in range(B):
        s = styles_h[i]
        mu = xf[i].mean(0, keepdim=True)
        var = xf[i].var(0, unbiased=False, keepdim=True)
        outs.append((xf[i] - mu) / torch.sqrt(var + 1e-5) * gp[s] + bp[s])
    yr = F.leaky_relu(torch.stack(outs) + rf, 0.01)
    assert_parity(mean, xf.mean(1), 1e-4, "mean from the statistics")
    assert_parity(y, yr, TOL[dtype], "y against float64")
    # the check bites on real output: the kernel's result against the reference with its last row lost must fail
    lost = yr.detach().clone()
    lost[B - 1, S - 1] = 0
    with pytest.raises(AssertionError):
        assert_parity(y, lost, TOL[dtype], "mutated reference: last row zeroed")
    dy = rnd(B, S, C, dtype=dtype, seed=7)
    yr.backward(dy.double())
    dg = [torch.zeros(C, device=DEV) for _ in range(2)]
    db = [torch.zeros(C, device=DEV) for _ in range(2)]
    dx, dres = ops.instnorm_bwd(dy, y, x, B, S, stat, styles, gam, dg, db, act=L.ACT_LEAKY, slope=0.01, want_dres=True)
    tol = TOL[dtype] * (3 if dtype == torch.bfloat16 else 1)
    assert_parity(dx, xf.grad, tol, "dx against float64")
    assert_parity(dres, rf.grad, tol, "dres against float64")
    for s in set(styles_h):
        assert_parity(dg[s], gp[s].grad, tol, f"dgamma of style {s}")
        assert_parity(db[s], bp[s].grad, tol, f"dbeta of style {s}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,S,C", [(2, 700, 24), (1, 4096 + 17, 48), (3, 530, 10)])
def test_instnorm_residual_pair(dtype, B, S, C):
    """y = LeakyReLU(norm_a(xa) + norm_b(xb)) in one apply pass (the shortcut norm rides as `res_stat`) and its joint backward (one
    reduction + one apply launch for both norms): against fp64 autograd of the composition, per-sample styles."""
    ops, L = _ops(), _L()
    xa = rnd(B, S, C, dtype=dtype, seed=31) * 1.5 + 0.3
    xb = rnd(B, S, C, dtype=dtype, seed=32) * 0.7 - 0.2
    gam = [[rnd(C, seed=33 + 4 * k + s) * 0.2 + 1 for s in range(2)] for k in range(2)]
    bet = [[rnd(C, seed=35 + 4 * k + s) * 0.1 for s in range(2)] for k in range(2)]
    styles_h = [(i + 1) % 2 for i in range(B)]
    styles = torch.tensor(styles_h, dtype=torch.int32, device=DEV)
    sa, sb = ops.instnorm_stats(xa, B, S), ops.instnorm_stats(xb, B, S)
    y = ops.instnorm_apply(xa, B, S, sa, styles, gam[0], bet[0], res=xb, act=L.ACT_LEAKY, slope=0.01, res_stat=sb, res_gammas=gam[1], res_betas=bet[1])
    xs = [xa.double().requires_grad_(True), xb.double().requires_grad_(True)]
    gp = [[g.double().requires_grad_(True) for g in gam[k]] for k in range(2)]
    bp = [[b.double().requires_grad_(True) for b in bet[k]] for k in range(2)]
    outs = []
    for i in range(B):
        s = styles_h[i]
        tot = 0
        for k in range(2):
            mu = xs[k][i].mean(0, keepdim=True)
            var = xs[k][i].var(0, unbiased=False, keepdim=True)
            tot = tot + (xs[k][i] - mu) / torch.sqrt(var + 1e-5) * gp[k][s] + bp[k][s]
        outs.append(tot)
    yr = F.leaky_relu(torch.stack(outs), 0.01)
    assert_parity(y, yr, TOL[dtype], "y of the pair against float64")
    dy = rnd(B, S, C, dtype=dtype, seed=47)
    yr.backward(dy.double())
    dg = [[torch.zeros(C, device=DEV) for _ in range(2)] for _ in range(2)]
    db = [[torch.zeros(C, device=DEV) for _ in range(2)] for _ in range(2)]
    dxa, dxb = ops.instnorm_pair_bwd(dy, y, xa, xb, B, S, sa, sb, styles, gam[0], gam[1], dg[0], db[0], dg[1], db[1], slope=0.01)
    tol = TOL[dtype] * (3 if dtype == torch.bfloat16 else 1)
    assert_parity(dxa, xs[0].grad, tol, "dxa against float64")
    assert_parity(dxb, xs[1].grad, tol, "dxb against float64")
    for k in range(2):
        for s in set(styles_h):
            assert_parity(dg[k][s], gp[k][s].grad, tol, f"dgamma of norm {k}, style {s}")
            assert_parity(db[k][s], bp[k][s].grad, tol, f"dbeta of norm {k}, style {s}")
    # without y the kernels recompute the activation's sign from xa / xb with the forward's own expression: the same bits
    dg2 = [[torch.zeros(C, device=DEV) for _ in range(2)] for _ in range(2)]
    db2 = [[torch.zeros(C, device=DEV) for _ in range(2)] for _ in range(2)]
    dxa2, dxb2 = ops.instnorm_pair_bwd(dy, None, xa, xb, B, S, sa, sb, styles, gam[0], gam[1], dg2[0], db2[0], dg2[1], db2[1], slope=0.01,
                                       betas_a=bet[0], betas_b=bet[1])
    assert torch.equal(dxa2, dxa) and torch.equal(dxb2, dxb)
    for k in range(2):
        for s in set(styles_h):
            assert_parity(dg2[k][s], dg[k][s], 1e-6, f"dgamma of norm {k}, style {s}: sign recomputed against y given")
            assert_parity(db2[k][s], db[k][s], 1e-6, f"dbeta of norm {k}, style {s}: sign recomputed against y given")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("S,C", [(4096 + 17, 48), (3000, 24), (2100, 16)])
def test_instnorm_residual_pair_rank1_shortcut(dtype, S, C):
    """the stem block's shortcut conv1x1x1(one-channel image) is never materialised: its product is formed inside the pair's apply and
    backward kernels (r1x / r1w) and its weight gradient is reduced by the backward kernel - against the materialised path: the same
    bits for y and dxa (the product is rounded exactly as the rank-1 GEMM rounds it), the weight gradient against the TN GEMM."""
    ops, L = _ops(), _L()
    B = 1
    xa = rnd(B, S, C, dtype=dtype, seed=71) * 1.5 + 0.3
    x1 = rnd(B, S, 1, dtype=dtype, seed=72)
    w = (rnd(C, 1, dtype=dtype, seed=73) * 0.8).contiguous()
    gam = [[rnd(C, seed=33 + 4 * k + s) * 0.2 + 1 for s in range(2)] for k in range(2)]
    bet = [[rnd(C, seed=35 + 4 * k + s) * 0.1 for s in range(2)] for k in range(2)]
    styles = torch.tensor([1], dtype=torch.int32, device=DEV)
    ops.begin_step()
    xb = ops.gemm_nt(x1, w)                                        # the materialised shortcut
    sa, sb = ops.instnorm_stats(xa, B, S), ops.instnorm_stats(xb, B, S)
    y_ref = ops.instnorm_apply(xa, B, S, sa, styles, gam[0], bet[0], res=xb, act=L.ACT_LEAKY, slope=0.01, res_stat=sb, res_gammas=gam[1], res_betas=bet[1])
    sb1 = ops.rank1_stats(x1, w)
    assert torch.allclose(sb1.sum(0), sb.sum(0), rtol=2e-6, atol=1e-3)
    y = ops.instnorm_apply(xa, B, S, sa, styles, gam[0], bet[0], act=L.ACT_LEAKY, slope=0.01, res_stat=sb, res_gammas=gam[1], res_betas=bet[1], r1=(x1, w))
    assert torch.equal(y, y_ref)
    dy = rnd(B, S, C, dtype=dtype, seed=47)

    def zeros():
        return [[torch.zeros(C, device=DEV) for _ in range(2)] for _ in range(2)]
    dg, db, dg2, db2 = zeros(), zeros(), zeros(), zeros()
    dxa_ref, dxb_ref = ops.instnorm_pair_bwd(dy, None, xa, xb, B, S, sa, sb, styles, gam[0], gam[1], dg[0], db[0], dg[1], db[1], slope=0.01,
                                             betas_a=bet[0], betas_b=bet[1])
    dw = torch.zeros(C, device=DEV)
    dxa, none = ops.instnorm_pair_bwd(dy, None, xa, None, B, S, sa, sb, styles, gam[0], gam[1], dg2[0], db2[0], dg2[1], db2[1], slope=0.01,
                                      betas_a=bet[0], betas_b=bet[1], r1=(x1, w, dw))
    assert none is None and torch.equal(dxa, dxa_ref)
    for k in range(2):
        assert_parity(dg2[k][1], dg[k][1], 1e-5, f"dgamma of norm {k}: rank-1 route against the materialised one")
        assert_parity(db2[k][1], db[k][1], 1e-5, f"dbeta of norm {k}: rank-1 route against the materialised one")
    terms = dxb_ref.double().reshape(S, C) * x1.double().reshape(S, 1)
    dw_ref = terms.sum(0)
    # This gradient all but vanishes (a 1x1x1 convolution in front of an instance norm: the norm removes its scale): each element is what is left
    # of S terms that cancel about a thousandfold.  Yardstick: torch's own fp32 sum of the same terms (exact products of
    # the rounded factors) against dw_ref, measured 1.2e-4 at 4113 x 48 fp32 and below 5e-5 in the other five cases; the kernel, which adds the terms in
    # float64 per thread and workgroup and in fp32 across workgroups, stands at 7e-7 .. 3.8e-5 (3.8e-5 / 2.0e-5 at 4113 x 48 fp32 / bf16).
    yard = local_err(terms.float().sum(0), dw_ref)[0]
    assert_parity(dw, dw_ref, 1e-4, "rank-1 dW against float64", local_tol=max(1e-4, 2 * yard))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_layernorm(dtype):
    ops = _ops()
    x = rnd(777, 96, dtype=dtype, seed=11)
    g, b = rnd(96, seed=12) * 0.2 + 1, rnd(96, seed=13) * 0.1
    y, mean, rstd = ops.layernorm_fwd(x, g, b)
    xf = x.double().clone().requires_grad_(True)
    gp, bp = g.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)
    yr = F.layer_norm(xf, (96,), gp, bp)
    assert_parity(y, yr, TOL[dtype], "y against float64")
    dy = rnd(777, 96, dtype=dtype, seed=14)
    yr.backward(dy.double())
    dg, db = torch.zeros(96, device=DEV), torch.zeros(96, device=DEV)
    dx = ops.layernorm_bwd(dy, x, g, mean, rstd, dg, db)
    assert_parity(dx, xf.grad, 2 * TOL[dtype], "dx against float64")
    assert_parity(dg, gp.grad, 2 * TOL[dtype], "dgamma against float64")
    assert_parity(db, bp.grad, 2 * TOL[dtype], "dbeta against float64")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(300, 144, 48), (1000, 48, 192), (129, 12, 12), (27, 768, 3072), (513, 96, 384), (64, 36, 20)])
def test_gemm_nt(dtype, M, N, K):
    ops, L = _ops(), _L()
    a, w, bias = rnd(M, K, dtype=dtype, seed=21), rnd(N, K, dtype=dtype, seed=22) / K ** 0.5, rnd(N, seed=23)
    y = ops.gemm_nt(a, w, bias)
    yr = a.double() @ w.double().t() + bias
    assert_parity(y, yr, TOL[dtype], "bias")
    y2 = ops.gemm_nt(a, w, bias, act=L.ACT_GELU)
    assert_parity(y2, F.gelu(yr), TOL[dtype], "bias + GELU")


@pytest.mark.parametrize("M,N,K", [(4096, 48, 48), (5003, 144, 48), (4100, 192, 48), (4097, 48, 192), (6000, 384, 96), (4099, 96, 96), (4300, 16, 96),
                                   (4101, 48, 144), (13824, 96, 288), (4200, 96, 384), (5000, 48, 384), (4098, 112, 288)])
def test_gemm_nt_streaming_path(M, N, K):
    """tall-skinny bf16 GEMMs take the weight-resident streaming kernel (M >= 4096, K in 48/96/144/192/288/384): ragged M, the
    half k-step of K = 48 / 144, N beyond one accumulator chunk, bias + GELU epilogue; exact on small integers."""
    ops, L = _ops(), _L()
    dtype = torch.bfloat16
    assert {_gemm_plan(M, N, K, bias=1, act=act).kernel for act in (L.ACT_NONE, L.ACT_GELU)} == {L.GEMM_NT_STREAM}
    a, w, bias = rnd(M, K, dtype=dtype, seed=21), rnd(N, K, dtype=dtype, seed=22) / K ** 0.5, rnd(N, seed=23)
    yr = a.double() @ w.double().t() + bias
    y = ops.gemm_nt(a, w, bias)
    assert_parity(y, yr, TOL[dtype], "bias")
    assert_parity(ops.gemm_nt(a, w, bias, act=L.ACT_GELU), F.gelu(yr), TOL[dtype], "bias + GELU")
    if M == 5003:
        # the check bites on real output: against a reference whose ragged tail row is lost, the kernel's result must fail
        lost = yr.clone()
        lost[M - 1] = 0
        with pytest.raises(AssertionError):
            assert_parity(y, lost, TOL[dtype], "mutated reference: tail row zeroed")
    ai = (torch.arange(M * K, device=DEV).reshape(M, K) % 7 - 3).to(dtype)
    wi = (torch.arange(N * K, device=DEV).reshape(N, K) % 5 - 2).to(dtype)
    assert torch.equal(ops.gemm_nt(ai, wi).float(), (ai.float() @ wi.float().t()).to(dtype).float())


@pytest.mark.parametrize("M,N,K,with_res", [(4096, 48, 48, False), (13825, 48, 192, True), (110592, 96, 96, True), (5003, 48, 96, False), (4101, 96, 192, True),
                                            (4099, 32, 48, False), (1728, 192, 192, True), (1728, 192, 768, True), (216, 384, 1536, True), (27, 768, 3072, False)])
def test_gemm_nt_streaming_statistics(M, N, K, with_res):
    """want_stat: the streaming kernel's epilogue leaves the instance-norm statistics (one sample = all M rows) of its ROUNDED output
    (bias and residual included) in the replicated fp64 buffer - against the separate statistics pass over the same output; a
    shape the path does not cover (N = 144, GELU) leaves no statistics and the caller falls back."""
    ops, L = _ops(), _L()
    dtype = torch.bfloat16
    a, w, bias = rnd(M, K, dtype=dtype, seed=21), rnd(N, K, dtype=dtype, seed=22) / K ** 0.5, rnd(N, seed=23)
    res = rnd(M, N, dtype=dtype, seed=24) if with_res else None
    plan = _gemm_plan(M, N, K, bias=1, stat=1, res=1 << 12 if with_res else None)
    assert (plan.kernel, plan.stat) == (L.GEMM_NT_STREAM if M > 2048 else L.GEMM_NT_SMALL, 1)
    ops.begin_step()
    y = ops.gemm_nt(a, w, bias, res=res, want_stat=True)
    st = ops.pop_gemm_stat(y)
    assert st is not None and st.shape[1:] == (1, N, 2)
    assert ops.pop_gemm_stat(y) is None                          # handed over once
    plain = ops.gemm_nt(a, w, bias, res=res)
    assert torch.equal(y, plain)                                 # same output as the plain instantiation
    got = st.sum(0)[0]                                           # [N, 2]
    yf = y.double()
    want = torch.stack([yf.sum(0), (yf * yf).sum(0)], -1)
    assert torch.allclose(got, want, rtol=2e-6, atol=1e-3), (got - want).abs().max()
    ref = ops.instnorm_stats(y.view(1, M, N), 1, M).sum(0)[0]
    assert torch.allclose(got, ref, rtol=2e-6, atol=1e-3)
    if M > 2048:      # (the small-M kernel of the deep stages - round 5 - has the epilogue for every width)
        y2 = ops.gemm_nt(a, rnd(144, K, dtype=dtype, seed=25), want_stat=True)
        assert ops.pop_gemm_stat(y2) is None
    y3 = ops.gemm_nt(a, w, bias, act=L.ACT_GELU, want_stat=True)
    assert ops.pop_gemm_stat(y3) is None


@pytest.mark.parametrize("grid,Cin,Cout", [((1, 17, 16, 16), 48, 48), ((2, 12, 14, 13), 96, 48), ((1, 16, 16, 16), 48, 24), ((1, 6, 6, 6), 96, 48)])
def test_gemm_nt_scatter_is_the_transposed_conv_store(grid, Cin, Cout):
    """the ConvTranspose3d(k2, s2) GEMM with the 2x2x2 scatter as its store (left half of a concat buffer) against the two-step path
    (GEMM to [voxels, 8*Cout], then channel_to_space): the same bits; a grid below the streaming path's size reports False."""
    ops = _ops()
    from mi_seg_amd.hip.functional import STD_OFFSETS
    dtype = torch.bfloat16
    B, d, h, w = grid
    x = rnd(B, d, h, w, Cin, dtype=dtype, seed=61)
    wf = rnd(8 * Cout, Cin, dtype=dtype, seed=62) / Cin ** 0.5
    cat = torch.full((B, 2 * d, 2 * h, 2 * w, 2 * Cout), 7.0, dtype=dtype, device=DEV)
    done = ops.gemm_nt_scatter(x, wf, cat[..., :Cout], grid)
    assert done == (B * d * h * w >= 4096)
    if not done:
        return
    plan = _gemm_plan(B * d * h * w, 8 * Cout, Cin, ldc=2 * Cout, scat=(d, h, w, Cout))
    assert (plan.kernel, plan.scat) == (_L().GEMM_NT_STREAM, 1)
    ref = torch.full_like(cat, 7.0)
    ops.channel_to_space(ops.gemm_nt(x, wf), STD_OFFSETS, (B, 2 * d, 2 * h, 2 * w, Cout), out=ref[..., :Cout])
    assert torch.equal(cat, ref)                      # the right half (the skip's place) untouched
    # and against the definition: out[b, 2d+jd, 2h+jh, 2w+jw, co] = sum_ci x[b,d,h,w,ci] * wf[(j,co), ci]
    y = (x.double().reshape(-1, Cin) @ wf.double().t()).reshape(B, d, h, w, 2, 2, 2, Cout)
    y = y.permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(B, 2 * d, 2 * h, 2 * w, Cout)
    assert_parity(cat[..., :Cout], y, TOL[dtype], "scattered store against the definition")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gemm_nt_rank1(dtype):
    """K == 1 (the stem block's 1x1x1 shortcut on a one-channel image): the outer-product kernel"""
    ops = _ops()
    dt = _L().BF16 if dtype == torch.bfloat16 else _L().F32
    assert (_gemm_plan(5003, 48, 1, dt=dt, bias=1).kernel, _gemm_plan(5003, 48, 1, dt=dt, stat=1).kernel) == (_L().GEMM_NT_RANK1, _L().GEMM_NT_RANK1_STAT)
    a, w, bias = rnd(5003, 1, dtype=dtype, seed=31), rnd(48, 1, dtype=dtype, seed=32), rnd(48, seed=33)
    yr = a.double() @ w.double().t()
    assert_parity(ops.gemm_nt(a, w), yr, TOL[dtype], "rank-1 product")
    assert_parity(ops.gemm_nt(a, w, bias), yr + bias, TOL[dtype], "rank-1 product + bias")
    # with the instance-norm statistics of the rounded output from the same launch (the stem block's shortcut feeds norm3)
    ops.begin_step()
    for b_ in (None, bias):
        y = ops.gemm_nt(a, w, b_, want_stat=True)
        st = ops.pop_gemm_stat(y)
        assert st is not None and torch.equal(y, ops.gemm_nt(a, w, b_))
        yd = y.double()
        want = torch.stack([yd.sum(0), (yd * yd).sum(0)], -1)
        assert torch.allclose(st.sum(0)[0], want, rtol=2e-6, atol=1e-3)


@pytest.mark.parametrize("M,N,K", [(216, 1536, 384), (216, 384, 1536), (27, 3072, 768), (1728, 768, 192), (1727, 192, 768), (215, 1152, 384), (100, 16, 32),
                                   (2048, 48, 96), (512, 256, 128), (512, 256, 96), (512, 256, 64), (2048, 64, 128),
                                   (216, 3072, 768), (200, 2880, 64)])      # the 64 x 48 tile (one round of <= 256 workgroups), ragged M
def test_gemm_nt_small_path(M, N, K):
    """deep-stage linears (M <= 2048, K % 32 == 0) take the register-direct kernel with K split over the four waves."""
    ops, L = _ops(), _L()
    dtype = torch.bfloat16
    assert {_gemm_plan(M, N, K, act=act).kernel for act in (L.ACT_NONE, L.ACT_GELU)} == {L.GEMM_NT_SMALL}
    a, w, bias = rnd(M, K, dtype=dtype, seed=21), rnd(N, K, dtype=dtype, seed=22) / K ** 0.5, rnd(N, seed=23)
    yr = a.double() @ w.double().t() + bias
    assert_parity(ops.gemm_nt(a, w, bias), yr, TOL[dtype], "bias")
    assert_parity(ops.gemm_nt(a, w, bias, act=L.ACT_GELU), F.gelu(yr), TOL[dtype], "bias + GELU")
    assert_parity(ops.gemm_nt(a, w), yr - bias, TOL[dtype], "no bias")
    ai = (torch.arange(M * K, device=DEV).reshape(M, K) % 7 - 3).to(dtype)
    wi = (torch.arange(N * K, device=DEV).reshape(N, K) % 5 - 2).to(dtype)
    assert torch.equal(ops.gemm_nt(ai, wi).float(), (ai.float() @ wi.float().t()).to(dtype).float())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(5000, 192, 48), (216, 1536, 384), (300, 144, 40), (13824, 96, 384)])
def test_gemm_nt_epilogues(dtype, M, N, K):
    """residual add, pre-activation side output and GELU-derivative epilogues on every NT kernel (streaming, small, generic)."""
    ops, L = _ops(), _L()
    family = {5000: L.GEMM_NT_STREAM, 13824: L.GEMM_NT_STREAM, 216: L.GEMM_NT_SMALL, 300: L.GEMM_NT_GENERIC}[M] if dtype == torch.bfloat16 else L.GEMM_NT_GENERIC
    assert _gemm_plan(M, N, K, dt=L.BF16 if dtype == torch.bfloat16 else L.F32, bias=1, res=1 << 12, aux=1 << 12, epi_mode=1, act=L.ACT_GELU).kernel == family
    a, w, bias = rnd(M, K, dtype=dtype, seed=21), rnd(N, K, dtype=dtype, seed=22) / K ** 0.5, rnd(N, seed=23)
    res, h = rnd(M, N, dtype=dtype, seed=24), rnd(M, N, dtype=dtype, seed=25)
    z = a.double() @ w.double().t() + bias
    assert_parity(ops.gemm_nt(a, w, bias, res=res), z + res.double(), TOL[dtype], "residual add")
    pre = torch.empty(M, N, dtype=dtype, device=DEV)
    y = ops.gemm_nt(a, w, bias, act=L.ACT_GELU, preact_out=pre, res=res)
    assert_parity(pre, z, TOL[dtype], "pre-activation side output")
    assert_parity(y, F.gelu(z) + res.double(), TOL[dtype], "GELU + residual")
    hf = h.double().clone().requires_grad_(True)
    F.gelu(hf).backward(torch.ones_like(hf))
    assert_parity(ops.gemm_nt(a, w, None, gelu_grad_of=h), (z - bias) * hf.grad, 2 * TOL[dtype], "GELU derivative epilogue")


@pytest.mark.parametrize("M,Cm", [(4096, 48), (13829, 48), (13824, 96), (4111, 96)])
def test_fused_mlp_forward_and_backward(M, Cm):
    """the one-launch MLP of the 48-channel Swin stage (hidden tile fed from the first product's accumulator into the second) and its
    backward (pre-activation recomputed; dz, h written for the weight-gradient products) against fp32 torch on the bf16-rounded operands,
    the fused statistics against a statistics pass over y, and the two-GEMM path it replaces (gemm_nt twice, called directly)."""
    ops = _ops()
    dt = torch.bfloat16
    Hm = 4 * Cm      # (round 5: the 96-channel stage too - weights resident in 155 KB of LDS, W1^T read transposed in the backward kernel)
    x, res, dy = rnd(1, M, Cm, dtype=dt, seed=81), rnd(1, M, Cm, dtype=dt, seed=82), rnd(1, M, Cm, dtype=dt, seed=83)
    w1, b1 = rnd(Hm, Cm, seed=84) / Cm ** 0.5, rnd(Hm, seed=85) / 4
    w2, b2 = rnd(Cm, Hm, seed=86) / Hm ** 0.5, rnd(Cm, seed=87) / 4
    w1b, w2b = w1.to(dt), w2.to(dt)
    assert ops.mlp_fused(x, Hm)
    ops.begin_step()
    y = ops.mlp_fwd(x, w1b, b1, w2b, b2, res=res, want_stat=True)
    stat = ops.pop_gemm_stat(y)
    z = x.double() @ w1b.double().t() + b1
    hr = F.gelu(z)
    yr = hr.to(dt).double() @ w2b.double().t() + b2 + res.double()
    assert_parity(y, yr, 5e-3, "y against float64")
    assert stat is not None and torch.allclose(stat.sum(0), ops.instnorm_stats(y, 1, M).sum(0), rtol=1e-6, atol=1e-3)
    zf = z.clone().requires_grad_(True)
    F.gelu(zf).backward(torch.ones_like(zf))
    dzr = (dy.double() @ w2b.double()) * zf.grad
    dz, h, dx = ops.mlp_bwd(x, dy, w1b, b1, w2b.t().contiguous(), w1b.t().contiguous())
    assert_parity(h, hr, 5e-3, "h against float64")
    assert_parity(dz, dzr, 5e-3, "dz against float64")
    assert_parity(dx, dz.double() @ w1b.double(), 5e-3, "dx against float64 on the stored dz")
    # the path it replaces (pre-activation rounded to bf16 before gelu'): same results within bf16 rounding
    pre = torch.empty(1, M, Hm, dtype=dt, device=DEV)
    a0 = ops.gemm_nt(x, w1b, b1, act=_L().ACT_GELU, preact_out=pre)
    y0 = ops.gemm_nt(a0, w2b, b2, res=res)
    assert_parity(y, y0, 5e-3, "y against the two-GEMM route")
    assert_parity(h, a0, 5e-3, "h against the two-GEMM route")
    assert_parity(dz, ops.gemm_nt(dy, w2b.t().contiguous(), gelu_grad_of=pre), 1e-2, "dz against the two-GEMM route")


@pytest.mark.parametrize("M,K,N,gelu,styled", [(110592, 48, 144, False, True), (13824, 96, 288, False, True), (13824, 96, 384, True, False), (4100, 48, 48, False, False),
                                               (1728, 192, 576, False, True), (1728, 192, 768, True, True), (216, 384, 1152, False, False), (216, 384, 1536, True, True)])
def test_gemm_with_the_instance_norm_folded_into_its_operand_load(M, K, N, gelu, styled):
    """round 5: y = act(norm(x) W^T + b) with the (conditional) instance norm's apply pass inside the streaming GEMM's operand load
    (miseg_gemm_params.an) - the same bits as miseg_instnorm_apply followed by the plain GEMM (same fma, same rounding), for y, for the stored
    norm(x) and for the GELU pre-activation; the Swin shapes qkv @ 48^3 / 24^3, fc1 @ 24^3 and a ragged row count."""
    ops, L = _ops(), _L()
    dt = torch.bfloat16
    plan = _gemm_plan(M, N, K, an=2 if styled else 1, act=L.ACT_GELU if gelu else L.ACT_NONE)
    assert (plan.kernel, plan.anorm, plan.gelu) == (L.GEMM_NT_STREAM if M > 2048 else L.GEMM_NT_SMALL, 1, int(gelu))
    x = (rnd(1, M, K, dtype=torch.float32, seed=91) * 1.7 + 0.4).to(dt)
    w, b = (rnd(N, K, seed=92) / K ** 0.5).to(dt), rnd(N, seed=93) / 4
    gam = [rnd(K, seed=94) * 0.2 + 1.0, rnd(K, seed=95) * 0.2 + 1.0] if styled else None
    bet = [rnd(K, seed=96) * 0.3, rnd(K, seed=97) * 0.3] if styled else None
    styles = torch.tensor([1], dtype=torch.int32, device=DEV) if styled else None
    ops.begin_step()
    stat = ops.instnorm_stats(x, 1, M)
    xn0 = ops.instnorm_apply(x, 1, M, stat, styles, gam, bet)
    pre0 = torch.empty(1, M, N, dtype=dt, device=DEV) if gelu else None
    y0 = ops.gemm_nt(xn0, w, b, act=L.ACT_GELU if gelu else L.ACT_NONE, preact_out=pre0)
    ref = ops.NormRef(stat, styles, gam, bet, 1e-5)
    assert ops.gemm_nt_folds(x, w, anorm=ref, act=L.ACT_GELU if gelu else L.ACT_NONE)
    pre1 = torch.empty(1, M, N, dtype=dt, device=DEV) if gelu else None
    y1, xn1 = ops.gemm_nt(x, w, b, act=L.ACT_GELU if gelu else L.ACT_NONE, preact_out=pre1, anorm=ref, anorm_out=True)
    assert torch.equal(xn0, xn1)
    assert torch.equal(y0, y1)
    assert not gelu or torch.equal(pre0, pre1)
    y2 = ops.gemm_nt(x, w, b, act=L.ACT_GELU if gelu else L.ACT_NONE, anorm=ref)            # without the stored copy
    assert torch.equal(y0, y2)
    # and against torch in fp32 on the same operands
    mu, var = x.double().mean(1, keepdim=True), x.double().var(1, unbiased=False, keepdim=True)
    xr = (x.double() - mu) / torch.sqrt(var + 1e-5) * (gam[1] if styled else 1.0) + (bet[1] if styled else 0.0)
    assert_parity(xn1, xr, 5e-3, "stored norm(x) against float64")


@pytest.mark.parametrize("M,K,N", [(110592, 144, 48), (13824, 288, 96), (5000, 96, 48), (1728, 576, 192), (1728, 768, 192), (216, 1152, 384), (216, 1536, 384)])
def test_gemm_with_the_norm_backward_sums_in_its_epilogue(M, K, N):
    """round 5: the data-gradient GEMM behind an instance norm leaves the norm's backward sums (sum g, sum g * xhat) in its epilogue
    (miseg_gemm_params.stat_mode 2) - against miseg_instnorm_bwd_reduce over the stored gradient, and the apply-only backward
    (miseg_instnorm_bwd_apply) against the two-launch backward incl. affine gradients and the skip-branch add.
    dx of the two routes: pooled distance <= 5.4e-6 (bar 2e-3); locally the two bf16 roundings differ by one unit in the last place at single
    elements (4.2e-3 at 110592 x 48, 1.1e-3 at 1728 x 192, 0 elsewhere).  Its local bound is max(2e-3, 2 x yardstick), the yardstick being the local
    error of the norm backward through torch's bf16 ops against the float64 one: 1.6e-2 .. 2.3e-2 on the seven shapes, so bounds of 3.2e-2 .. 4.6e-2; both routes are also held to float64 at the instance
    norm's backward bar."""
    ops = _ops()
    dt = torch.bfloat16
    plan = _gemm_plan(M, N, K, stat=1, stat_mode=2, bs_x=1 << 12)
    assert (plan.kernel, plan.stat) == (_L().GEMM_NT_STREAM if M > 2048 else _L().GEMM_NT_SMALL, 2)
    dy = rnd(1, M, K, dtype=dt, seed=101)
    wt = (rnd(N, K, seed=102) / K ** 0.5).to(dt)
    x = (rnd(1, M, N, dtype=torch.float32, seed=103) * 1.3 - 0.2).to(dt)
    gskip = rnd(1, M, N, dtype=dt, seed=104)
    gam, styles = [rnd(N, seed=105) * 0.2 + 1.0, rnd(N, seed=106) * 0.2 + 1.0], torch.tensor([0], dtype=torch.int32, device=DEV)
    ops.begin_step()
    stat = ops.instnorm_stats(x, 1, M)
    g0 = ops.gemm_nt(dy, wt)
    assert ops.gemm_nt_folds(dy, wt, bstat_x=x) == (M > 2048 or ops.SMALL_BSTAT)      # (small M: the kernel has the epilogue, the step keeps the one-launch norm backward)
    g1 = ops.gemm_nt(dy, wt, bstat=(x, stat, 1e-5))
    dstat = ops.pop_gemm_stat(g1)
    assert torch.equal(g0, g1) and dstat is not None
    want = ops.instnorm_bwd_reduce(g0, x, 1, M, stat).sum(0)                      # [1, N, 2] fp64
    got = dstat.view(-1, 1, N, 2).sum(0)
    scale = want.abs().max(dim=1, keepdim=True).values
    assert float(((got - want).abs() / scale).max()) < 2e-5, float(((got - want).abs() / scale).max())
    dg0, db0, dg1, db1 = (torch.zeros(2, N, device=DEV) for _ in range(4))
    dx0, _ = ops.instnorm_bwd(g0, None, x, 1, M, stat, styles, gam, [dg0[0], None], [db0[0], None], gadd=gskip)
    dx1 = ops.instnorm_bwd_apply(g1, x, 1, M, stat, dstat, styles, gam, [dg1[0], None], [db1[0], None], gadd=gskip)
    # float64 norm backward on the stored gradient: dx = gamma rstd (g - mean g - xhat mean(g xhat)) + skip; the yardstick is the same expression through
    # torch's bf16 ops
    def norm_bwd(dt):
        xx, gg = x.to(dt), g0.to(dt)
        mu, var = xx.mean(1, keepdim=True), xx.var(1, unbiased=False, keepdim=True)
        rstd = (var + 1e-5).rsqrt()
        xh = (xx - mu) * rstd
        return gam[0].to(dt) * rstd * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True)) + gskip.to(dt)
    dx64 = norm_bwd(torch.float64)
    bound = max(2e-3, 2 * local_err(norm_bwd(dt), dx64)[0])
    assert_parity(dx1, dx64, 3 * TOL[dt], "dx of the apply-only route against float64")
    assert_parity(dx1, dx0, 2e-3, "dx of the apply-only route against the two-launch route", local_tol=bound)      # bf16 outputs of sums that differ in their last fp32 bits
    assert_parity(dg1[0], dg0[0], 1e-4, "dgamma: apply-only route against the two-launch route")
    assert_parity(db1[0], db0[0], 1e-4, "dbeta: apply-only route against the two-launch route")
    assert float(dg1[1].abs().max()) == 0.0


@pytest.mark.parametrize("M,Cm", [(110592, 48), (13824, 96)])
def test_fused_mlp_with_the_norm_folded_in_and_its_backward_sums(M, Cm):
    """round 5: mlp_fwd with norm2 folded into its token load = instnorm_apply + mlp_fwd bit for bit (y, the stored norm(x), the fused output
    statistics); mlp_bwd's norm-backward sums against miseg_instnorm_bwd_reduce over its dx"""
    ops = _ops()
    dt, Hm = torch.bfloat16, 4 * Cm
    x, dy = (rnd(1, M, Cm, dtype=torch.float32, seed=111) * 1.5 + 0.3).to(dt), rnd(1, M, Cm, dtype=dt, seed=112)
    w1, b1 = (rnd(Hm, Cm, seed=113) / Cm ** 0.5).to(dt), rnd(Hm, seed=114) / 4
    w2, b2 = (rnd(Cm, Hm, seed=115) / Hm ** 0.5).to(dt), rnd(Cm, seed=116) / 4
    gam, bet, styles = [rnd(Cm, seed=117) * 0.2 + 1.0], [rnd(Cm, seed=118) * 0.3], None
    ops.begin_step()
    stat = ops.instnorm_stats(x, 1, M)
    xn0 = ops.instnorm_apply(x, 1, M, stat, styles, gam, bet)
    y0 = ops.mlp_fwd(xn0, w1, b1, w2, b2, res=x, want_stat=True)
    s0 = ops.pop_gemm_stat(y0)
    y1, xn1 = ops.mlp_fwd(x, w1, b1, w2, b2, res=x, want_stat=True, anorm=ops.NormRef(stat, styles, gam, bet, 1e-5), anorm_out=True)
    s1 = ops.pop_gemm_stat(y1)
    assert torch.equal(xn0, xn1) and torch.equal(y0, y1)
    assert torch.allclose(s0.sum(0), s1.sum(0), rtol=1e-6, atol=1e-3)
    w2t, w1t = w2.t().contiguous(), w1.t().contiguous()
    dz0, h0, dx0 = ops.mlp_bwd(xn0, dy, w1, b1, w2t, w1t)
    dz1, h1, dx1, dstat = ops.mlp_bwd(xn1, dy, w1, b1, w2t, w1t, bstat=(x, stat, 1e-5))
    assert torch.equal(dz0, dz1) and torch.equal(h0, h1) and torch.equal(dx0, dx1)
    want = ops.instnorm_bwd_reduce(dx0, x, 1, M, stat).sum(0)
    got = dstat.view(-1, 1, Cm, 2).sum(0)
    scale = want.abs().max(dim=1, keepdim=True).values
    assert float(((got - want).abs() / scale).max()) < 2e-5


def test_gemm_nt_exact_integers():
    """asymmetric small-integer operands: catches transposed / permuted MFMA fragment maps exactly."""
    ops = _ops()
    for dtype in (torch.float32, torch.bfloat16):
        a = (torch.arange(70 * 40, device=DEV).reshape(70, 40) % 7 - 3).to(dtype)
        w = (torch.arange(33 * 40, device=DEV).reshape(33, 40) % 5 - 2).to(dtype)
        y = ops.gemm_nt(a, w, out_dtype=None)
        assert torch.equal(y.float(), a.float() @ w.float().t())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("K,M,N", [(1000, 144, 48), (27, 768, 200), (5000, 48, 48), (333, 12, 36), (4096, 96, 384)])
def test_gemm_tn(dtype, K, M, N):
    ops = _ops()
    a, b = rnd(K, M, dtype=dtype, seed=31), rnd(K, N, dtype=dtype, seed=32)
    y = ops.gemm_tn(a, b)
    yr = a.double().t() @ b.double()
    assert_parity(y, yr, TOL[dtype], "library-chosen split")
    y1 = ops.gemm_tn(a, b, split_k=1)
    assert_parity(y1, yr, TOL[dtype], "split_k = 1")


def test_gemm_tn_exact_integers():
    ops = _ops()
    for dtype in (torch.float32, torch.bfloat16):
        a = (torch.arange(100 * 50, device=DEV).reshape(100, 50) % 7 - 3).to(dtype)
        b = (torch.arange(100 * 70, device=DEV).reshape(100, 70) % 5 - 2).to(dtype)
        y = ops.gemm_tn(a, b, split_k=1)
        assert torch.equal(y, a.float().t() @ b.float())


def _conv_case(dtype, B, D, H, W, Cin, Cout, seed=0):
    x = rnd(B, D, H, W, Cin, dtype=dtype, seed=41 + seed)
    w = rnd(Cout, Cin, 3, 3, 3, seed=42 + seed) / (27 * Cin) ** 0.5
    return x, w


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,D,H,W,Cin,Cout", [(1, 8, 8, 8, 48, 48), (2, 5, 9, 11, 12, 24), (1, 12, 16, 8, 96, 48), (1, 3, 3, 3, 192, 96),
                                             (1, 6, 6, 6, 8, 12), (1, 4, 8, 16, 48, 96), (1, 7, 7, 7, 16, 16), (2, 9, 10, 13, 32, 16), (1, 24, 24, 24, 16, 32),
                                             (1, 5, 8, 8, 32, 32),       # (the 16 / 32-channel bf16 cases take the narrow-layer weight-gradient kernel)
                                             # rows >= 256 bytes that are no multiple of 96: K side padded to the next chunk (conv3_k96),
                                             # forward on Cin, data gradient on Cout; ragged channel counts and a generic-path partner
                                             (1, 12, 12, 12, 128, 256), (1, 6, 7, 5, 256, 128), (2, 5, 6, 7, 130, 64), (1, 4, 4, 4, 200, 40),
                                             # whole 48-channel blocks on volumes that are no whole number of 4 x 8 x 8 bricks: the pipelined weight-gradient
                                             # loop with partial last bricks (round 5; remainders 4 / 1, 5, 3 / 2, 3)
                                             (1, 12, 12, 12, 192, 96), (1, 9, 13, 19, 48, 48), (2, 6, 11, 8, 96, 96)])
def test_conv3_fwd_dgrad_wgrad(dtype, B, D, H, W, Cin, Cout):
    ops = _ops()
    x, w = _conv_case(dtype, B, D, H, W, Cin, Cout)
    fwdp, bwdp = ops.pack_conv3(w, dtype)
    y = ops.conv3_fwd(x, fwdp, Cout)
    xr = x.double().permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    wr = w.double().clone().requires_grad_(True)
    wq = wr.to(dtype).double() if dtype == torch.bfloat16 else wr
    yr = F.conv3d(xr, wq, padding=1)
    assert_parity(y.permute(0, 4, 1, 2, 3), yr, TOL[dtype], "forward")
    if (dtype, B, D, H, W, Cin, Cout) == (torch.bfloat16, 1, 9, 13, 19, 48, 48):
        # the check bites on real output (a ragged brick-path case): against a reference whose corner voxel is lost, the kernel's result must fail
        lost = yr.detach().clone()
        lost[0, :, D - 1, H - 1, W - 1] = 0
        with pytest.raises(AssertionError):
            assert_parity(y.permute(0, 4, 1, 2, 3), lost, TOL[dtype], "mutated reference: corner voxel zeroed")
    dy = rnd(B, D, H, W, Cout, dtype=dtype, seed=43)
    yr.backward(dy.double().permute(0, 4, 1, 2, 3))
    dx = ops.conv3_fwd(dy, bwdp, Cin)
    assert_parity(dx.permute(0, 4, 1, 2, 3), xr.grad, TOL[dtype], "data gradient")
    dw = ops.conv3_wgrad(x, dy)
    assert_parity(dw, wr.grad, TOL[dtype], "weight gradient")
    # accumulate into an existing gradient (mode 1) and into a zeroed slot (mode 2), as the training arena asks for
    acc = torch.full_like(dw, 0.5)
    ops.conv3_wgrad(x, dy, dw=acc, accumulate=True)
    assert_parity(acc - 0.5, wr.grad, 2 * TOL[dtype], "weight gradient accumulated onto 0.5")
    z = torch.zeros_like(dw)
    ops.conv3_wgrad(x, dy, dw=z, accumulate=2)
    assert_parity(z, wr.grad, TOL[dtype], "weight gradient into a zeroed slot")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,D,H,W,Cin,Cout", [(2, 8, 8, 16, 48, 48), (1, 5, 9, 11, 96, 24), (1, 12, 8, 20, 48, 96),
                                             # chunks of 4 and of 2 k groups (64- / 32-byte rows, round 4): no padding to 96 bytes
                                             (1, 8, 8, 16, 32, 32), (2, 5, 9, 11, 16, 16), (1, 8, 12, 16, 64, 32), (1, 9, 8, 17, 16, 48)])
def test_conv3_fused_residual_and_statistics(dtype, B, D, H, W, Cin, Cout):
    """epilogue pieces of the 96-byte-chunk path: out = conv(x) + res, and the instance-norm statistics of the ROUNDED output
    (what miseg_instnorm_stats computes from the stored tensor) accumulated into the zeroed fp64 buffer.
    bf16: the two-launch `want` rounds twice, the fused epilogue once - pooled 2.4e-3 (bar 4e-3), locally one unit in the last place at single
    elements (5.8e-3 .. 5.9e-3 on all seven shapes).  Local bound of that comparison: max(tol, 2 x yardstick), the yardstick being the local error of
    `want` against float64: 4.5e-3 .. 5.6e-3 on the seven shapes, so bounds of 9.1e-3 .. 1.1e-2; the fused output is held to float64 as well."""
    ops = _ops()
    if dtype == torch.float32:
        Cin = Cin // 2          # 96-byte rows: 24 fp32 channels per chunk
    x, w = _conv_case(dtype, B, D, H, W, Cin, Cout, seed=7)
    fwdp, _ = ops.pack_conv3(w, dtype)
    res = rnd(B, D, H, W, Cout, dtype=dtype, seed=77)
    plain = ops.conv3_fwd(x, fwdp, Cout)
    ops.begin_step()
    y, stat = ops.conv3_fwd(x, fwdp, Cout, res=res, want_stat=True)
    want = (plain.float() + res.float()).to(dtype)
    # float64 on the same operands; the two-launch `want` (the stored convolution plus the residual through torch, rounded twice) is the yardstick
    wq = w.to(dtype).double() if dtype == torch.bfloat16 else w.double()
    ref64 = F.conv3d(x.double().permute(0, 4, 1, 2, 3), wq, padding=1).permute(0, 2, 3, 4, 1) + res.double()
    yard = local_err(want, ref64)[0]
    assert_parity(y, ref64, TOL[dtype], "fused conv + res against float64", local_tol=max(TOL[dtype], 2 * yard))
    tol2 = 1e-6 if dtype == torch.float32 else 4e-3
    assert_parity(y.float(), want.float(), tol2, "fused conv + res against the two-launch route", local_tol=max(tol2, 2 * yard))
    if stat is None:        # split reduction on this shape: the caller's norm computes the statistics itself
        return
    s = stat.sum(0)         # [B, Cout, 2]
    yf = y.double().reshape(B, -1, Cout)
    assert torch.allclose(s[..., 0], yf.sum(1), rtol=1e-5, atol=1e-3)
    assert torch.allclose(s[..., 1], (yf * yf).sum(1), rtol=1e-5, atol=1e-3)
    ref = ops.instnorm_stats(y, B, D * H * W).sum(0)
    assert torch.allclose(s, ref, rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("B,D,H,W,Cin,Cout,Csc,with_res", [(1, 16, 16, 32, 48, 96, 48, False), (1, 9, 7, 17, 48, 96, 48, True), (1, 32, 32, 32, 96, 48, 96, False),
                                                          (1, 16, 16, 16, 48, 40, 48, False)])
def test_conv3_takes_a_1x1x1_shortcut_term_along(B, D, H, W, Cin, Cout, Csc, with_res):
    """round 5 (miseg_conv3_params.sc_x): y = conv3x3x3(x) + g W^T [+ res] in one launch - the data-gradient pass of a residual block's first
    convolution with the gradient of the block's 1x1x1 shortcut (dynunet_block.py:100-126) - against the two-launch route (GEMM, then the
    convolution with the fused residual): the same bf16 rounding points except that the shortcut term joins in fp32."""
    ops = _ops()
    dtype = torch.bfloat16
    x, w = _conv_case(dtype, B, D, H, W, Cin, Cout, seed=21)
    fwdp, _ = ops.pack_conv3(w, dtype)
    g = rnd(B, D, H, W, Csc, dtype=dtype, seed=22)
    ws = (rnd(Cout, Csc, seed=23) / Csc ** 0.5).to(dtype)
    res = rnd(B, D, H, W, Cout, dtype=dtype, seed=24) if with_res else None
    assert ops.conv3_fuses_shortcut(x, Cout, Csc)
    assert not ops.conv3_fuses_shortcut(x.float(), Cout, Csc) and not ops.conv3_fuses_shortcut(x, Cout, 40)
    assert ops.conv3_fuses_shortcut(x, Cout, g, ws)      # (asked with the operands themselves)
    y = ops.conv3_fwd(x, fwdp, Cout, res=res, sc=(g, ws))
    ref = F.conv3d(x.double().permute(0, 4, 1, 2, 3), w.to(dtype).double(), padding=1).permute(0, 2, 3, 4, 1) + g.double() @ ws.double().t()
    if with_res:
        ref = ref + res.double()
    assert_parity(y.float(), ref, TOL[dtype], "conv + shortcut term")
    # against the unfused route
    y2 = ops.conv3_fwd(x, fwdp, Cout, res=ops.gemm_nt(g, ws) if res is None else ops.add(ops.gemm_nt(g, ws), res))
    assert_parity(y.float(), y2.float(), 2 * TOL[dtype], "fused against the two-launch route")
    # a strided shortcut operand (a channel slice of a wider buffer)
    gw = rnd(B, D, H, W, Csc + 16, dtype=dtype, seed=25)
    y3 = ops.conv3_fwd(x, fwdp, Cout, sc=(gw[..., 16:], ws))
    ref3 = F.conv3d(x.double().permute(0, 4, 1, 2, 3), w.to(dtype).double(), padding=1).permute(0, 2, 3, 4, 1) + gw[..., 16:].double() @ ws.double().t()
    assert_parity(y3.float(), ref3, TOL[dtype], "1x1x1 output")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,D,H,W,Cin,Cout,Cl", [(1, 16, 16, 32, 48, 96, 48), (2, 8, 12, 34, 48, 96, 48), (1, 16, 32, 32, 96, 64, 16)])
def test_conv3_stores_its_left_channels_in_space_to_channel_order(dtype, B, D, H, W, Cin, Cout, Cl):
    """round 5 (miseg_conv3_params.s2c_out): the first Cl output channels leave the kernel as [.., D/2, H/2, W/2, 8, Cl] (what the transposed
    convolution in front of a decoder block reads as the gradient of its output), the others as usual - bit-identical to the plain launch
    followed by the gather pass."""
    ops = _ops()
    from mi_seg_amd.hip.functional import STD_OFFSETS
    if dtype == torch.float32:
        Cin = Cin // 2
    x, w = _conv_case(dtype, B, D, H, W, Cin, Cout, seed=31)
    fwdp, _ = ops.pack_conv3(w, dtype)
    if not ops.conv3_fuses_s2c(x, Cout, Cl):
        pytest.skip("this shape takes an output-channel tile that does not divide the left part")
    plain = ops.conv3_fwd(x, fwdp, Cout)
    want8 = ops.space_to_channel(plain[..., :Cl], STD_OFFSETS)
    y8 = torch.full((B, D // 2, H // 2, W // 2, 8 * Cl), 7.0, dtype=dtype, device=DEV)
    y = torch.full((B, D, H, W, Cout), 5.0, dtype=dtype, device=DEV)
    ops.conv3_fwd(x, fwdp, Cout, out=y, s2c=y8)
    assert torch.equal(y8, want8)
    assert torch.equal(y[..., Cl:], plain[..., Cl:])
    assert bool((y[..., :Cl] == 5.0).all()), "the left channels of the ordinary output must stay untouched"
    assert not ops.conv3_fuses_s2c(rnd(1, 15, 16, 32, Cin, dtype=dtype, seed=1), Cout, Cl)      # odd extent


@pytest.mark.parametrize("B,D,H,W,Cin,Cout", [(1, 32, 32, 64, 96, 48), (1, 33, 31, 65, 96, 48), (1, 16, 16, 16, 48, 96)])
def test_conv3_with_the_shortcut_convolution_as_a_second_output(B, D, H, W, Cin, Cout):
    """round 5 (miseg_conv3_params.fs_w): y = conv3x3x3(x, w1) and y3 = conv1x1x1(x, w3) from ONE launch, each with its instance-norm statistics -
    against the 3x3x3 launch and the GEMM it replaces (bit-identical first output; second output within bf16 rounding of the GEMM's)."""
    ops = _ops()
    dtype = torch.bfloat16
    x, w = _conv_case(dtype, B, D, H, W, Cin, Cout, seed=41)
    fwdp, _ = ops.pack_conv3(w, dtype)
    w3 = (rnd(Cout, Cin, seed=42) / Cin ** 0.5).to(dtype)
    assert ops.conv3_fuses_fwd_shortcut(x, Cout)
    ops.begin_step()
    y0, st0 = ops.conv3_fwd(x, fwdp, Cout, want_stat=True)
    y, st, y3, st3 = ops.conv3_fwd(x, fwdp, Cout, want_stat=True, fs=(w3, True))
    assert torch.equal(y, y0) and torch.allclose(st.sum(0), st0.sum(0), rtol=1e-9, atol=1e-6)
    ref3 = x.double() @ w3.double().t()
    assert_parity(y3.float(), ref3, TOL[dtype], "1x1x1 output")
    assert_parity(y3.float(), ops.gemm_nt(x, w3).float(), TOL[dtype], "second output against the GEMM")
    assert torch.allclose(st3.sum(0), ops.instnorm_stats(y3, B, D * H * W).sum(0), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("B,S,Cin,Cout", [(1, 3, 768, 768), (2, 3, 96, 96), (1, 6, 384, 768), (2, 6, 96, 48), (1, 6, 144, 40)])
def test_conv3_tiny_volume_weight_streaming_kernel(B, S, Cin, Cout):
    """round 5 (conv3_fwd_tiny_kernel): 3^3 / 6^3 volumes whose every 48-channel chunk is a split of its own - a wave streams the pack's
    fragments for its 16 output channels straight into the matrix pipe, the chunk's volume sits zero-bordered in LDS; same slabs, same second
    launch as the brick kernel.  Against F.conv3d on the bf16-rounded operands, forward and data gradient."""
    ops = _ops()
    dtype = torch.bfloat16
    x, w = _conv_case(dtype, B, S, S, S, Cin, Cout, seed=61)
    assert ops.conv3_fwd_plan(x, Cout).kernel == ops.L.CONV3_FWD_TINY
    fwdp, bwdp = ops.pack_conv3(w, dtype)
    y = ops.conv3_fwd(x, fwdp, Cout)
    wq = w.to(dtype).double()
    ref = F.conv3d(x.double().permute(0, 4, 1, 2, 3), wq, padding=1)
    assert_parity(y.permute(0, 4, 1, 2, 3), ref, TOL[dtype], "forward")
    dy = rnd(B, S, S, S, Cout, dtype=dtype, seed=62)
    dx = ops.conv3_fwd(dy, bwdp, Cin)
    refx = torch.nn.grad.conv3d_input((B, Cin, S, S, S), wq, dy.double().permute(0, 4, 1, 2, 3), padding=1)
    assert_parity(dx.permute(0, 4, 1, 2, 3), refx, TOL[dtype], "data gradient")
    # with the statistics and a residual behind the slab sum
    res = rnd(B, S, S, S, Cout, dtype=dtype, seed=63)
    ops.begin_step()
    y2, st = ops.conv3_fwd(x, fwdp, Cout, res=res, want_stat=True)
    assert_parity(y2.float(), (ref.permute(0, 2, 3, 4, 1) + res.double()), TOL[dtype], "with residual")
    if st is not None:
        assert torch.allclose(st.sum(0), ops.instnorm_stats(y2, B, S ** 3).sum(0), rtol=1e-5, atol=1e-3)


def test_conv3_shortcut_is_refused_where_the_launch_splits():
    ops = _ops()
    x = rnd(1, 6, 6, 6, 384, dtype=torch.bfloat16, seed=3)
    assert not ops.conv3_fuses_shortcut(x, 768, 384)        # 6^3: the reduction is split over workgroups (fp32 slabs + a second launch)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,D,H,W,Cin,Cout,with_res", [(1, 12, 12, 12, 192, 192, True), (2, 6, 6, 6, 96, 48, False), (1, 3, 3, 3, 768, 768, True), (2, 5, 7, 6, 96, 96, True),
                                                      (1, 12, 12, 12, 128, 128, True), (1, 6, 6, 6, 256, 128, False)])      # 64-byte chunks (C-UNETR's deep layers)
def test_split_conv_leaves_its_slabs_to_the_instance_norm(dtype, B, D, H, W, Cin, Cout, with_res):
    """conv -> (conditional) instance norm -> + residual -> LeakyReLU at the small stages (dynunet_block.py:100-126): a split convolution
    asked with want_stat="defer" stops after its fp32 partial slabs and the norm's ONE launch sums them, writes the convolution's output
    (the backward pass reads it), and normalises (miseg_instnorm_fwd_slabs).  Against the two-step route: bit-identical convolution output,
    the same statistics and result."""
    ops = _ops()
    from mi_seg_amd.hip import lib as hiplib
    if dtype == torch.float32:
        Cin = Cin // 2
    x, w = _conv_case(dtype, B, D, H, W, Cin, Cout, seed=11)
    fwdp, _ = ops.pack_conv3(w, dtype)
    S = D * H * W
    styles = torch.tensor([1, 0][:B], dtype=torch.int32, device=DEV)
    gam = [rnd(Cout, seed=21 + i) * 0.2 + 1.0 for i in range(2)]
    bet = [rnd(Cout, seed=31 + i) * 0.2 for i in range(2)]
    res = rnd(B, D, H, W, Cout, dtype=dtype, seed=41) if with_res else None
    ops.begin_step()
    y0, st0 = ops.conv3_fwd(x, fwdp, Cout, want_stat=True)
    if st0 is None:
        st0 = ops.instnorm_stats(y0, B, S)
    out0 = ops.instnorm_apply(y0, B, S, st0, styles, gam, bet, res=res, act=hiplib.ACT_LEAKY, slope=0.01)
    y1, pend = ops.conv3_fwd(x, fwdp, Cout, want_stat="defer")
    assert isinstance(pend, ops.PendingSlabs), "these shapes split their reduction and have <= 2048 rows per sample"
    out1, st1 = ops.instnorm_fwd_slabs(y1, pend, B, S, styles, gam, bet, res=res, act=hiplib.ACT_LEAKY, slope=0.01)
    assert torch.equal(y1, y0)
    assert torch.allclose(st1.sum(0), st0.sum(0), rtol=1e-4, atol=1e-3)      # (the one-launch form sums a lane's rows in fp32 before the fp64 totals)
    assert_parity(out1.float(), out0.float(), (1e-6 if dtype == torch.float32 else 4e-3), "norm output behind the slab sum")
    # the same in the backward direction: the data-gradient convolution (mirrored pack, Cout -> Cin) in front of the norm's backward pass
    # leaves its slabs to miseg_instnorm_bwd_slabs - the incoming gradient is never written
    _, bwdp = ops.pack_conv3(w, dtype)
    g2 = rnd(B, D, H, W, Cout, dtype=dtype, seed=51)
    xin = rnd(B, D, H, W, Cin, dtype=dtype, seed=52)          # the norm's input (Cin channels), its statistics and affine rows
    gam_i = [rnd(Cin, seed=61 + i) * 0.2 + 1.0 for i in range(2)]
    bet_i = [rnd(Cin, seed=71 + i) * 0.2 for i in range(2)]
    st_in = ops.instnorm_stats(xin, B, S)
    def grads():
        return [torch.zeros(Cin, device=DEV) for _ in range(2)], [torch.zeros(Cin, device=DEV) for _ in range(2)]
    dy0 = ops.conv3_fwd(g2, bwdp, Cin)
    dg0, db0 = grads()
    dx0, _ = ops.instnorm_bwd(dy0, None, xin, B, S, st_in, styles, gam_i, dg0, db0, act=hiplib.ACT_LEAKY, slope=0.01, betas=bet_i)
    dy1, pend = ops.conv3_fwd(g2, bwdp, Cin, defer=True)
    assert isinstance(pend, ops.PendingSlabs) == (Cout * g2.element_size() > 96), "one 96-byte chunk on the K side: nothing to split"
    if pend is None:
        assert torch.equal(dy1, dy0)
    dg1, db1 = grads()
    dx1, _ = ops.instnorm_bwd(dy1, None, xin, B, S, st_in, styles, gam_i, dg1, db1, act=hiplib.ACT_LEAKY, slope=0.01, betas=bet_i, pending=pend)
    assert_parity(dx1.float(), dx0.float(), (1e-6 if dtype == torch.float32 else 4e-3), "norm backward behind the slab sum")
    for a_, b_ in zip(dg1 + db1, dg0 + db0):
        if float(b_.abs().max()) != 0.0:
            assert_parity(a_, b_, 1e-4, "affine gradients behind the slab sum")
    # a volume above the fused norm's row limit or an unsplit launch keeps the two-step route
    xb, wb = _conv_case(dtype, 1, 16, 16, 16, 48 if dtype == torch.bfloat16 else 24, 48, seed=12)
    fb, _ = ops.pack_conv3(wb, dtype)
    _, stb = ops.conv3_fwd(xb, fb, 48, want_stat="defer")
    assert not isinstance(stb, ops.PendingSlabs)


def test_conv3_exact_integers():
    ops = _ops()
    for dtype in (torch.float32, torch.bfloat16):
        x = (torch.arange(1 * 5 * 6 * 9 * 16, device=DEV).reshape(1, 5, 6, 9, 16) % 5 - 2).to(dtype)
        w = (torch.arange(32 * 16 * 27, device=DEV).reshape(32, 16, 3, 3, 3) % 3 - 1).float()
        fwdp, _ = ops.pack_conv3(w, dtype)
        y = ops.conv3_fwd(x, fwdp, 32)
        yr = F.conv3d(x.float().permute(0, 4, 1, 2, 3), w, padding=1).permute(0, 2, 3, 4, 1)
        assert torch.equal(y.float(), yr)
        dy = (torch.arange(1 * 5 * 6 * 9 * 32, device=DEV).reshape(1, 5, 6, 9, 32) % 3 - 1).to(dtype)
        dw = ops.conv3_wgrad(x, dy)
        xr = x.float().permute(0, 4, 1, 2, 3)
        dwr = torch.nn.grad.conv3d_weight(xr, w.shape, dy.float().permute(0, 4, 1, 2, 3), padding=1)
        assert torch.equal(dw, dwr)


@pytest.mark.parametrize("B,S,Cin,Cout", [(1, 3, 768, 768), (2, 3, 48, 96), (1, 6, 768, 384), (2, 6, 32, 48), (1, 6, 384, 384), (3, 3, 16, 48)])
def test_conv3_wgrad_tiny_volumes(B, S, Cin, Cout):
    """the write-bound weight-gradient kernel of the 3^3 / 6^3 layers (encoder10 / decoder5: dynunet_block.py:100-126 at 1/32 resolution;
    csrc/conv3d.hip::conv3_wgrad_tiny_kernel, taps on the N side of the matrix product) against torch's conv3d_weight on the bf16-rounded
    operands: plain, accumulate, and "slot holds zeros" modes; batches > 1 (the k dimension continues over the samples)."""
    ops = _ops()
    dtype = torch.bfloat16
    x = rnd(B, S, S, S, Cin, dtype=dtype, seed=301)
    dy = rnd(B, S, S, S, Cout, dtype=dtype, seed=302)
    assert ops.conv3_wgrad_plan(x, dy).kernel == ops.L.CONV3_WGRAD_TINY
    ref = torch.nn.grad.conv3d_weight(x.double().permute(0, 4, 1, 2, 3), (Cout, Cin, 3, 3, 3), dy.double().permute(0, 4, 1, 2, 3), padding=1)
    dw = ops.conv3_wgrad(x, dy)
    assert_parity(dw, ref, 1e-5, "weight gradient")      # exact products of bf16 operands, fp32 sums: only the summation order differs
    base = rnd(Cout, Cin, 3, 3, 3, seed=303)
    acc = base.clone()
    ops.conv3_wgrad(x, dy, dw=acc, accumulate=True)
    assert_parity(acc - base, ref, 1e-4, "weight gradient accumulated")
    z = torch.zeros_like(dw)
    ops.conv3_wgrad(x, dy, dw=z, accumulate=2)
    assert torch.equal(z, dw)
    # strided operands (channel slices of wider buffers, as the concat buffers of the decoders hand them out)
    xw = rnd(B, S, S, S, Cin + 16, dtype=dtype, seed=304)
    dyw = rnd(B, S, S, S, Cout + 8, dtype=dtype, seed=305)
    xs, dys = xw[..., 16:], dyw[..., 8:]
    ref2 = torch.nn.grad.conv3d_weight(xs.double().permute(0, 4, 1, 2, 3), (Cout, Cin, 3, 3, 3), dys.double().permute(0, 4, 1, 2, 3), padding=1)
    assert_parity(ops.conv3_wgrad(xs, dys), ref2, 1e-5, "weight gradient of strided operands")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gemm_tn_grouped_launch_with_both_tile_forms(dtype):
    """the queued small weight-gradient GEMMs of a step in one grouped call (miseg_gemm_tn_group): every problem runs in 64 x 64 tiles, the only
    tile gemm_tn_group_kernel has, here from 2 x 2 (100 x 72) to 36 x 12 (2304 x 768) workgroups, none with a split reduction (K <= 2048);
    accumulate modes 1 (add to what the slot holds) and 2 (the slot is known to hold zeros: the tiles are stored).  The launch forms, the
    split path and the operand layouts have their rows in tests/test_hip_step_end_forms.py."""
    ops = _ops()
    shapes = [(216, 768, 3072), (216, 2304, 768), (1728, 192, 768), (216, 384, 1536), (27, 768, 3072), (216, 768, 768), (300, 640, 512), (216, 100, 72)]
    for mode in (1, 2):
        ops.DEFAULT_QUEUES = ops.StepQueues()
        try:
            cases = []
            for i, (K, M, N) in enumerate(shapes):
                a, b = rnd(K, M, dtype=dtype, seed=200 + i), rnd(K, N, dtype=dtype, seed=300 + i)
                out = torch.full((M, N), 0.25, device=DEV) if mode == 1 else torch.zeros(M, N, device=DEV)
                ops.gemm_tn(a, b, out=out, accumulate=mode)
                cases.append((a, b, out))
            assert len(ops.DEFAULT_QUEUES.gemm_tn) == len(shapes)
            ops.DEFAULT_QUEUES.flush()
        finally:
            ops.DEFAULT_QUEUES = None
        for a, b, out in cases:
            ref = a.double().t() @ b.double()
            assert_parity(out - (0.25 if mode == 1 else 0.0), ref, (1e-5 if dtype == torch.float32 else 2e-5), f"grouped TN product, mode {mode}, a {tuple(a.shape)}, b {tuple(b.shape)}")


@pytest.mark.parametrize("K,M,N", [(110592, 144, 48), (13824, 96, 384), (5000, 48, 96), (4096, 96, 40)])
def test_gemm_tn_with_the_bias_gradient_in_its_launch(K, M, N):
    """round 5 (miseg_gemm_params.tn_colsum): dW = dy^T x of a linear layer carries db = column sums of dy where the product takes the
    streaming path (whole 48-blocks, >= 2048 tokens); elsewhere ops.gemm_tn falls back to the column-sum kernel.  Accumulating into slots
    of a step queue, as the training arena asks for."""
    ops = _ops()
    dy = rnd(K, M, dtype=torch.bfloat16, seed=11)
    x = rnd(K, N, dtype=torch.bfloat16, seed=12)
    ops.DEFAULT_QUEUES = ops.StepQueues()
    try:
        dw = torch.full((M, N), 0.25, device=DEV)
        db = torch.full((M,), 0.5, device=DEV)
        ops.gemm_tn(dy, x, out=dw, accumulate=True, colsum_out=db)
        p = ops.L.Gemm(ops._ptr(dy), M, ops._ptr(x), N, ops._ptr(dw), N, M, N, K, 1, 1, ops.L.BF16, ops.L.F32, None, ops.L.ACT_NONE, 1, 0, None, None, 0, None, 0, 0, 0)
        fused = bool(ops.L.load().miseg_gemm_tn_fuses_colsum(ops.C.byref(p)))
        assert (_gemm_plan(M, N, K, tn=1, accumulate=1).kernel == ops.L.GEMM_TN_STREAM) == fused
        assert fused == (M % 48 == 0 and N % 48 == 0 and K >= 2048)
        assert len(ops.DEFAULT_QUEUES.colsum) == (0 if fused else 1)
        ops.DEFAULT_QUEUES.flush()
    finally:
        ops.DEFAULT_QUEUES = None
    ref_w = dy.double().t() @ x.double()
    ref_b = dy.double().sum(0)
    assert_parity(dw - 0.25, ref_w, 1e-5, "dW with the bias gradient in its launch")
    assert_parity(db - 0.5, ref_b, 1e-5, "bias gradient")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv3_wgrad_grouped(dtype):
    """the queued weight gradients of a backward pass: one grouped launch (direct epilogue for single-split layers, slabs +
    grouped partial sums for the others) must accumulate exactly what the per-layer launches give, on top of what dw held."""
    ops = _ops()
    shapes = [(1, 3, 3, 3, 96, 96), (1, 6, 6, 6, 48, 96), (2, 12, 12, 12, 48, 48), (1, 24, 24, 24, 96, 48), (1, 5, 9, 11, 12, 24),
              (1, 3, 3, 3, 40, 72), (1, 16, 40, 24, 48, 48), (1, 9, 13, 19, 48, 96)]
    cases = []
    for i, (B, D, H, W, Cin, Cout) in enumerate(shapes):
        x = rnd(B, D, H, W, Cin, dtype=dtype, seed=70 + i)
        dy = rnd(B, D, H, W, Cout, dtype=dtype, seed=90 + i)
        base = rnd(Cout, Cin, 3, 3, 3, seed=110 + i)
        cases.append((x, dy, base))
    ops.DEFAULT_QUEUES = ops.StepQueues()
    try:
        outs = []
        for x, dy, base in cases:
            dw = base.clone()
            assert ops.conv3_wgrad(x, dy, dw=dw, accumulate=True) is dw
            outs.append(dw)
        # (tiny volumes with whole channel blocks - bf16 (1, 3, 3, 3, 96, 96) and (1, 6, 6, 6, 48, 96) - take the write-bound kernel of their own right away)
        tiny = [ops.conv3_wgrad_plan(x, dy).kernel == ops.L.CONV3_WGRAD_TINY for x, dy, _ in cases]
        assert len(ops.DEFAULT_QUEUES.conv_wgrad) == len(cases) - sum(tiny) and sum(tiny) == (2 if dtype == torch.bfloat16 else 0)
        assert all(torch.equal(o, c[2]) for o, c, t in zip(outs, cases, tiny) if not t), "queued launches must not have run yet"
        ops.DEFAULT_QUEUES.flush()
        assert not ops.DEFAULT_QUEUES.conv_wgrad
    finally:
        ops.DEFAULT_QUEUES = None
    for (x, dy, base), dw in zip(cases, outs):
        ref = torch.nn.grad.conv3d_weight(x.double().permute(0, 4, 1, 2, 3), base.shape, dy.double().permute(0, 4, 1, 2, 3), padding=1)
        assert_parity(dw - base, ref, TOL[dtype], f"grouped weight gradient against float64, x {tuple(x.shape)}")
        single = ops.conv3_wgrad(x, dy)
        assert_parity(dw - base, single, (1e-5 if dtype == torch.float32 else 1e-3), f"grouped against the single launch, x {tuple(x.shape)}")
    # accumulate mode 2: "dw holds zeros" (a fresh arena slot) - stores instead of read-modify-write, no fill for the slab layers
    ops.DEFAULT_QUEUES = ops.StepQueues()
    try:
        zs = [torch.zeros_like(c[2]) for c in cases]
        for (x, dy, _), z in zip(cases, zs):
            ops.conv3_wgrad(x, dy, dw=z, accumulate=2)
        ops.DEFAULT_QUEUES.flush()
    finally:
        ops.DEFAULT_QUEUES = None
    for (x, dy, base), dw, z in zip(cases, outs, zs):
        assert_parity(z, dw - base, (1e-5 if dtype == torch.float32 else 1e-3), f"zeroed-slot mode against accumulate mode, x {tuple(x.shape)}")
        z2 = torch.zeros_like(z)
        ops.conv3_wgrad(x, dy, dw=z2, accumulate=2)
        assert_parity(z2, z, (1e-5 if dtype == torch.float32 else 1e-3), f"zeroed-slot mode: grouped against single, x {tuple(x.shape)}")


def test_fill32_ranges():
    """round 5: up to 16 (offset, length) word ranges of one buffer in one launch (the gradient arena minus the slots a kernel overwrites whole)"""
    ops = _ops()
    n = 1 << 20
    t = torch.full((n,), 7.0, device=DEV)
    ranges = [(0, 4096), (8192, 12), (8208, 3), (100000, 65537), (n - 8, 8)] + [(200000 + 64 * i, 5 + i) for i in range(20)]
    ops.fill32_ranges(t, ranges)
    want = torch.full((n,), 7.0)
    for o, l in ranges:
        want[o:o + l] = 0.0
    assert torch.equal(t.cpu(), want)
    with pytest.raises(ValueError):
        ops.fill32_ranges(t, [(2, 8)])            # offsets are multiples of 4 words


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("K,Cin,Cout", [(27, 768, 384), (216, 384, 192), (1728, 192, 96), (13824, 96, 48), (110592, 48, 48)])
def test_gemm_tn_with_the_transposed_conv_regrouping_in_its_store(dtype, K, Cin, Cout):
    """round 5: dW[ci][co][j] of a ConvTranspose3d(k2, s2) = x^T dy8 with the product's column (j, co) stored at (co, j) by the grouped
    launch / the batched partial-tile sum (miseg_gemm_tn_desc.regroup, miseg_tn_reduce_desc.regroup) - against gemm_tn + permute3, the
    two-launch form with its [(j, co)][ci] intermediate; both the accumulate-onto-existing and the known-zero slot"""
    ops = _ops()
    x, dy8 = rnd(K, Cin, dtype=dtype, seed=61), rnd(K, 8 * Cout, dtype=dtype, seed=62)
    dwf = ops.gemm_tn(dy8, x)                                                          # [(j, co)][ci]
    want = torch.zeros(Cin, Cout, 8, device=DEV)
    ops.permute3(dwf, want, (Cin, Cout, 8), (1, Cin, Cout * Cin))
    assert_parity(want, (x.double().t() @ dy8.double()).view(Cin, 8, Cout).transpose(1, 2), TOL[dtype], "gemm_tn + permute3 against float64")
    base = rnd(Cin, Cout, 8, seed=63)
    for mode, start in ((2, torch.zeros_like(base)), (1, base.clone())):
        out = start.clone()
        ops.DEFAULT_QUEUES = ops.StepQueues()
        try:
            if dtype == torch.float32 and K >= 2048 and Cin % 48 == 0:
                pass      # (fp32 takes the grouped launch at every size)
            assert ops.gemm_tn_regroups(x, dy8, out)
            ops.gemm_tn(x, dy8, out=out.view(Cin, 8 * Cout), accumulate=mode, regroup=Cout)
            ops.DEFAULT_QUEUES.flush()
        finally:
            ops.DEFAULT_QUEUES = None
        assert_parity(out - (start if mode == 1 else 0), want, (1e-5 if dtype == torch.float32 else 2e-3), f"regrouped store, mode {mode}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv3_thin_and_head_and_patch_embed(dtype):
    ops = _ops()
    x = rnd(2, 1, 9, 10, 12, seed=51)
    w = rnd(24, 1, 3, 3, 3, seed=52) / 5
    y = ops.conv3_thin_fwd(x, w, dtype)
    yr = F.conv3d(x.double(), w.double(), padding=1)
    assert_parity(y.permute(0, 4, 1, 2, 3), yr, TOL[dtype], "thin fwd 1 -> 24")
    dy = rnd(2, 9, 10, 12, 24, dtype=dtype, seed=53)
    dw = ops.conv3_thin_wgrad(x, dy, torch.zeros_like(w))
    dwr = torch.nn.grad.conv3d_weight(x.double(), w.shape, dy.double().permute(0, 4, 1, 2, 3), padding=1)
    assert_parity(dw, dwr, TOL[dtype], "thin wgrad 1 -> 24")
    # two image channels / 20 output channels: the generic thin kernels (the one-channel case above runs the brick kernels)
    x2, w2 = rnd(1, 2, 6, 9, 17, seed=57), rnd(20, 2, 3, 3, 3, seed=58) / 7
    assert_parity(ops.conv3_thin_fwd(x2, w2, dtype).permute(0, 4, 1, 2, 3), F.conv3d(x2.double(), w2.double(), padding=1), TOL[dtype], "thin fwd 2 -> 20")
    dy2 = rnd(1, 6, 9, 17, 20, dtype=dtype, seed=59)
    assert_parity(ops.conv3_thin_wgrad(x2, dy2, torch.zeros_like(w2)),
                  torch.nn.grad.conv3d_weight(x2.double(), w2.shape, dy2.double().permute(0, 4, 1, 2, 3), padding=1), TOL[dtype], "thin wgrad 2 -> 20")
    # 48 output channels on a volume with whole bricks (the headline stem) and accumulation on top of existing values
    x3, w3 = rnd(1, 1, 8, 8, 32, seed=60), rnd(48, 1, 3, 3, 3, seed=61) / 5
    assert_parity(ops.conv3_thin_fwd(x3, w3, dtype).permute(0, 4, 1, 2, 3), F.conv3d(x3.double(), w3.double(), padding=1), TOL[dtype], "stem fwd 1 -> 48")
    dy3, base = rnd(1, 8, 8, 32, 48, dtype=dtype, seed=62), rnd(48, 1, 3, 3, 3, seed=63)
    got = ops.conv3_thin_wgrad(x3, dy3, base.clone()) - base
    assert_parity(got, torch.nn.grad.conv3d_weight(x3.double(), w3.shape, dy3.double().permute(0, 4, 1, 2, 3), padding=1), TOL[dtype], "stem wgrad 1 -> 48")
    # enough bricks for the partial-sum path of the matrix-core form (per-workgroup sums + a reduce launch instead of atomics); ragged volume
    x4, dy4 = rnd(1, 1, 18, 15, 33, seed=70), rnd(1, 18, 15, 33, 48, dtype=dtype, seed=71)
    got4 = ops.conv3_thin_wgrad(x4, dy4, base.clone()) - base
    assert_parity(got4, torch.nn.grad.conv3d_weight(x4.double(), w3.shape, dy4.double().permute(0, 4, 1, 2, 3), padding=1), TOL[dtype], "stem wgrad, partial sums")
    # head
    xh = rnd(2, 5, 6, 7, 48, dtype=dtype, seed=54)
    wh, bh = rnd(6, 48, 1, 1, 1, seed=55) / 7, rnd(6, seed=56)
    lo = ops.head_fwd(xh, wh, bh)
    lor = F.conv3d(xh.double().permute(0, 4, 1, 2, 3), wh.double(), bh.double())
    assert_parity(lo, lor, TOL[dtype], "head fwd")
    g = rnd(2, 6, 5, 6, 7, seed=57)
    dwh, dbh = torch.zeros_like(wh), torch.zeros_like(bh)
    dxh = ops.head_bwd(xh, g, wh, dwh, dbh)
    assert_parity(dxh.permute(0, 4, 1, 2, 3), torch.nn.grad.conv3d_input(lor.shape[:1] + (48,) + lor.shape[2:], wh.double(), g.double()), TOL[dtype], "head dx")
    assert_parity(dwh, torch.nn.grad.conv3d_weight(xh.double().permute(0, 4, 1, 2, 3), wh.shape, g.double()), TOL[dtype], "head dw")
    assert_parity(dbh, g.double().sum((0, 2, 3, 4)), 1e-4, "head dbias")
    # 512 voxels per sample (whole 256-row tiles): the bf16 weight gradient runs on the matrix cores; accumulates on top of dw / dbias
    xh2, g2 = rnd(2, 8, 8, 8, 48, dtype=dtype, seed=64), rnd(2, 6, 8, 8, 8, seed=65)
    dw2, db2 = wh.clone(), bh.clone()
    dx2 = ops.head_bwd(xh2, g2, wh, dw2, db2)      # (bf16 data gradient: the tile kernel - dy staged per 256 voxels, weights in registers)
    assert_parity(dx2.permute(0, 4, 1, 2, 3), torch.nn.grad.conv3d_input((2, 48, 8, 8, 8), wh.double(), g2.double()), TOL[dtype], "head dx, tile kernel")
    assert_parity(dw2 - wh, torch.nn.grad.conv3d_weight(xh2.double().permute(0, 4, 1, 2, 3), wh.shape, g2.double()), TOL[dtype], "head dw, accumulated")
    assert_parity(db2 - bh, g2.double().sum((0, 2, 3, 4)), 1e-4, "head dbias, accumulated")
    # patch embed
    xp = rnd(2, 1, 8, 10, 12, seed=58)
    wp, bp = rnd(24, 1, 2, 2, 2, seed=59) / 3, rnd(24, seed=60)
    yp = ops.patch_embed_fwd(xp, wp, bp, dtype)
    ypr = F.conv3d(xp.double(), wp.double(), bp.double(), stride=2)
    assert_parity(yp.permute(0, 4, 1, 2, 3), ypr, TOL[dtype], "patch embed fwd")
    gp = rnd(2, 4, 5, 6, 24, dtype=dtype, seed=61)
    dwp, dbp = torch.zeros_like(wp), torch.zeros_like(bp)
    ops.patch_embed_bwd(xp, gp, dwp, dbp)
    assert_parity(dwp, torch.nn.grad.conv3d_weight(xp.double(), wp.shape, gp.double().permute(0, 4, 1, 2, 3), stride=2), TOL[dtype], "patch embed dw")
    assert_parity(dbp, gp.double().sum((0, 1, 2, 3)), TOL[dtype], "patch embed dbias")
    # enough coarse voxels for the partial-sum path (per-workgroup sums + a reduce launch instead of atomics), on top of existing values
    xq, wq = rnd(1, 1, 44, 40, 36, seed=65), rnd(48, 1, 2, 2, 2, seed=66) / 3
    gq = rnd(1, 22, 20, 18, 48, dtype=dtype, seed=67)
    base_w, base_b = rnd(48, 1, 2, 2, 2, seed=68), rnd(48, seed=69)
    dwq, dbq = base_w.clone(), base_b.clone()
    ops.patch_embed_bwd(xq, gq, dwq, dbq)
    assert_parity(dwq - base_w, torch.nn.grad.conv3d_weight(xq.double(), wq.shape, gq.double().permute(0, 4, 1, 2, 3), stride=2), TOL[dtype], "patch embed dw, partial sums")
    assert_parity(dbq - base_b, gq.double().sum((0, 1, 2, 3)), TOL[dtype], "patch embed dbias, partial sums")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_space_channel_im2col_misc(dtype):
    ops = _ops()
    from mi_seg_amd.hip.functional import MERGE_V1_OFFSETS, STD_OFFSETS
    x = rnd(2, 5, 6, 7, 8, dtype=dtype, seed=71)
    for offs in (STD_OFFSETS, MERGE_V1_OFFSETS):
        y = ops.space_to_channel(x, offs)
        xp = F.pad(x, (0, 0, 0, 1, 0, 0, 0, 1))
        yr = torch.cat([xp[:, i::2, j::2, k::2, :] for (i, j, k) in offs], -1)
        assert torch.equal(y, yr)
        g = rnd(*y.shape, dtype=dtype, seed=72)
        xr = x.double().clone().requires_grad_(True)
        xpr = F.pad(xr, (0, 0, 0, 1, 0, 0, 0, 1))
        torch.cat([xpr[:, i::2, j::2, k::2, :] for (i, j, k) in offs], -1).backward(g.double())
        dx = ops.channel_to_space(g, offs, tuple(x.shape))
        assert_parity(dx, xr.grad, TOL[dtype], "channel_to_space against float64")
    col = ops.im2col3(x)
    colr = F.unfold  # noqa: F841  (3D unfold is not in torch; build by shifts)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1, 1, 1))
    ref = torch.cat([xp[:, a:a + 5, b:b + 6, c:c + 7, :] for a in range(3) for b in range(3) for c in range(3)], -1)
    assert torch.equal(col, ref)
    back = ops.im2col3(col, adjoint=True)
    xr = x.double().clone().requires_grad_(True)
    xpr = F.pad(xr, (0, 0, 1, 1, 1, 1, 1, 1))
    torch.cat([xpr[:, a:a + 5, b:b + 6, c:c + 7, :] for a in range(3) for b in range(3) for c in range(3)], -1).backward(col.double())
    assert_parity(back, xr.grad, TOL[dtype], "col2im against float64")
    # add / gelu / colsum / cast
    a, b = rnd(100, 48, dtype=dtype, seed=73), rnd(100, 48, dtype=dtype, seed=74)
    assert_parity(ops.add(a, b), a.double() + b.double(), TOL[dtype], "add")
    assert_parity(ops.gelu_fwd(a), F.gelu(a.double()), TOL[dtype], "gelu_fwd")
    af = a.double().clone().requires_grad_(True)
    F.gelu(af).backward(b.double())
    assert_parity(ops.gelu_bwd(b, a), af.grad, TOL[dtype], "gelu_bwd")
    assert_parity(ops.colsum(a), a.double().sum(0), TOL[dtype], "colsum 100 x 48")
    big = rnd(5000, 300, dtype=dtype, seed=75)
    assert_parity(ops.colsum(big), big.double().sum(0), TOL[dtype], "colsum 5000 x 300")
    w = rnd(37, 53, seed=76)
    assert torch.equal(ops.cast_matrix(w, dtype, transpose=True), w.t().contiguous().to(dtype))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_param_cast_batch_every_layout_in_one_launch(dtype):
    """miseg_param_cast_batch (include/miseg_hip.h): the per-step re-layout of every non-conv weight - plain casts (whole-tile matrices take
    the flat path), transposes, the (co, tap) -> (tap, co) regrouping of ConvTranspose3d weights (unetr_block.py:80), ragged edges and
    one-column matrices - in ONE launch against torch index arithmetic, bit for bit; and the versioned form skips a current table."""
    import ctypes as C
    L, ops = _L(), _ops()
    lib = L.load()
    shapes = [(64, 96, 0, 1, 1), (64, 96, 1, 1, 1), (96, 256, 0, 8, 32), (96, 256, 1, 8, 32), (37, 53, 0, 1, 1), (37, 53, 1, 1, 1), (48, 1, 0, 1, 1),
              (50, 24, 0, 8, 3), (50, 24, 1, 8, 3), (1152, 384, 0, 1, 1), (384, 1152, 1, 1, 1), (32, 36, 0, 1, 1), (40, 64, 1, 1, 1), (33, 64, 0, 1, 1)]
    srcs, dsts, refs = [], [], []
    descs = (L.CastDesc * len(shapes))()
    tile0 = 0
    for i, (R, Cc, tr, inner, outer) in enumerate(shapes):
        w = rnd(R, Cc, seed=300 + i)
        m = torch.arange(Cc, device=DEV)
        m = (m % inner) * outer + m // inner                       # destination column of source column c
        ref = torch.empty(R, Cc, device=DEV)
        ref[:, m] = w
        ref = (ref.t().contiguous() if tr else ref).to(dtype)
        dst = torch.full(ref.shape, float("nan"), dtype=dtype, device=DEV)
        descs[i] = L.CastDesc(w.data_ptr(), dst.data_ptr(), R, Cc, tr, inner, outer, tile0)
        tile0 += ((R + 31) // 32) * ((Cc + 31) // 32)
        srcs.append(w); dsts.append(dst); refs.append(ref)
    raw = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(DEV)
    dt = L.F32 if dtype == torch.float32 else L.BF16
    L.check(lib.miseg_param_cast_batch(raw.data_ptr(), len(shapes), tile0, dt, None, None, ops._stream()), "param_cast_batch")
    torch.cuda.synchronize()
    for sh, d, r in zip(shapes, dsts, refs):
        assert torch.equal(d, r), sh
    # versioned: state == version -> nothing is written; a bumped version -> everything again
    ver = torch.tensor([5, 5, 0], dtype=torch.int64, device=DEV)      # params_version | state[0] = version of the copies, state[1] = arrival counter
    for d in dsts:
        d.fill_(7.0)
    L.check(lib.miseg_param_cast_batch(raw.data_ptr(), len(shapes), tile0, dt, C.c_void_p(ver.data_ptr()), C.c_void_p(ver.data_ptr() + 8), ops._stream()), "param_cast_batch")
    torch.cuda.synchronize()
    assert all(bool((d == 7.0).all()) for d in dsts)
    ver[0] = 6
    L.check(lib.miseg_param_cast_batch(raw.data_ptr(), len(shapes), tile0, dt, C.c_void_p(ver.data_ptr()), C.c_void_p(ver.data_ptr() + 8), ops._stream()), "param_cast_batch")
    torch.cuda.synchronize()
    for sh, d, r in zip(shapes, dsts, refs):
        assert torch.equal(d, r), sh
    assert int(ver[1]) == 6 and int(ver[2]) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dims,ws,ss,heads,C", [((14, 14, 14), (7, 7, 7), (3, 3, 3), 3, 48), ((10, 9, 8), (7, 7, 7), (0, 0, 0), 3, 48),
                                                ((10, 9, 8), (7, 7, 7), (3, 3, 3), 2, 32), ((6, 6, 6), (6, 6, 6), (0, 0, 0), 3, 48),
                                                ((7, 7, 7), (7, 7, 7), (0, 0, 0), 3, 12)])
def test_window_attention_core(dtype, dims, ws, ss, heads, C):
    ops = _ops()
    B = 2
    qkv = rnd(B, *dims, 3 * C, dtype=dtype, seed=81)
    qb = rnd(3 * C, seed=82) * 0.3
    table = rnd(2197, heads, seed=83) * 0.5
    scale = (C // heads) ** -0.5
    out, lse = ops.winattn_fwd(qkv, qb, table, heads, ws, ss, 7, scale)
    qr = qkv.double().clone().requires_grad_(True)
    qbr, tr = qb.double().clone().requires_grad_(True), table.double().clone().requires_grad_(True)
    ref = _ref_window_attention(qr, qbr, tr, heads, ws, ss, 7, scale)
    assert_parity(out, ref, TOL[dtype], "out against float64")
    g = rnd(*out.shape, dtype=dtype, seed=84)
    ref.backward(g.double())
    dqb, dtab = torch.zeros_like(qb), torch.zeros_like(table)
    dqkv = ops.winattn_bwd(qkv, out, lse, g, qb, table, heads, ws, ss, 7, scale, dqb, dtab)
    tol = TOL[dtype] * (2 if dtype == torch.bfloat16 else 1)
    assert_parity(dqkv, qr.grad, tol, "dqkv against float64", local_tol=_dqkv_local_tol(tol, qkv, qb, table, g, heads, ws, ss, scale, qr.grad))
    assert_parity(dtab, tr.grad, tol, "dtable against float64")
    # the Linear's own bias gradient is not part of the fused core: only padded tokens contribute here
    pad_tokens = any((-d) % w for d, w in zip(dims, ws))
    if pad_tokens:
        assert_parity(dqb, qbr.grad, 2 * tol, "dqkv_bias against float64")
    else:
        assert float(dqb.abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dims,ws,ss,heads,C", [((14, 14, 14), (7, 7, 7), (3, 3, 3), 3, 48), ((10, 9, 8), (7, 7, 7), (3, 3, 3), 2, 32),
                                                ((6, 6, 6), (6, 6, 6), (0, 0, 0), 3, 48)])
def test_window_attention_dropout_on_the_probabilities(dtype, dims, ws, ss, heads, C):
    """attn_drop > 0 (swin_transformer_block.py:56-58 -> window_attention.py:93,114): out = (softmax(.) * mask / (1 - p)) v.  The mask the
    kernels draw is miseg_dropout's over the matrix [windows * heads * n][n], so the reference takes it from ops.dropout_apply on ones with the
    same key; forward, every gradient, and the backward pass re-creating the mask from the key alone."""
    ops = _ops()
    B, p = 2, 0.25
    qkv = rnd(B, *dims, 3 * C, dtype=dtype, seed=85)
    qb = rnd(3 * C, seed=86) * 0.3
    table = rnd(2197, heads, seed=87) * 0.5
    scale = (C // heads) ** -0.5
    n = ws[0] * ws[1] * ws[2]
    nwin = B * math.prod(-(-d // w) for d, w in zip(dims, ws))
    ops.begin_step()
    key = ops.DROP.next_key(qkv.device)
    mask = ops.dropout_apply(torch.ones(nwin * heads * n, n, device=DEV), p, key).view(nwin, heads, n, n)
    kept = float((mask != 0).float().mean())
    assert abs(kept - (1 - p)) < 0.01 and torch.all((mask == 0) | ((mask - 1 / (1 - p)).abs() < 1e-6))
    out, lse = ops.winattn_fwd(qkv, qb, table, heads, ws, ss, 7, scale, drop=(p, key))
    # round 3: attention dropout no longer leaves the matrix-core kernels (head_dim 16, bf16) - the same mask, drawn in their accumulator layout
    import ctypes
    from mi_seg_amd.hip import lib as hiplib
    prm = ops.winattn_params(qkv, out, qb, table, lse, heads, ws, ss, 7, scale, (p, key))
    assert hiplib.load().miseg_winattn_on_matrix_cores(ctypes.byref(prm)) == (1 if dtype == torch.bfloat16 else 0)
    qr = qkv.double().clone().requires_grad_(True)
    qbr, tr = qb.double().clone().requires_grad_(True), table.double().clone().requires_grad_(True)
    ref = _ref_window_attention(qr, qbr, tr, heads, ws, ss, 7, scale, drop_mask=mask)
    assert_parity(out, ref, TOL[dtype], "out against float64")
    plain, _ = ops.winattn_fwd(qkv, qb, table, heads, ws, ss, 7, scale)
    assert rel_err(plain, ref) > 0.1                      # the mask really was applied
    g = rnd(*out.shape, dtype=dtype, seed=88)
    ref.backward(g.double())
    dqb, dtab = torch.zeros_like(qb), torch.zeros_like(table)
    dqkv = ops.winattn_bwd(qkv, out, lse, g, qb, table, heads, ws, ss, 7, scale, dqb, dtab, drop=(p, key))
    tol = TOL[dtype] * (2 if dtype == torch.bfloat16 else 1)
    yard = _dqkv_local_tol(tol, qkv, qb, table, g, heads, ws, ss, scale, qr.grad, drop_mask=mask)      # (of the whole dqkv: its worst third)
    for i, name in enumerate("qkv"):
        assert_parity(dqkv[..., i * C:(i + 1) * C], qr.grad[..., i * C:(i + 1) * C], tol, f"d{name}", local_tol=yard)
    assert_parity(dtab, tr.grad, tol, "dtable against float64")
    if any((-d) % w for d, w in zip(dims, ws)):
        assert_parity(dqb, qbr.grad, 2 * tol, "dqkv_bias against float64")


@pytest.mark.parametrize("dims,heads", [((4, 4, 4), 2), ((6, 6, 6), 12), ((5, 5, 5), 2), ((2, 3, 5), 3)])
def test_global_attention_dropout_on_the_matrix_cores(dims, heads):
    """the SABlock of the ViT with dropout_rate > 0 (MONAI SABlock.drop_weights, reference transformer_block.py:59): head_dim 64, no bias table,
    one window.  Round 4: the head_dim-64 matrix-core kernels (csrc/attention_global.hip) draw miseg_dropout's mask over [samples * heads * n][n]
    in their accumulator layouts themselves; against softmax(q k^T scale) o mask @ v with the mask miseg_dropout gives for the same key."""
    import ctypes
    from mi_seg_amd.hip import lib as hiplib
    ops = _ops()
    B, p = 2, 0.1
    C, n = 64 * heads, dims[0] * dims[1] * dims[2]
    qkv = rnd(B, *dims, 3 * C, dtype=torch.bfloat16, seed=93)
    scale = 64 ** -0.5
    ops.begin_step()
    key = ops.DROP.next_key(qkv.device)
    mask = ops.dropout_apply(torch.ones(B * heads * n, n, device=DEV), p, key).view(B, heads, n, n)
    assert 0.05 < float((mask == 0).float().mean()) < 0.15
    out = torch.empty(B, *dims, C, dtype=torch.bfloat16, device=DEV)
    prm = ops.winattn_params(qkv, out, None, None, torch.empty(B, heads, n, device=DEV), heads, dims, (0, 0, 0), 1, scale, drop=(p, key))
    assert hiplib.load().miseg_winattn_on_matrix_cores(ctypes.byref(prm)) == 1
    out, lse = ops.winattn_fwd(qkv, None, None, heads, dims, (0, 0, 0), 1, scale, drop=(p, key))
    qr = qkv.double().clone().requires_grad_(True)
    q, k, v = qr.reshape(B, n, 3, heads, 64).permute(2, 0, 3, 1, 4)
    ref = ((((q @ k.transpose(-2, -1)) * scale).softmax(-1) * mask) @ v).transpose(1, 2).reshape(B, *dims, C)
    assert_parity(out, ref, TOL[torch.bfloat16], "out against float64")
    g = rnd(*out.shape, dtype=torch.bfloat16, seed=94)
    ref.backward(g.double())
    dqkv = ops.winattn_bwd(qkv, out, lse, g, None, None, heads, dims, (0, 0, 0), 1, scale, None, None, drop=(p, key))
    for i, name in enumerate("qkv"):
        assert_parity(dqkv[..., i * C:(i + 1) * C], qr.grad[..., i * C:(i + 1) * C], 2 * TOL[torch.bfloat16], f"d{name}")
    # the same key gives the same mask again (what the backward pass relies on); another key another mask
    out2, _ = ops.winattn_fwd(qkv, None, None, heads, dims, (0, 0, 0), 1, scale, drop=(p, key))
    assert torch.equal(out, out2)
    out3, _ = ops.winattn_fwd(qkv, None, None, heads, dims, (0, 0, 0), 1, scale, drop=(p, ops.DROP.next_key(qkv.device)))
    assert not torch.equal(out, out3)


@pytest.mark.parametrize("dims,heads", [((6, 6, 6), 12), ((5, 5, 5), 2), ((3, 3, 3), 3), ((4, 8, 8), 1), ((2, 3, 5), 2)])
def test_global_attention_head_dim_64_on_the_matrix_cores(dims, heads):
    """the ViT attention of C-UNETR (BASELINE configs[2]): one window = the whole token grid, no bias table, head_dim 64, bf16 -> the MFMA
    kernels of csrc/attention_global.hip; against softmax((q k^T) scale) v in fp32 on the same bf16-rounded qkv (MONAI SABlock semantics,
    reference transformer_block.py:59), and bit-reproducible run to run (no atomics)."""
    ops = _ops()
    B, C = 2, 64 * heads
    n = dims[0] * dims[1] * dims[2]
    qkv = rnd(B, *dims, 3 * C, dtype=torch.bfloat16, seed=91)
    scale = 64 ** -0.5
    out, lse = ops.winattn_fwd(qkv, None, None, heads, dims, (0, 0, 0), 1, scale)
    qr = qkv.double().clone().requires_grad_(True)
    q, k, v = qr.reshape(B, n, 3, heads, 64).permute(2, 0, 3, 1, 4)
    ref = (((q @ k.transpose(-2, -1)) * scale).softmax(-1) @ v).transpose(1, 2).reshape(B, *dims, C)
    assert_parity(out, ref, TOL[torch.bfloat16], "out against float64")
    g = rnd(*out.shape, dtype=torch.bfloat16, seed=92)
    ref.backward(g.double())
    dqkv = ops.winattn_bwd(qkv, out, lse, g, None, None, heads, dims, (0, 0, 0), 1, scale, None, None)
    for i, name in enumerate("qkv"):
        assert_parity(dqkv[..., i * C:(i + 1) * C], qr.grad[..., i * C:(i + 1) * C], 2 * TOL[torch.bfloat16], f"d{name}")
    out2, lse2 = ops.winattn_fwd(qkv, None, None, heads, dims, (0, 0, 0), 1, scale)
    assert torch.equal(out, out2) and torch.equal(lse, lse2)
    assert torch.equal(dqkv, ops.winattn_bwd(qkv, out, lse, g, None, None, heads, dims, (0, 0, 0), 1, scale, None, None))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,S,C", [(2, 216, 768), (1, 27, 768), (2, 1728, 384), (2, 210, 6), (1, 512, 48), (2, 513, 48)])
def test_instnorm_fused_small(dtype, B, S, C):
    """tensors of <= 512 rows per sample take the one-launch forward / backward kernels; same numbers as the reference
    formula (and as the chunked kernels just above the threshold)."""
    ops, L = _ops(), _L()
    x = rnd(B, S, C, dtype=dtype, seed=5) * 2 + 0.5
    res = rnd(B, S, C, dtype=dtype, seed=6)
    dy = rnd(B, S, C, dtype=dtype, seed=7)
    styles = torch.tensor([1, 0][:B], dtype=torch.int32, device=DEV)
    gam = [rnd(C, seed=8) * 0.2 + 1, rnd(C, seed=9) * 0.2 + 1]
    bet = [rnd(C, seed=10) * 0.2, rnd(C, seed=11) * 0.2]
    ops.begin_step()
    y, stat = ops.instnorm_fwd(x, B, S, styles, gam, bet, res=res, act=L.ACT_LEAKY, slope=0.01)
    dg, db = [torch.zeros(C, device=DEV) for _ in range(2)], [torch.zeros(C, device=DEV) for _ in range(2)]
    dx, dres = ops.instnorm_bwd(dy, y, x, B, S, stat, styles, gam, dg, db, act=L.ACT_LEAKY, slope=0.01, want_dres=True)
    xf = x.double().clone().requires_grad_(True)
    rf = res.double().clone().requires_grad_(True)
    gp = [g.double().clone().requires_grad_(True) for g in gam]
    bp = [b_.double().clone().requires_grad_(True) for b_ in bet]
    mu = xf.mean(1, keepdim=True)
    var = ((xf - mu) ** 2).mean(1, keepdim=True)
    xh = (xf - mu) / torch.sqrt(var + 1e-5)
    G = torch.stack([gp[int(s)] for s in styles.tolist()])[:, None]
    Bt = torch.stack([bp[int(s)] for s in styles.tolist()])[:, None]
    yr = F.leaky_relu(xh * G + Bt + rf, 0.01)
    yr.backward(dy.double())
    tol = 4 * TOL[dtype]
    assert_parity(y, yr, tol, "y against float64")
    assert_parity(dx, xf.grad, tol, "dx against float64")
    assert_parity(dres, rf.grad, tol, "dres against float64")
    for s_ in set(styles.tolist()):
        assert_parity(dg[s_], gp[s_].grad, tol, f"dg[{s_}]")
        assert_parity(db[s_], bp[s_].grad, tol, f"db[{s_}]")


def test_flag_wait_orders_two_streams_on_the_device_and_gives_up_after_its_timeout():
    """miseg_flag_wait (round 4): a one-thread kernel that spins until *flag >= *want - an ordering between two streams (or two hipGraph
    launches) without an event.  (a) a flag set later by another stream releases the waiter, and what follows it sees the producer's data;
    (b) a flag that never comes costs the timeout, increments *timed_out and lets the stream go on (no wave spins for ever)."""
    import ctypes as C
    import time
    from mi_seg_amd.hip import lib as hiplib
    lib = hiplib.load()
    P = lambda t: C.c_void_p(t.data_ptr())
    flag = torch.zeros(1, dtype=torch.int64, device=DEV)
    want = torch.ones(1, dtype=torch.int64, device=DEV)
    one = torch.ones(1, dtype=torch.int64, device=DEV)
    tout = torch.zeros(1, dtype=torch.int32, device=DEV)
    data = torch.zeros(1 << 20, device=DEV)
    seen = torch.zeros(1 << 20, device=DEV)
    # the waiter must not share a hardware queue with the producer (it would block the kernel that releases it: ADVICE round 4) - streams
    # are picked by the library's own probe, as include/miseg_hip_debug.h demands of every user of miseg_flag_wait
    sa, sb, rejected = torch.cuda.Stream(), None, []
    for _ in range(12):
        cand = torch.cuda.Stream()
        rc = lib.miseg_streams_run_concurrently(C.c_void_p(sa.cuda_stream), C.c_void_p(cand.cuda_stream))
        assert rc >= 0, lib.miseg_last_error()
        if rc == 1:
            sb = cand
            break
        rejected.append(cand)          # kept alive: a destroyed stream's queue slot would be handed out again
    assert sb is not None, "no second stream on a hardware queue of its own in 12 tries"
    with pytest.raises(ValueError):
        hiplib.check(lib.miseg_streams_run_concurrently(C.c_void_p(sa.cuda_stream), C.c_void_p(sa.cuda_stream)), "streams_run_concurrently")
    torch.cuda.synchronize()
    with torch.cuda.stream(sb):      # the consumer first: it must wait on the device
        hiplib.check(lib.miseg_flag_wait(P(flag), P(want), 1000000, P(tout), C.c_void_p(sb.cuda_stream)), "flag_wait")
        seen.copy_(data)
    time.sleep(0.05)
    assert not sb.query(), "the waiter must still be spinning: nobody has set the flag"
    with torch.cuda.stream(sa):      # the producer: data, then the flag
        data.fill_(7.0)
        hiplib.check(lib.miseg_counter_copy(P(flag), P(one), C.c_void_p(sa.cuda_stream)), "counter_copy")
    torch.cuda.synchronize()
    assert int(tout.item()) == 0, "the waiter ran into its timeout: its results are void (a hard error, never a statistic)"
    assert bool((seen == 7.0).all())
    # (b) nobody sets flag >= 5: the wait gives up after ~2 ms
    want.fill_(5)
    t0 = time.perf_counter()
    hiplib.check(lib.miseg_flag_wait(P(flag), P(want), 2000, P(tout), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "flag_wait")
    torch.cuda.synchronize()
    assert int(tout.item()) == 1 and time.perf_counter() - t0 < 0.5
    with pytest.raises(ValueError):
        hiplib.check(lib.miseg_flag_wait(P(flag), P(want), 0, P(tout), C.c_void_p(0)), "flag_wait")
