"""The tall weight-gradient products of one block of the backward pass in ONE streaming launch (miseg_gemm_tn_stream_group, ABI 15;
hip/ops.py: gemm_tn queues them on the step's StepQueues, tn_stream_close / every flush issues the open group).  The plan on the host
(no device), the grouped kernel against exact integer products and against the float64 product / the ungrouped launch, the queue's
behaviour, and one Swin block + one decoder block with a training arena, grouped against ungrouped."""
import ctypes as C

import pytest
import torch

from parity import assert_parity
from test_hip_kernels import TOL, rnd

DEV = "cuda"
A = 1 << 12      # an aligned stand-in address: the plan reads pointers for alignment only


def _ops():
    from mi_seg_amd.hip import ops
    return ops


def _L():
    from mi_seg_amd.hip import lib
    return lib


# ------------------------------------------------------------------------------------------------------------ 1. the plan (host only)
STAGE1_BLOCK = [(110592, 192, 48), (110592, 48, 192), (110592, 48, 48), (110592, 144, 48)]      # (T, M, N): fc1, fc2, proj, qkv of the headline's stage 1
PLAN_GROUPS = {
    "stage-1 block": STAGE1_BLOCK,
    "stage-2 block": [(13824, 384, 96), (13824, 96, 384), (13824, 96, 96), (13824, 288, 96)],
    "decoder1 (shortcut, transposed conv)": [(884736, 48, 96), (110592, 96, 384)],
    "decoder2": [(110592, 96, 192), (13824, 192, 768)],
    "a lone product": [(13824, 96, 384)],
    "the kernel tests' group": [(2048, 192, 48), (2113, 48, 192), (4100, 96, 96), (2048, 48, 48), (4100, 144, 48), (2113, 48, 384)],
    "one long stream beside short ones": [(393216, 192, 48), (2048, 48, 48), (2048, 144, 48), (2113, 96, 96)],
}


def _plan(group):
    L = _L()
    n = len(group)
    descs, plans = (L.GemmTnStreamDesc * n)(), (L.GemmTnStreamPlan * n)()
    for j, (T, M, N) in enumerate(group):
        descs[j] = L.GemmTnStreamDesc(A, M, A, N, A, N, None, None, M, N, T, 1)
    assert L.load().miseg_gemm_tn_stream_group_plan(descs, n, plans) == 0, L.load().miseg_last_error()
    return list(plans)


def _lone_splits(T, M, N):
    L = _L()
    p = L.Gemm(A, M, A, N, A, N, M, N, T, 1, 1, L.BF16, L.F32, None, L.ACT_NONE, 1, 0, None, None, 0, None, 0, 0, 0)
    return L.load().miseg_gemm_tn_splits(C.byref(p))


@pytest.mark.parametrize("name", list(PLAN_GROUPS))
def test_group_plan_properties(name):
    group = PLAN_GROUPS[name]
    target = _L().load().miseg_gemm_tn_stream_group_target()
    plans = _plan(group)
    blocks = 0
    for (T, M, N), pl in zip(group, plans):
        # the tile form stays the lone plan's: 4x1 for N <= 48, 1x4 for M <= 48, else 2x2 wave tiles of 48x48
        assert (pl.wm, pl.wn) == ((4, 1) if N <= 48 else (1, 4) if M <= 48 else (2, 2))
        assert pl.gx == -(-M // (48 * pl.wm)) and pl.gy == -(-N // (48 * pl.wn))
        assert pl.tps % 64 == 0 and pl.splits >= 1
        assert pl.splits * pl.tps >= T and (pl.splits - 1) * pl.tps < T
        assert pl.block0 == blocks                                   # contiguous ranges, in order
        blocks += pl.gx * pl.gy * pl.splits
        assert pl.workspace_bytes == (pl.splits * M * N * 4 if pl.splits > 1 else 0)
    assert blocks <= target + len(group), (blocks, target)          # the target plus one rounding block per problem
    if name == "one long stream beside short ones":
        assert plans[0].splits > 1 and all(pl.splits == 1 for pl in plans[1:])      # (the direct-store test below relies on it)


def test_a_group_leaves_fewer_partial_tiles_than_its_products_planned_alone():
    """the figures of DESIGN.md section 9.4: partial-tile bytes of the headline's stage-1 block, grouped and as four lone launches"""
    plans = _plan(STAGE1_BLOCK)
    grouped = sum(pl.workspace_bytes for pl in plans)
    alone = 0
    for T, M, N in STAGE1_BLOCK:
        s = _lone_splits(T, M, N)
        assert s >= 1
        alone += s * M * N * 4 if s > 1 else 0
    print(f"stage-1 block partial tiles: grouped {grouped} bytes ({[pl.splits for pl in plans]} splits), alone {alone} bytes")
    assert 0 < grouped < alone


def test_group_plan_refuses_what_the_streaming_kernel_does_not_take():
    L = _L()
    for T, M, N, a in ((2047, 48, 48, A), (4096, 40, 48, A), (4096, 48, 48, A + 8)):
        d = (L.GemmTnStreamDesc * 1)(L.GemmTnStreamDesc(a, M, A, N, A, N, None, None, M, N, T, 1))
        assert L.load().miseg_gemm_tn_stream_group_plan(d, 1, (L.GemmTnStreamPlan * 1)()) != 0
    d = (L.GemmTnStreamDesc * 9)()
    assert L.load().miseg_gemm_tn_stream_group_plan(d, 9, (L.GemmTnStreamPlan * 9)()) != 0


# ------------------------------------------------------------------------------------------------------------ 2. / 3. the kernel
# (T, M, N, mode, regroup, colsum): mode 0 fresh (garbage in the destination), 1 accumulate onto content, 2 accumulate onto known zeros
SIX = [(2048, 192, 48, 1, 0, True), (2113, 48, 192, 0, 0, False), (4100, 96, 96, 2, 0, False), (2048, 48, 48, 1, 0, True), (4100, 144, 48, 0, 0, False),
       (2113, 48, 384, 2, 48, False)]


def _ints(n, c, mod, off, dtype):
    return ((torch.arange(n * c, device=DEV) * 3 + off) % mod - mod // 2).reshape(n, c).to(dtype)


def _operands(cases, integer):
    out = []
    for i, (T, M, N, mode, regroup, cs) in enumerate(cases):
        if integer:
            a, b = _ints(T, M, 7, i, torch.bfloat16), _ints(T, N, 5, i, torch.bfloat16)      # values in [-3, 3] and [-2, 2]: |sum| <= 6 T < 2^24
            prior = _ints(M, N, 9, i, torch.float32)
            cprior = _ints(1, M, 5, i, torch.float32).reshape(M)
        else:
            a, b = rnd(T, M, dtype=torch.bfloat16, seed=51 + i), rnd(T, N, dtype=torch.bfloat16, seed=61 + i)
            prior, cprior = rnd(M, N, seed=71 + i), rnd(M, seed=81 + i)
        out.append((a, b, prior, cprior))
    return out


def _regrouped(p, c):
    """column j * c + i of the product at column i * (N / c) + j"""
    M, N = p.shape
    return p.view(M, N // c, c).transpose(1, 2).reshape(M, N)


def _run_group(cases, operands):
    """every case through ONE open group of a fresh StepQueues, then flush(); returns [(out, colsum_out)], the number of grouped launches"""
    ops = _ops()
    q = ops.StepQueues()
    keep, ops.DEFAULT_QUEUES = ops.DEFAULT_QUEUES, q
    n0 = ops.TN_STREAM_GROUP_LAUNCHES
    res = []
    try:
        for (T, M, N, mode, regroup, cs), (a, b, prior, cprior) in zip(cases, operands):
            out = torch.full((M, N), float("nan"), device=DEV) if mode == 0 else prior.clone() if mode == 1 else torch.zeros(M, N, device=DEV)
            cso = cprior.clone() if cs else None
            if mode == 0:      # gemm_tn queues accumulate-mode products only (a gradient slot): the overwriting form enters the group here
                ops._tn_stream_enqueue(q, (a, b, out, 0, 0, cso))
            else:
                ops.gemm_tn(a, b, out=out, accumulate=mode, regroup=regroup, colsum_out=cso)
            res.append((out, cso))
        assert len(q.tn_stream) == len(cases) and ops.TN_STREAM_GROUP_LAUNCHES == n0
        q.flush()
        assert not q.tn_stream and not q.tn_reduce
    finally:
        ops.DEFAULT_QUEUES = keep
    return res, ops.TN_STREAM_GROUP_LAUNCHES - n0


def _expected(case, a, b, prior, cprior, product):
    T, M, N, mode, regroup, cs = case
    p = _regrouped(product, regroup) if regroup else product
    return (p + prior.to(p.dtype) if mode == 1 else p), (cprior.to(p.dtype) + a.to(p.dtype).sum(0) if cs else None)


@pytest.mark.gpu
def test_group_of_six_exact_integers():
    """small integer operands: every summation order is exact, so the three tile forms, the ragged last stages (2113, 4100 = 64 * 64 + 4), the
    three destination modes, the regrouped store and the column sums must equal the fp32 torch product bit for bit"""
    operands = _operands(SIX, integer=True)
    res, launches = _run_group(SIX, operands)
    assert launches == 1
    for case, (a, b, prior, cprior), (out, cso) in zip(SIX, operands, res):
        want, cwant = _expected(case, a, b, prior, cprior, a.float().t() @ b.float())
        assert torch.equal(out, want), case
        if cwant is not None:
            assert torch.equal(cso, cwant), case


@pytest.mark.gpu
def test_group_of_six_random_bf16():
    ops = _ops()
    operands = _operands(SIX, integer=False)
    res, launches = _run_group(SIX, operands)
    assert launches == 1
    for case, (a, b, prior, cprior), (out, cso) in zip(SIX, operands, res):
        want, cwant = _expected(case, a, b, prior, cprior, a.double().t() @ b.double())
        assert_parity(out, want, TOL[torch.bfloat16], f"grouped vs float64 {case}")
        lone, _ = _expected(case, a, b, prior, cprior, ops.gemm_tn(a, b))          # the ungrouped launch: same bf16 products, fp32 sums in another order
        assert_parity(out, lone, TOL[torch.float32], f"grouped vs ungrouped {case}")
        if cwant is not None:
            assert_parity(cso, cwant, TOL[torch.bfloat16], f"column sums {case}")


@pytest.mark.gpu
def test_a_problem_with_one_split_stores_or_adds_directly():
    """one long stream takes nearly the whole target: the short products beside it get ONE split each and write their destination from the
    kernel's epilogue - a store (fresh), an add onto content, an add onto known zeros - with the column sums beside; exact integers"""
    cases = [(393216, 192, 48, 1, 0, False), (2048, 48, 48, 0, 0, False), (2048, 144, 48, 1, 0, True), (2113, 96, 96, 2, 0, False)]
    plans = _plan([c[:3] for c in cases])
    assert plans[0].splits > 1 and all(pl.splits == 1 for pl in plans[1:])
    operands = _operands(cases, integer=True)      # |sum| <= 6 * 393216 < 2^24
    res, launches = _run_group(cases, operands)
    assert launches == 1
    for case, (a, b, prior, cprior), (out, cso) in zip(cases, operands, res):
        want, cwant = _expected(case, a, b, prior, cprior, a.float().t() @ b.float())
        assert torch.equal(out, want), case
        if cwant is not None:
            assert torch.equal(cso, cwant), case


# ------------------------------------------------------------------------------------------------------------ 4. the queue
@pytest.mark.gpu
def test_queue_behaviour():
    ops = _ops()
    L = _L()
    shapes = [(2048, 192, 48), (2113, 48, 192), (2048, 48, 48), (4100, 144, 48)]
    ab = [(rnd(T, M, dtype=torch.bfloat16, seed=5 + i), rnd(T, N, dtype=torch.bfloat16, seed=9 + i)) for i, (T, M, N) in enumerate(shapes)]
    keep = ops.DEFAULT_QUEUES
    try:
        q = ops.DEFAULT_QUEUES = ops.StepQueues()
        n0 = ops.TN_STREAM_GROUP_LAUNCHES
        outs = [torch.zeros(M, N, device=DEV) for _, M, N in shapes]
        for (a, b), o in zip(ab, outs):
            ops.gemm_tn(a, b, out=o, accumulate=True)
        torch.cuda.synchronize()
        assert len(q.tn_stream) == 4 and ops.TN_STREAM_GROUP_LAUNCHES == n0 and not q.tn_reduce
        assert all(bool((o == 0).all()) for o in outs)                       # nothing was launched
        ops.tn_stream_close()
        plans = _plan(shapes)
        assert ops.TN_STREAM_GROUP_LAUNCHES == n0 + 1 and not q.tn_stream
        assert len(q.tn_reduce) == sum(1 for pl in plans if pl.splits > 1) == 4      # one deferred sum per split product
        q.flush()
        for (a, b), o in zip(ab, outs):
            assert_parity(o, a.double().t() @ b.double(), TOL[torch.bfloat16], "closed group")

        # a ninth product closes the first eight by itself (the descriptor capacity), and flush() issues an open group without a close
        assert L.TN_STREAM_GROUP_CAP == 8
        n0 = ops.TN_STREAM_GROUP_LAUNCHES
        outs = [torch.zeros(48, 48, device=DEV) for _ in range(9)]
        a, b = ab[2]
        for i, o in enumerate(outs):
            ops.gemm_tn(a, b, out=o, accumulate=True)
            assert ops.TN_STREAM_GROUP_LAUNCHES == n0 + (1 if i >= 7 else 0)
        assert len(q.tn_stream) == 1
        q.flush()
        assert ops.TN_STREAM_GROUP_LAUNCHES == n0 + 2 and not q.tn_stream and not q.tn_reduce
        want = a.double().t() @ b.double()
        for o in outs:
            assert_parity(o, want, TOL[torch.bfloat16], "capacity / flush")
        assert torch.equal(outs[0], outs[7])
        ops.check_no_pending()

        # a group of one whose plan equals the lone plan is the lone launch, bit for bit
        T, M, N = shapes[0]
        assert _plan([shapes[0]])[0].splits == _lone_splits(T, M, N)
        a, b = ab[0]
        one, lone = torch.zeros(M, N, device=DEV), torch.zeros(M, N, device=DEV)
        ops.gemm_tn(a, b, out=one, accumulate=True)
        q.flush()
        ops.TN_STREAM_GROUP = False
        n0 = ops.TN_STREAM_GROUP_LAUNCHES
        ops.gemm_tn(a, b, out=lone, accumulate=True)
        assert not q.tn_stream and len(q.tn_reduce) == 1                    # switched off: launched where it is issued, its sum still deferred
        q.flush()
        assert ops.TN_STREAM_GROUP_LAUNCHES == n0
        assert torch.equal(one, lone)
        ops.TN_STREAM_GROUP = True

        # fp32 operands never take the streaming kernel: the grouped small-product launch as before
        af, bf = a.float(), b.float()
        of = torch.zeros(M, N, device=DEV)
        ops.gemm_tn(af, bf, out=of, accumulate=True)
        assert not q.tn_stream and len(q.gemm_tn) == 1
        q.flush()
        assert_parity(of, af.double().t() @ bf.double(), TOL[torch.float32], "fp32")

        # an open group at the end of a pass is an error, not a silently missing gradient
        ops.gemm_tn(a, b, out=one, accumulate=True)
        with pytest.raises(RuntimeError, match="never launched"):
            ops.check_no_pending()
        assert not q.tn_stream
    finally:
        ops.TN_STREAM_GROUP = True
        ops.DEFAULT_QUEUES = keep
    # without a queue (the eager path) nothing is queued at all
    n0 = ops.TN_STREAM_GROUP_LAUNCHES
    y = ops.gemm_tn(*ab[0])
    assert ops.TN_STREAM_GROUP_LAUNCHES == n0
    assert_parity(y, ab[0][0].double().t() @ ab[0][1].double(), TOL[torch.bfloat16], "eager")


# ------------------------------------------------------------------------------------------------------------ 5. model level
@pytest.mark.gpu
def test_swin_block_and_decoder_block_grouped_against_ungrouped():
    """one stage-1 Swin block (16^3 = 4096 tokens at 48 channels: its four linears take the streaming path) feeding one decoder block as the
    skip, with a training arena: forward and data gradients never touch the queue (bit-identical), every parameter gradient agrees to the
    summation order of the split token ranges, and the pass ends with no product left waiting"""
    from mi_seg_amd.hip import ops
    from mi_seg_amd.networks.blocks.swin_transformer_block import SwinTransformerBlock
    from mi_seg_amd.networks.blocks.unetr_block import UnetrUpBlock
    from mi_seg_amd.networks.norms.conditional_instance_norm import styles_to_device
    from mi_seg_amd.networks.norms.utils import parse_normalization
    from mi_seg_amd.runtime.arena import ParamArena
    from mi_seg_amd.utils.detfill import fill_module_
    import gemm_cases
    L = _L()
    for M, N in ((144, 48), (48, 48), (192, 48), (48, 192)):      # dW of qkv, proj, fc1, fc2 over the 4096 tokens
        plan = L.GemmPlan()
        assert L.load().miseg_gemm_plan(C.byref(gemm_cases.params(L, M, N, 4096, tn=1, accumulate=1)), C.byref(plan)) == 0 and plan.kernel == L.GEMM_TN_STREAM
    cond, inst = parse_normalization("instance_cond", True, 4, 2), parse_normalization("instance", True, 4, 2)
    swin = SwinTransformerBlock(48, 3, (7, 7, 7), (3, 3, 3), norm_type=cond)
    up = UnetrUpBlock(3, 96, 48, 3, 2, inst, res_block=True)
    for m in (swin, up):
        fill_module_(m)
        m.to(DEV)
    st = styles_to_device([1], DEV, 1)
    g = torch.Generator().manual_seed(11)
    x0 = (torch.randn(1, 16, 16, 16, 48, generator=g) * 1.5 + 0.3).to(DEV).to(torch.bfloat16)
    z0 = torch.randn(1, 8, 8, 8, 96, generator=g).to(DEV).to(torch.bfloat16)
    cot = torch.randn(1, 16, 16, 16, 48, generator=g).to(DEV).to(torch.bfloat16)
    named = [(f"swin.{k}", p) for k, p in swin.named_parameters()] + [(f"up.{k}", p) for k, p in up.named_parameters()]
    named = [(k, p) for k, p in named if p.requires_grad]
    arena = ParamArena([p for _, p in named], torch.bfloat16)
    res = {}
    try:
        for grouped in (True, False):
            ops.TN_STREAM_GROUP = grouped
            n0 = ops.TN_STREAM_GROUP_LAUNCHES
            x, z = x0.clone().requires_grad_(True), z0.clone().requires_grad_(True)
            arena.begin_step()
            y = up(z, swin(x, st), st)
            y.backward(cot)
            arena.publish()                    # end_backward: flushes, then fails on any product still queued
            ops.check_no_pending()
            res[grouped] = (y.detach().clone(), x.grad.clone(), z.grad.clone(), {k: p.grad.clone() for k, p in named if p.grad is not None},
                            ops.TN_STREAM_GROUP_LAUNCHES - n0)
    finally:
        ops.TN_STREAM_GROUP = True
        arena.detach()
    (y1, dx1, dz1, g1, n1), (y0, dx0, dz0, g0, n0) = res[True], res[False]
    assert n1 == 2 and n0 == 0, (n1, n0)      # the decoder's shortcut (its transposed conv has 512 rows: the small-product launch) and the Swin block's four
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0) and torch.equal(dz1, dz0)
    assert sorted(g1) == sorted(g0) and any(k.endswith("mlp.linear1.weight") for k in g1)
    for k in g0:
        assert_parity(g1[k], g0[k], TOL[torch.float32], k)
