"""GPU tests of gradient clipping and the non-finite step guard of the fused optimiser (csrc/training.hip: grad_sqsum_kernel,
grad_norm_finish_kernel and the clipped forms of opt_step_kernel / opt_pack_conv3_batch_kernel; training/optim.py::ArenaOptimizer).

The norm is held to the numpy restatement tests/grad_clip_ref.py (which tests/test_grad_clip_cpu.py holds to torch in float64) within one
float32 ulp: the kernel and the restatement both sum the n <= 2^26 squares in double, where a sum errs by at most n 2^-53 relative - far
below float32's 2^-24 - so after the rounding to float32 the two can differ by one place at most.  Everything the clipped optimiser writes
is compared BIT FOR BIT with the plain optimiser run on gradients that torch clipped beforehand (a float32 multiply by the record's
coefficient, or torch.clamp): the clipping adds one rounding of its own and nothing else."""
import numpy as np
import pytest
import torch

import grad_clip_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(48, 48, 3, 3, 3), (7,), (4097,), (4096,), (4095,), (3, 5), (1,), (96, 33)]          # the optimiser tests' shapes + the 4096-block edges
FUSED_SHAPES = [(16, 16, 3, 3, 3), (40, 24, 3, 3, 3), (7,), (96, 33)]
KINDS = ["adamw", "adam", "sgd"]


def _bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).clone()


def _optimizer(arena, kind, **kw):
    from mi_seg_amd.training.optim import ArenaOptimizer
    if kind == "sgd":
        return ArenaOptimizer(arena, "sgd", momentum=0.9, lr=3e-2, weight_decay=1e-2, **kw)
    return ArenaOptimizer(arena, kind, lr=3e-2, weight_decay=1e-2, **kw)


def _record(opt):
    """the device record as a dict with float32 norm / coef (ArenaOptimizer.clip_stats returns python floats of the same values)"""
    r = opt.clip_record.cpu()
    f = r[:2].view(torch.float32).numpy()
    return {"norm": f[0], "coef": f[1], "finite": int(r[2]), "skip": int(r[3]), "seen": int(r[4]), "clipped": int(r[5]), "skipped": int(r[6]),
            "reserved": int(r[7])}


def _state(arena, opt, params, packs):
    """bits of everything a step may write: parameters, both moments, step counts, the arena's version words and (fused path) the conv packs"""
    s = {"params": [_bits(p) for p in params], "state1": _bits(opt.state1), "steps": opt.steps.clone(), "versions": arena.versions.clone()}
    if opt.state2 is not None:
        s["state2"] = _bits(opt.state2)
    if packs:
        s["packs"] = [(_bits(arena._packs[id(p)][1]), _bits(arena._packs[id(p)][2])) for p in params if p.dim() == 5]
    return s


def _assert_same(a, b, what, skip=()):
    for k in a:
        if k in skip:
            continue
        if isinstance(a[k], list):
            for i, (x, y) in enumerate(zip(a[k], b[k])):
                if isinstance(x, tuple):
                    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]), f"{what}: {k}[{i}] differs"
                else:
                    assert torch.equal(x, y), f"{what}: {k}[{i}] differs in {int((x != y).sum())} of {x.numel()} elements"
        else:
            assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


def _run(shapes, kind, steps, grads, used, opt_kw, dtype=torch.float32, packs=False, feed=None):
    """`steps` optimiser steps on parameters filled from seed 1 with the gradients grads[step][i] (used[step][i] False: `grad is None`).
    feed(step, opt): called after the gradients are in the arena and before the step (to look at / replace them).  Returns per step
    (state after the step, record or None) and the optimiser's `_fused` decision."""
    from mi_seg_amd.runtime.arena import ParamArena
    g = torch.Generator().manual_seed(1)
    params = [torch.nn.Parameter(torch.randn(*s, generator=g).to(DEV)) for s in shapes]
    arena = ParamArena(params, dtype)
    out = []
    try:
        if packs:
            for p in params:
                if p.dim() == 5:
                    assert arena.conv_packs(p) is None          # first request: registered
            arena.begin_step()                                   # builds the table, fills the packs
            # the pack buffers have padding no kernel writes (whatever the allocation held): zeroed, and the packs refilled, so that two runs
            # can be compared buffer for buffer
            for p in params:
                if p.dim() == 5:
                    arena._packs[id(p)][1].zero_()
                    arena._packs[id(p)][2].zero_()
            arena.versions[3] = -1
            arena.begin_step()
        opt = _optimizer(arena, kind, **opt_kw)
        for st in range(steps):
            for i, p in enumerate(params):
                p._miseg_used = bool(used[st][i])
                arena.views[i].copy_(grads[st][i])
            if feed is not None:
                feed(st, opt, arena)
            before = _state(arena, opt, params, packs)
            opt.step()
            torch.cuda.synchronize()
            out.append((_state(arena, opt, params, packs), _record(opt) if opt.clipping else None, before))
        fused = opt.__dict__.get("_fused") is not None and opt._fused[1] is not None
        return out, fused
    finally:
        arena.detach()


def _random_grads(shapes, steps, seed, scales=None):
    g = torch.Generator().manual_seed(seed)
    return [[(torch.randn(*s, generator=g) * (1.0 if scales is None else scales[st])).to(DEV) for s in shapes] for st in range(steps)]


def _ulp_close(got, want):
    got, want = np.float32(got), np.float32(want)
    return bool(np.abs(np.float64(got) - np.float64(want)) <= np.float64(np.spacing(np.abs(want))))


# ------------------------------------------------------------------------------------------------------------------ 1. the norm
@pytest.mark.parametrize("scale", [1.0, 1e-20, 1e18])          # the squares of the last two leave float32's range, not double's
@pytest.mark.parametrize("pattern", ["all", "subset", "none"])
def test_global_norm_matches_the_restatement_within_one_ulp(pattern, scale):
    used = {"all": [True] * 8, "subset": [True, False, True, True, False, True, False, True], "none": [False] * 8}[pattern]
    grads = _random_grads(SHAPES, 1, 7, [scale])
    for i, u in enumerate(used):                                  # an unused slot may hold anything: it is not read
        if not u:
            grads[0][i].view(-1)[0] = float("nan")
            grads[0][i].view(-1)[-1] = float("inf")
    norms = []
    from mi_seg_amd.runtime.arena import ParamArena
    from mi_seg_amd.training.optim import ArenaOptimizer
    g = torch.Generator().manual_seed(1)
    params = [torch.nn.Parameter(torch.randn(*s, generator=g).to(DEV)) for s in SHAPES]
    arena = ParamArena(params, torch.float32)
    try:
        opt = ArenaOptimizer(arena, "sgd", lr=1e-3, gradient_clip_val=1.0, track_grad_norm=True)
        host = [None if not u else t.cpu().numpy() for t, u in zip(grads[0], used)]
        want = R.record(host, "norm", 1.0)
        want_pp = R.param_norms(host)
        for st in range(2):
            for i, p in enumerate(params):
                p._miseg_used = used[i]
                arena.views[i].copy_(grads[0][i])
            opt.step()
            rec = _record(opt)
            pp = opt.grad_norms.cpu().numpy()
            print(f"norm[{pattern}, {scale:g}] device {rec['norm']!r} restatement {want['norm']!r} coef {rec['coef']!r} / {want['coef']!r}")
            assert _ulp_close(rec["norm"], want["norm"]), (rec["norm"], want["norm"])
            assert rec["coef"] == R.clip_coef(rec["norm"], 1.0)          # the coefficient rule, applied to the device's own norm
            assert rec["finite"] == 1 and rec["skip"] == 0 and rec["reserved"] == 0 and rec["seen"] == st + 1 and rec["skipped"] == 0
            assert rec["clipped"] == (st + 1) * int(rec["coef"] < 1)
            for i in range(len(SHAPES)):
                assert _ulp_close(pp[i], want_pp[i]), (i, pp[i], want_pp[i])
                assert used[i] or pp[i] == 0
            assert float(opt.grad_norm) == float(rec["norm"]) and opt.grad_norm.dim() == 0 and opt.grad_norm.is_cuda
            st_ = opt.clip_stats()
            assert st_["norm"] == float(rec["norm"]) and st_["coef"] == float(rec["coef"]) and st_["seen"] == st + 1
            norms.append((rec["norm"].tobytes(), pp.tobytes()))
        if pattern == "none":
            assert rec["norm"] == 0 and rec["coef"] == 1 and rec["finite"] == 1
        else:
            assert rec["norm"] > 0
        assert norms[0] == norms[1], "two runs over the same gradients must give the same bits"
    finally:
        arena.detach()


# ------------------------------------------------------------------------------------------------------------------ 2. norm clipping
@pytest.mark.parametrize("kind", KINDS)
def test_norm_clipping_is_the_plain_step_on_prescaled_gradients_bit_for_bit(kind):
    """three steps; max_norm lies below the norm in steps 0 and 2 and above it in step 1 (whose gradients are ten times smaller)"""
    max_norm = 100.0          # the norm of 77.7 k standard-normal elements is about 279; a tenth of them: 28
    grads = _random_grads(SHAPES, 3, 11, [1.0, 0.1, 1.0])
    used = [[True] * 8, [True] * 8, [True, True, True, True, True, False, True, True]]
    got, _ = _run(SHAPES, kind, 3, grads, used, dict(gradient_clip_val=max_norm))
    coefs = [rec["coef"] for _, rec, _ in got]
    print("norm clipping", kind, [(float(rec["norm"]), float(rec["coef"])) for _, rec, _ in got])
    assert coefs[0] < 1 and coefs[1] == 1 and coefs[2] < 1
    assert [rec["clipped"] for _, rec, _ in got] == [1, 1, 2] and [rec["seen"] for _, rec, _ in got] == [1, 2, 3]
    for st, (_, rec, _) in enumerate(got):
        host = [t.cpu().numpy() if u else None for t, u in zip(grads[st], used[st])]
        assert _ulp_close(rec["norm"], R.total_norm(host)) and rec["coef"] == R.clip_coef(rec["norm"], max_norm)
    # the plain optimiser, built without clipping, on gradients multiplied in float32 by the coefficient (step 1: the raw gradients)
    pre = [[t if st == 1 else t * torch.tensor(coefs[st], dtype=torch.float32, device=DEV) for t in grads[st]] for st in range(3)]
    want, _ = _run(SHAPES, kind, 3, pre, used, {})
    for st in range(3):
        _assert_same(got[st][0], want[st][0], f"{kind} step {st}")
    assert got[2][0]["steps"].tolist() == [3, 3, 3, 3, 3, 2, 3, 3]


# ------------------------------------------------------------------------------------------------------------------ 3. value clipping
@pytest.mark.parametrize("kind,guard", [("adamw", False), ("adam", False), ("sgd", False), ("adamw", True)])
def test_value_clipping_is_the_plain_step_on_clamped_gradients_bit_for_bit(kind, guard):
    v = 0.75
    grads = _random_grads(SHAPES, 2, 13)
    used = [[True] * 8, [True, False, True, True, True, True, True, True]]
    got, _ = _run(SHAPES, kind, 2, grads, used, dict(gradient_clip_val=v, gradient_clip_algorithm="value", skip_nonfinite=guard))
    want, _ = _run(SHAPES, kind, 2, [[torch.clamp(t, -v, v) for t in gs] for gs in grads], used, {})
    for st in range(2):
        _assert_same(got[st][0], want[st][0], f"{kind} step {st}")
        rec = got[st][1]
        assert rec["seen"] == (st + 1 if guard else 0) and rec["clipped"] == 0          # without the guard value clipping needs no norm launch
    assert float((grads[0][0].abs() > v).float().mean()) > 0.2          # the clamp really cut


# ------------------------------------------------------------------------------------------------------------------ 4. fused conv-pack path
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_norm_clipping_on_the_fused_conv_pack_path_bit_for_bit(kind, dtype):
    max_norm = 10.0           # 36 k standard-normal elements: the norm is about 190
    grads = _random_grads(FUSED_SHAPES, 2, 17)
    used = [[True] * 4, [True] * 4]
    got, fused = _run(FUSED_SHAPES, kind, 2, grads, used, dict(gradient_clip_val=max_norm), dtype=dtype, packs=True)
    assert fused, "the fused conv-pack launch must have run"
    coefs = [rec["coef"] for _, rec, _ in got]
    assert all(c < 1 for c in coefs) and got[1][1]["clipped"] == 2
    pre = [[t * torch.tensor(coefs[st], dtype=torch.float32, device=DEV) for t in grads[st]] for st in range(2)]
    want, fused = _run(FUSED_SHAPES, kind, 2, pre, used, {}, dtype=dtype, packs=True)
    assert fused
    for st in range(2):
        _assert_same(got[st][0], want[st][0], f"{kind} {dtype} step {st}")
        assert len(got[st][0]["packs"]) == 2
        v = got[st][0]["versions"].tolist()
        assert v[3] == v[0] and v[1] != v[0], "pack table current, cast table stale"


# ------------------------------------------------------------------------------------------------------------------ 5. the guard
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("clip", [None, 10.0])
@pytest.mark.parametrize("fused", [False, True])
def test_a_nonfinite_gradient_skips_the_whole_step(fused, clip, bad):
    """step 0 carries one inf / NaN in a used slot and must change nothing; step 1 (finite) is the first update"""
    shapes = FUSED_SHAPES if fused else SHAPES
    n = len(shapes)
    grads = _random_grads(shapes, 2, 19)
    grads[0][1 if fused else 2].view(-1)[5] = bad
    used = [[True] * n, [True] * n]
    kw = dict(skip_nonfinite=True) if clip is None else dict(skip_nonfinite=True, gradient_clip_val=clip)
    got, took = _run(shapes, "adamw", 2, grads, used, kw, dtype=torch.bfloat16 if fused else torch.float32, packs=fused)
    assert took == fused
    (after0, rec0, before0), (after1, rec1, _) = got
    _assert_same(after0, before0, "the skipped step")
    assert rec0["finite"] == 0 and rec0["skip"] == 1 and rec0["skipped"] == 1 and rec0["seen"] == 1
    assert after0["steps"].tolist() == [0] * n
    assert rec1["finite"] == 1 and rec1["skip"] == 0 and rec1["skipped"] == 1 and rec1["seen"] == 2
    assert after1["steps"].tolist() == [1] * n                                  # ... and counts as update 1: the plain optimiser's first step
    scaled = [t * torch.tensor(rec1["coef"], dtype=torch.float32, device=DEV) for t in grads[1]]
    want, _ = _run(shapes, "adamw", 1, [scaled], used[:1], {}, dtype=torch.bfloat16 if fused else torch.float32, packs=fused)
    _assert_same(after1, want[0][0], "the step after the skipped one")


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_guard_off_only_reports(bad):
    grads = _random_grads(SHAPES, 1, 23)
    grads[0][3].view(-1)[9] = bad
    got, _ = _run(SHAPES, "adamw", 1, grads, [[True] * 8], dict(gradient_clip_val=1.0))
    rec = got[0][1]
    assert rec["finite"] == 0 and rec["skip"] == 0 and rec["skipped"] == 0 and rec["seen"] == 1
    if bad == float("inf"):
        assert np.isinf(rec["norm"]) and rec["coef"] == 0 and rec["clipped"] == 1
    else:
        assert np.isnan(rec["norm"]) and rec["coef"] == 1 and rec["clipped"] == 0


# ------------------------------------------------------------------------------------------------------------------ 6. refusal
@pytest.mark.parametrize("kw", [dict(gradient_clip_val=1.0), dict(gradient_clip_val=1.0, gradient_clip_algorithm="value"), dict(skip_nonfinite=True),
                                dict(track_grad_norm=True)])
def test_split_early_is_refused_with_clipping_on(kw):
    from mi_seg_amd.runtime.arena import ParamArena
    params = [torch.nn.Parameter(torch.zeros(*s, device=DEV)) for s in [(7,), (3, 5)]]
    arena = ParamArena(params, torch.float32)
    try:
        opt = _optimizer(arena, "adamw", **kw)
        with pytest.raises(ValueError, match="split_early"):
            opt.split_early([params[0]])
        _optimizer(arena, "adamw").split_early([params[0]])          # ... and is what it was with everything off
    finally:
        arena.detach()


# ------------------------------------------------------------------------------------------------------------------ 7. the captured step
def test_graphed_train_step_with_norm_clipping_matches_the_eager_loop():
    """the small bf16 C-UNet of test_hip_unet_vanilla.py::test_graphed_train_step_matches_the_eager_loop (the smallest model a graphed train
    step test uses), three steps that all clip, under that test's parity bars; the graph's gradient norm against the eager one likewise"""
    from mi_seg_amd.networks.nets.unet_vanilla import UNetVanilla
    from mi_seg_amd.networks.norms.utils import parse_normalization
    from mi_seg_amd.runtime.arena import ParamArena
    from mi_seg_amd.runtime.graph import GraphedTrainStep
    from mi_seg_amd.training.losses import DiceFocalLoss
    from mi_seg_amd.training.optim import ArenaOptimizer
    from mi_seg_amd.utils.detfill import det_input, fill_module_

    def small():
        m = UNetVanilla(3, 1, 6, channels=[8, 16, 32, 64], strides=[1, 2, 2, 2], num_res_units=2, act="prelu",
                        norm_down=parse_normalization("instance_cond", True, 4, 2), norm_up=parse_normalization("instance", True, 4, 2), dropout=0.0,
                        bias=True, adn_ordering="NDA")
        fill_module_(m)
        return m.to(DEV).set_compute_dtype(torch.bfloat16)

    clip = 1e-2
    crit = DiceFocalLoss(include_background=False, to_onehot_y=True, softmax=True, squared_pred=True, smooth_nr=0.0, smooth_dr=1e-6)
    xs = [det_input(30 + i, (1, 1, 64, 64, 64)).to(DEV) for i in range(3)]
    ys = [(x.abs() * 3).floor().clamp(0, 5).to(torch.int32) for x in xs]
    mods = [0, 1, 1]
    lrs = [2e-3, 2e-3, 2e-3]
    runs = {}
    for mode in ("eager", "graph"):
        m = small()
        arena = ParamArena([p for p in m.parameters() if p.requires_grad], torch.bfloat16)
        try:
            opt = ArenaOptimizer(arena, "adamw", lr=lrs[0], weight_decay=1e-5, gradient_clip_val=clip)
            losses, norms = [], []
            if mode == "graph":
                gts = GraphedTrainStep(m, crit, opt, xs[0].shape, ys[0].shape, arena)
            for x, y, md, lr in zip(xs, ys, mods, lrs):
                if mode == "graph":
                    gts.set_lr(lr)
                    losses.append(float(gts(x, y, [md])))
                    norms.append(float(gts.grad_norm))
                else:
                    arena.begin_step()
                    loss = crit(m(x, [md]), y)
                    loss.backward()
                    arena.publish()
                    opt.step(lr=lr)
                    losses.append(float(loss.detach()))
                    norms.append(float(opt.grad_norm))
            torch.cuda.synchronize()
            runs[mode] = (losses, {k: v.detach().clone() for k, v in m.state_dict().items()}, norms, opt.clip_stats())
        finally:
            arena.detach()
    le, lg = runs["eager"][0], runs["graph"][0]
    ne, ng = runs["eager"][2], runs["graph"][2]
    print("clipped train step losses: eager", [round(v, 5) for v in le], "graph", [round(v, 5) for v in lg], "norms: eager", ne, "graph", ng)
    assert all(v == v for v in lg)
    for mode in ("eager", "graph"):
        st = runs[mode][3]
        assert st["seen"] == 3 and st["clipped"] == 3 and st["skipped"] == 0 and st["finite"] == 1, (mode, st)
    for i, (a, b) in enumerate(zip(le, lg)):
        assert abs(a - b) < 2e-3 * (1 + i) * abs(a), (i, a, b)
    for i, (a, b) in enumerate(zip(ne, ng)):
        assert a > clip and abs(a - b) < 2e-3 * (1 + i) * abs(a), (i, a, b)
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
    assert moved > 50          # the clipped optimiser inside the graph really stepped
