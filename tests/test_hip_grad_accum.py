"""GPU tests of gradient accumulation over micro-batches (csrc/training.hip: grad_fold_kernel; training/optim.py::GradAccumulator;
runtime/graph.py::GraphedTrainStep(accumulate_grad_batches=)).

The kernel is held BIT FOR BIT to the numpy restatement tests/grad_accum_ref.py (which tests/test_grad_accum_cpu.py holds to torch autograd
in float64): it is one float32 add and one float32 multiply per element, each rounded on its own, so there is nothing to tolerate.  Through
the optimiser a window must leave the bits of the plain optimiser fed the restatement's mean gradient with the window's union of "used"
flags.  The captured step is held to an eager loop under the bars of test_hip_grad_clip.py's captured-step test, and end to end a window
over two samples must be the step on the batch of both."""
import ctypes as C

import numpy as np
import pytest
import torch

import grad_accum_ref as R
import grad_clip_ref as RC
import test_hip_grad_clip as T          # the optimiser harness (_run: state bits after every step) and FUSED_SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = T.SHAPES          # the optimiser tests' shapes: the 4096-block edges and the scalar tails
K = 3


def _patterns(k, n, rot=0):
    """used[j][i] of a window of k micro-batches over n parameters: always / only first / only last / only in the middle / never / always /
    first and last / always, rotated by `rot` so that every shape meets other codes"""
    kinds = [lambda j: True, lambda j: j == 0, lambda j: j == k - 1, lambda j: 0 < j < k - 1, lambda j: False, lambda j: True,
             lambda j: j in (0, k - 1), lambda j: True]
    return [[bool(kinds[(i + rot) % len(kinds)](j)) for i in range(n)] for j in range(k)]


def _arena(shapes, dtype=torch.float32):
    from mi_seg_amd.runtime.arena import ParamArena
    g = torch.Generator().manual_seed(1)
    params = [torch.nn.Parameter(torch.randn(*s, generator=g).to(DEV)) for s in shapes]
    return params, ParamArena(params, dtype)


def _slices(arena):
    return [slice(o, o + p.numel()) for o, p in zip(arena._offs, arena.params)]


# ------------------------------------------------------------------------------------------------------------------ 1. every op code
@pytest.mark.parametrize("rot", [0, 3])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_every_op_code_bit_for_bit(k, rot):
    """the entry point itself, launch by launch over a window of k micro-batches.  Before each launch every slot of either buffer that the
    table says is not read holds NaN - but for the accumulator's slot under op 2, which this launch leaves alone and a later one of the
    window reads; after it BOTH whole buffers (the padding between slots included) must equal the restatement's bits, so a slot that is
    not written keeps its exact bits."""
    from mi_seg_amd.hip import lib as L
    from mi_seg_amd.hip import ops
    from mi_seg_amd.training.optim import ArenaOptimizer
    params, arena = _arena(SHAPES)
    try:
        opt = ArenaOptimizer(arena, "sgd", lr=1e-3)
        n, sl = len(params), _slices(arena)
        g = torch.Generator().manual_seed(100 + 10 * k + rot)
        acc = torch.randn(arena.flat.numel(), generator=g).to(DEV)          # whatever the allocation held
        codes = torch.zeros(n, dtype=torch.int32, device=DEV)
        used = _patterns(k, n, rot)
        scale = R.scale_of(k)
        seen = [False] * n
        seen_codes = set()
        for j in range(k):
            opj = R.op_codes(used[j], seen, j == k - 1)
            seen_codes.update(opj)
            arena.flat.copy_(torch.randn(arena.flat.numel(), generator=g))
            for i, op in enumerate(opj):
                rg, ra = R.reads(op)
                if not rg:
                    arena.flat[sl[i]] = float("nan")
                if not ra and op != R.A:
                    acc[sl[i]] = float("nan")
            codes.copy_(torch.tensor(opj, dtype=torch.int32))
            h_g, h_a = arena.flat.cpu().numpy().copy(), acc.cpu().numpy().copy()
            new_a, new_g = R.fold([h_a[s] for s in sl], [h_g[s] for s in sl], opj, scale)
            want_g, want_a = h_g.copy(), h_a.copy()
            for i, s in enumerate(sl):
                wg, wa = R.writes(opj[i])
                if wg:
                    want_g[s] = new_g[i]
                if wa:
                    want_a[s] = new_a[i]
            p = L.GradFold(C.sizeof(L.GradFold), opt._table.data_ptr(), n, opt._blocks, arena.flat.data_ptr(), acc.data_ptr(), codes.data_ptr(),
                           arena.flat.numel(), float(scale))
            ops._call("miseg_grad_fold", p)
            torch.cuda.synchronize()
            got_g, got_a = arena.flat.cpu().numpy(), acc.cpu().numpy()
            bad_g, bad_a = got_g.view(np.int32) != want_g.view(np.int32), got_a.view(np.int32) != want_a.view(np.int32)
            assert not bad_g.any(), f"k {k} micro-batch {j}: arena differs in {int(bad_g.sum())} elements, first at {int(np.argmax(bad_g))}, ops {opj}"
            assert not bad_a.any(), f"k {k} micro-batch {j}: acc differs in {int(bad_a.sum())} elements, first at {int(np.argmax(bad_a))}, ops {opj}"
            if j == k - 1:          # the window's mean is finite wherever the window had a gradient
                for i, s in enumerate(sl):
                    if seen[i] or used[j][i]:
                        assert np.isfinite(got_g[s]).all(), i
            seen = [a or u for u, a in zip(used[j], seen)]
        assert seen_codes == {1: {4, 5}, 2: {0, 1, 4, 5, 6, 7}, 3: {0, 1, 2, 3, 4, 5, 6, 7}, 4: {0, 1, 2, 3, 4, 5, 6, 7}}[k]
    finally:
        arena.detach()


# ------------------------------------------------------------------------------------------------------------------ 2. through the optimiser
def _windows(shapes, n_windows, k, seed, rot0=0):
    """random gradients and "used" patterns of n_windows windows of k micro-batches; returns (grads[w][j][i], used[w][j][i], the restatement's
    mean gradients as device tensors - zeros for a parameter absent from the window -, the windows' unions)"""
    n = len(shapes)
    grads = [T._random_grads(shapes, k, seed + w) for w in range(n_windows)]
    used = [_patterns(k, n, rot0 + 2 * w) for w in range(n_windows)]
    means, unions = [], []
    for w in range(n_windows):
        host = [[grads[w][j][i].cpu().numpy() for i in range(n)] for j in range(k)]
        mean, union = R.window(host, used[w], k)
        means.append([torch.zeros(*shapes[i]).to(DEV) if m is None else torch.from_numpy(m).view(*shapes[i]).to(DEV) for i, m in enumerate(mean)])
        unions.append(union)
    return grads, used, means, unions


def _accumulating_feed(grads, used, k, lasts=None):
    """T._run's `feed` hook: replaces the step's gradients by a window of k micro-batches folded through a GradAccumulator.  An unused
    parameter's arena slot holds NaN in every micro-batch: it must never be read."""
    from mi_seg_amd.training.optim import GradAccumulator
    accs = {}

    def feed(st, opt, arena):
        acc = accs.get(id(opt))
        if acc is None:
            acc = accs[id(opt)] = GradAccumulator(opt, k)
        nmb = len(grads[st])
        for j in range(nmb):
            for i, p in enumerate(arena.params):
                p._miseg_used = bool(used[st][j][i])
                if used[st][j][i]:
                    arena.views[i].copy_(grads[st][j][i])
                else:
                    arena.views[i].fill_(float("nan"))
            closes = acc.plan(last=None if lasts is None else lasts[st][j])
            assert closes == (j == nmb - 1)
            acc.fold()
    return feed


@pytest.mark.parametrize("kind", T.KINDS)
def test_two_windows_through_the_optimiser_bit_for_bit(kind):
    grads, used, means, unions = _windows(SHAPES, 2, K, 31)
    got, _ = T._run(SHAPES, kind, 2, means, unions, {}, feed=_accumulating_feed(grads, used, K))
    want, _ = T._run(SHAPES, kind, 2, means, unions, {})
    for st in range(2):
        T._assert_same(got[st][0], want[st][0], f"{kind} window {st}")
    # a parameter absent from a window keeps its bits and its step count there
    steps = [[int(u) for u in unions[0]], [int(a) + int(b) for a, b in zip(unions[0], unions[1])]]
    assert not all(unions[0]) and not all(unions[1])
    for st in range(2):
        assert got[st][0]["steps"].tolist() == steps[st]
        for i, u in enumerate(unions[st]):
            if not u:
                assert torch.equal(got[st][0]["params"][i], got[st][2]["params"][i]), (st, i)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_two_windows_on_the_fused_conv_pack_path_bit_for_bit(kind, dtype):
    shapes = T.FUSED_SHAPES
    n = len(shapes)
    grads = [T._random_grads(shapes, K, 41 + w) for w in range(2)]
    # window 0: conv weight 1 only in the middle, the (7,) only first; window 1: conv weight 0 only last, the (96, 33) never
    used = [[[True, j == 1, j == 0, True] for j in range(K)], [[j == K - 1, True, True, False] for j in range(K)]]
    means, unions = [], []
    for w in range(2):
        mean, union = R.window([[grads[w][j][i].cpu().numpy() for i in range(n)] for j in range(K)], used[w], K)
        means.append([torch.zeros(*shapes[i]).to(DEV) if m is None else torch.from_numpy(m).view(*shapes[i]).to(DEV) for i, m in enumerate(mean)])
        unions.append(union)
    got, fused = T._run(shapes, kind, 2, means, unions, {}, dtype=dtype, packs=True, feed=_accumulating_feed(grads, used, K))
    assert fused, "the fused conv-pack launch must have run"
    want, fused = T._run(shapes, kind, 2, means, unions, {}, dtype=dtype, packs=True)
    assert fused
    for st in range(2):
        T._assert_same(got[st][0], want[st][0], f"{kind} {dtype} window {st}")
        assert len(got[st][0]["packs"]) == 2
    assert got[1][0]["steps"].tolist() == [2, 2, 2, 1]


# ------------------------------------------------------------------------------------------------------------------ 3. clipping and the guard
def test_the_clipped_norm_is_the_norm_of_the_folded_mean():
    """the norm launches run behind the closing fold, on the arena: the record holds the norm of the window's MEAN (within one float32 ulp
    of the restatement, the argument of test_hip_grad_clip.py), and the update is the plain one on the mean times the coefficient"""
    max_norm = 50.0          # the mean of three standard-normal gradients over 77.7 k elements has a norm of about 160
    grads, used, means, unions = _windows(SHAPES, 2, K, 51)
    got, _ = T._run(SHAPES, "adamw", 2, means, unions, dict(gradient_clip_val=max_norm), feed=_accumulating_feed(grads, used, K))
    pre = []
    for st in range(2):
        rec = got[st][1]
        host = [m.cpu().numpy() if u else None for m, u in zip(means[st], unions[st])]
        want_norm = RC.total_norm(host)
        print(f"window {st}: device norm {rec['norm']!r} restatement {want_norm!r} coef {rec['coef']!r}")
        assert T._ulp_close(rec["norm"], want_norm), (rec["norm"], want_norm)
        assert rec["coef"] == RC.clip_coef(rec["norm"], max_norm) and rec["coef"] < 1 and rec["seen"] == st + 1 and rec["clipped"] == st + 1
        pre.append([m * torch.tensor(rec["coef"], dtype=torch.float32, device=DEV) for m in means[st]])
    want, _ = T._run(SHAPES, "adamw", 2, pre, unions, {})
    for st in range(2):
        T._assert_same(got[st][0], want[st][0], f"clipped window {st}")


@pytest.mark.parametrize("where", [0, 1, 2])
def test_a_window_with_one_inf_gradient_is_skipped_whole(where):
    """window 0 carries one inf in micro-batch `where` and must change nothing; window 1 (clean) then leaves the bits of a run that never
    saw the bad window"""
    grads, used, means, unions = _windows(SHAPES, 2, K, 61)
    used[0] = [[True] * len(SHAPES) for _ in range(K)]
    grads[0][where][2].view(-1)[4100 % grads[0][where][2].numel()] = float("inf")
    got, _ = T._run(SHAPES, "adamw", 2, means, [[True] * len(SHAPES), unions[1]], dict(skip_nonfinite=True), feed=_accumulating_feed(grads, used, K))
    (after0, rec0, before0), (after1, rec1, _) = got
    T._assert_same(after0, before0, "the skipped window")
    assert rec0["finite"] == 0 and rec0["skip"] == 1 and rec0["skipped"] == 1 and after0["steps"].tolist() == [0] * len(SHAPES)
    assert rec1["finite"] == 1 and rec1["skip"] == 0 and rec1["skipped"] == 1 and rec1["seen"] == 2
    clean, _ = T._run(SHAPES, "adamw", 1, means[1:], unions[1:], dict(skip_nonfinite=True), feed=_accumulating_feed(grads[1:], used[1:], K))
    T._assert_same(after1, clean[0][0], "the window after the skipped one")
    plain, _ = T._run(SHAPES, "adamw", 1, means[1:], unions[1:], {})
    T._assert_same(after1, plain[0][0], "... which is the plain step on its mean")


def test_a_short_window_and_reset():
    """last=True closes a window early and still divides by k; reset() drops an open window"""
    grads, used, means, unions = _windows(SHAPES, 1, K, 71)
    host = [[grads[0][j][i].cpu().numpy() for i in range(len(SHAPES))] for j in range(2)]
    mean, union = R.window(host, used[0][:2], K)          # two micro-batches of a window of three
    short = [torch.zeros(*s).to(DEV) if m is None else torch.from_numpy(m).view(*s).to(DEV) for s, m in zip(SHAPES, mean)]
    got, _ = T._run(SHAPES, "sgd", 1, [short], [union], {}, feed=_accumulating_feed([grads[0][:2]], [used[0][:2]], K, lasts=[[None, True]]))
    want, _ = T._run(SHAPES, "sgd", 1, [short], [union], {})
    T._assert_same(got[0][0], want[0][0], "the short window")

    from mi_seg_amd.training.optim import ArenaOptimizer, GradAccumulator
    params, arena = _arena([(7,), (3, 5)])
    try:
        opt = ArenaOptimizer(arena, "sgd", lr=1e-3)
        acc = GradAccumulator(opt, 2)
        for p in params:
            p._miseg_used = True
        arena.flat.fill_(4.0)
        assert acc.plan() is False
        acc.fold()
        acc.reset()                                   # the open window (sum 4) is dropped
        arena.flat.fill_(1.0)
        assert acc.plan() is False and acc.ops.tolist() == [1, 1]
        acc.fold()
        arena.flat.fill_(2.0)
        assert acc.plan() is True and acc.ops.tolist() == [7, 7]
        acc.fold()
        assert all(bool((v == 1.5).all()) for v in arena.views) and all(p.grad is v for p, v in zip(params, arena.views))
        with pytest.raises(ValueError):
            GradAccumulator(opt, 0)
    finally:
        arena.detach()


# ------------------------------------------------------------------------------------------------------------------ the captured step
def _small_unet(dtype, channels=(8, 16, 32, 64), strides=(1, 2, 2, 2)):
    from mi_seg_amd.networks.nets.unet_vanilla import UNetVanilla
    from mi_seg_amd.networks.norms.utils import parse_normalization
    from mi_seg_amd.utils.detfill import fill_module_
    m = UNetVanilla(3, 1, 6, channels=list(channels), strides=list(strides), num_res_units=2, act="prelu",
                    norm_down=parse_normalization("instance_cond", True, 4, 2), norm_up=parse_normalization("instance", True, 4, 2), dropout=0.0,
                    bias=True, adn_ordering="NDA")
    fill_module_(m)
    return m.to(DEV).set_compute_dtype(dtype)


def _criterion():
    from mi_seg_amd.training.losses import DiceFocalLoss
    return DiceFocalLoss(include_background=False, to_onehot_y=True, softmax=True, squared_pred=True, smooth_nr=0.0, smooth_dr=1e-6)


def _samples(n, side, seed=30):
    from mi_seg_amd.utils.detfill import det_input
    xs = [det_input(seed + i, (1, 1, side, side, side)).to(DEV) for i in range(n)]
    return xs, [(x.abs() * 3).floor().clamp(0, 5).to(torch.int32) for x in xs]


# ------------------------------------------------------------------------------------------------------------------ 4. k = 1 is today's step
def test_accumulate_one_is_the_step_without_the_argument(monkeypatch):
    """every entry point that passes through ops._call while a GraphedTrainStep is built, captured and replayed: with
    accumulate_grad_batches=1 the sequence is the one of a GraphedTrainStep built without the argument, and miseg_grad_fold is not in it"""
    from mi_seg_amd.hip import ops
    from mi_seg_amd.runtime.arena import ParamArena
    from mi_seg_amd.runtime.graph import GraphedTrainStep
    from mi_seg_amd.training.optim import ArenaOptimizer
    names = []
    real = ops._call

    def spy(fn_name, *a, **kw):
        names.append(fn_name)
        return real(fn_name, *a, **kw)
    monkeypatch.setattr(ops, "_call", spy)
    xs, ys = _samples(2, 32)
    seqs, losses = {}, {}
    for tag, kw in (("plain", {}), ("one", dict(accumulate_grad_batches=1)), ("two", dict(accumulate_grad_batches=2))):
        m = _small_unet(torch.bfloat16, (8, 16, 32), (1, 2, 2))
        arena = ParamArena([p for p in m.parameters() if p.requires_grad], torch.bfloat16)
        try:
            opt = ArenaOptimizer(arena, "adamw", lr=2e-3, weight_decay=1e-5)
            del names[:]
            gts = GraphedTrainStep(m, _criterion(), opt, xs[0].shape, ys[0].shape, arena, **kw)
            losses[tag] = [float(gts(x, y, [0])) for x, y in zip(xs, ys)]
            torch.cuda.synchronize()
            seqs[tag] = list(names)
            assert (gts.acc is None) == (tag != "two")
        finally:
            arena.detach()
    assert "miseg_opt_step" in seqs["plain"] and len(seqs["plain"]) > 50
    assert "miseg_grad_fold" not in seqs["plain"] and "miseg_grad_fold" not in seqs["one"]
    assert seqs["one"] == seqs["plain"]
    # the same launches on the same data: the losses agree as two runs of ONE build do - not to the bit after a step, because the
    # weight-gradient sums are order-dependent across workgroups (two runs of the same code differ by up to 4e-5 after 25 steps: DESIGN.md 7.12)
    print("losses: plain", losses["plain"], "one", losses["one"])
    for a, b in zip(losses["one"], losses["plain"]):
        assert abs(a - b) <= 1e-4 * abs(b), (a, b)
    assert seqs["two"].count("miseg_grad_fold") == 2          # one per captured form ("fold", "fold_step"); the warm-up runs do not fold


# ------------------------------------------------------------------------------------------------------------------ 5. captured against eager
def test_graphed_accumulating_step_matches_the_eager_restatement():
    """the small bf16 C-UNet of test_hip_grad_clip.py's captured-step test under its bars: two windows of k = 2 (modalities [0, 1] - the
    window mixes conditional-norm rows - then [1, 1]), a short third one closed with last=True, and a fourth whose two micro-batches are
    both replays of graphs captured earlier.  The eager loop snapshots the arena after every micro-batch, applies the restatement's
    arithmetic in torch (sum in order, then times fl(1/k)) and steps."""
    from mi_seg_amd.runtime.arena import ParamArena
    from mi_seg_amd.runtime.graph import GraphedTrainStep
    from mi_seg_amd.training.optim import ArenaOptimizer, accumulation_scale
    k, lr = 2, 2e-3
    crit = _criterion()
    xs, ys = _samples(7, 64)
    mods = [0, 1, 1, 1, 1, 1, 1]
    window_of = [0, 0, 1, 1, 2, 3, 3]
    closes_at = [False, True, False, True, True, False, True]
    lasts = [None, None, None, None, True, None, None]
    runs = {}
    for mode in ("eager", "graph"):
        m = _small_unet(torch.bfloat16)
        arena = ParamArena([p for p in m.parameters() if p.requires_grad], torch.bfloat16)
        try:
            opt = ArenaOptimizer(arena, "adamw", lr=lr, weight_decay=1e-5)
            losses, replays = [], []
            if mode == "graph":
                gts = GraphedTrainStep(m, crit, opt, xs[0].shape, ys[0].shape, arena, accumulate_grad_batches=k)
                gts.set_lr(lr)
                for x, y, md, last, closes in zip(xs, ys, mods, lasts, closes_at):
                    v0, e0, g0 = int(arena.versions[0]), arena.epoch, len(gts.graphs)
                    losses.append(float(gts(x, y, [md], last=last)))
                    moved = int(arena.versions[0]) - v0
                    assert moved == (1 if closes else 0), (moved, closes)          # a non-closing micro-batch changes no parameter
                    if len(gts.graphs) == g0:                                      # a pure replay (a capture's warm-up steps move the host epoch)
                        replays.append(closes)
                        assert arena.epoch - e0 == (1 if closes else 0)
                    assert all(p.grad is None for p in arena.params) == (not closes)
                assert sorted(key[-1] for key in gts.graphs) == ["fold", "fold", "fold_step"]
                assert replays == [True, True, False, True]
            else:
                snaps = []
                for x, y, md, closes in zip(xs, ys, mods, closes_at):
                    arena.begin_step()
                    loss = crit(m(x, [md]), y)
                    loss.backward()
                    arena.publish()
                    losses.append(float(loss.detach()))
                    snaps.append((arena.flat.clone(), [bool(p._miseg_used) for p in arena.params]))
                    if closes:
                        s = torch.tensor(accumulation_scale(k), dtype=torch.float32, device=DEV)
                        for i, (p, v) in enumerate(zip(arena.params, arena.views)):
                            mine = [f[arena._offs[i]:arena._offs[i] + p.numel()].view(p.shape) for f, u in snaps if u[i]]
                            p._miseg_used = bool(mine)
                            if mine:
                                tot = mine[0]
                                for t in mine[1:]:
                                    tot = tot + t
                                v.copy_(tot * s)
                        snaps = []
                        opt.step(lr=lr)
            torch.cuda.synchronize()
            runs[mode] = (losses, {kk: v.detach().clone() for kk, v in m.state_dict().items()}, opt.steps.clone())
        finally:
            arena.detach()
    le, lg = runs["eager"][0], runs["graph"][0]
    print("accumulating train step losses: eager", [round(v, 5) for v in le], "graph", [round(v, 5) for v in lg])
    assert all(v == v for v in lg)
    for i, (a, b) in enumerate(zip(le, lg)):
        assert abs(a - b) < 2e-3 * (1 + window_of[i]) * abs(a), (i, a, b)
    assert torch.equal(runs["eager"][2], runs["graph"][2])          # the step counts: a row absent from a whole window was not stepped
    assert int(runs["graph"][2].max()) == 4 and int(runs["graph"][2].min()) == 1          # modality 0's rows: the first window only
    num = den = 0.0
    for kk, v in runs["eager"][1].items():
        w = runs["graph"][1][kk]
        if v.is_floating_point():
            assert float((v - w).abs().max()) <= 2.02 * 4 * lr, kk          # (2.02 x the sum of the learning rates of the four steps)
            num += float((v.double() - w.double()).pow(2).sum())
            den += float(v.double().pow(2).sum())
    assert (num / den) ** 0.5 < 2e-2, (num / den) ** 0.5
    sd0 = _small_unet(torch.bfloat16).state_dict()
    moved = sum(1 for kk, v in runs["graph"][1].items() if v.is_floating_point() and not torch.equal(v, sd0[kk]))
    assert moved > 50          # the optimiser inside the "fold_step" graphs really stepped


# ------------------------------------------------------------------------------------------------------------------ 6. the mean, end to end
def test_a_window_is_the_step_on_the_batch_of_its_samples():
    """float32 parity mode (model and arena float32), SGD - the update is linear in the gradient.  d_acc: the weight delta of one k = 2
    window over samples a, b.  d_batch: one eager step on the batch [a, b]; the Dice and focal terms are means over (b, c) and the norms are
    per sample, so it is the same gradient.  d_a: one step on a alone - what a window that dropped b would produce.
    Required: relL2(d_acc, d_batch) <= 0.01 relL2(d_a, d_batch).  A dropped micro-batch gives 1 x, a missing 1/k a distance of order 1,
    float32 reordering 1e-6 or so: the factor 100 separates them.
    Measured on an MI355X: relL2(d_acc, d_batch) = 1.455e-06, relL2(d_a, d_batch) = 2.583e-01."""
    from mi_seg_amd.runtime.arena import ParamArena
    from mi_seg_amd.runtime.graph import GraphedTrainStep
    from mi_seg_amd.training.optim import ArenaOptimizer
    crit = _criterion()
    xs, ys = _samples(2, 32, seed=40)
    mods = [0, 1]
    deltas = {}
    for mode in ("acc", "batch", "a"):
        m = _small_unet(torch.float32, (8, 16, 32), (1, 2, 2))
        before = {kk: v.detach().clone() for kk, v in m.state_dict().items() if v.is_floating_point()}
        arena = ParamArena([p for p in m.parameters() if p.requires_grad], torch.float32)
        try:
            opt = ArenaOptimizer(arena, "sgd", lr=1e-2, momentum=0.9, weight_decay=0.0)
            if mode == "acc":
                gts = GraphedTrainStep(m, crit, opt, xs[0].shape, ys[0].shape, arena, accumulate_grad_batches=2)
                for x, y, md in zip(xs, ys, mods):
                    gts(x, y, [md])
            else:
                x, y, md = (torch.cat(xs), torch.cat(ys), mods) if mode == "batch" else (xs[0], ys[0], mods[:1])
                arena.begin_step()
                crit(m(x, md), y).backward()
                arena.publish()
                opt.step()
            torch.cuda.synchronize()
            deltas[mode] = torch.cat([(v.detach().double() - before[kk].double()).reshape(-1) for kk, v in m.state_dict().items() if kk in before])
        finally:
            arena.detach()

    def rel(a, b):
        return float((a - b).norm() / b.norm())
    assert float(deltas["batch"].norm()) > 0
    r_acc, r_a = rel(deltas["acc"], deltas["batch"]), rel(deltas["a"], deltas["batch"])
    print(f"relL2(d_acc, d_batch) = {r_acc:.3e}   relL2(d_a, d_batch) = {r_a:.3e}")
    assert r_acc <= 0.01 * r_a, (r_acc, r_a)
