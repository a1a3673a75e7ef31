"""GPU tests of weight averaging on the device (csrc/training.hip: weight_average_tick_kernel, weight_average_kernel, weight_swap_kernel;
training/optim.py::WeightAverager; runtime/graph.py::GraphedTrainStep(weight_averager=)).

The kernels are held BIT FOR BIT to the numpy restatement tests/weight_avg_ref.py (which tests/test_weight_avg_cpu.py holds to
torch.optim.swa_utils.AveragedModel in float64): an update is one float32 subtract, multiply and add per element, each rounded on its own,
and the coefficient a handful of float32 operations of one thread - there is nothing to tolerate.  The captured step is held to the
restatement applied to snapshots of the weights it left, which is independent of how the step itself rounds; applied() to a twin model
loaded from averaged_state_dict, logit for logit."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_hip_grad_accum as TA          # the small C-UNet, its criterion and samples
import test_hip_grad_clip as T            # SHAPES: the 4096-block edges and the scalar tails
import test_weight_avg_cpu as TC          # the refusal cases
import weight_avg_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = T.SHAPES
FORMS = {"ema": dict(mode=R.EMA, decay=0.9), "ema_warmup": dict(mode=R.EMA, decay=0.999, warmup=True), "swa": dict(mode=R.MEAN, decay=0.0)}


def _arena(misaligned=True):
    """SHAPES in a float32 arena - plus, with `misaligned`, two parameters whose own storage starts 4 bytes off a 16-byte boundary (7 and 4099
    elements: the scalar path alone and over two blocks); their arena slots are aligned like all others"""
    from mi_seg_amd.runtime.arena import ParamArena
    from mi_seg_amd.training.optim import ArenaOptimizer
    g = torch.Generator().manual_seed(1)
    params = [torch.nn.Parameter(torch.randn(*s, generator=g).to(DEV)) for s in SHAPES]
    if misaligned:
        for n in (7, 4099):
            base = torch.randn(n + 5, generator=g).to(DEV)
            params.append(torch.nn.Parameter(base[1:1 + n]))
            assert params[-1].data_ptr() % 16 == 4 and params[-1].is_contiguous()
    arena = ParamArena(params, torch.float32)
    return params, arena, ArenaOptimizer(arena, "sgd", lr=1e-3)


def _slices(arena):
    return [slice(o, o + p.numel()) for o, p in zip(arena._offs, arena.params)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _record(rec):
    r = rec.cpu()
    return {"apply": int(r[0]), "first": int(r[1]), "coef": r[2:3].view(torch.float32).numpy()[0], "calls": int(r[3]), "n_averaged": int(r[4])}


def _params(L, opt, avg, rec, clip=None, mode=R.EMA, decay=0.9, warmup=False, start=0, every=1):
    return L.WeightAverage(C.sizeof(L.WeightAverage), mode, opt._table.data_ptr(), len(opt.arena.params), opt._blocks, avg.data_ptr(), rec.data_ptr(),
                           None if clip is None else clip.data_ptr(), decay, int(warmup), start, every)


def _new_weights(params, g):
    for p in params:
        p.data.copy_(torch.randn(p.numel(), generator=g).view(p.shape))
    return [p.detach().cpu().numpy().copy() for p in params]


def _expect(avg_host, ws, rec, sl):
    """the whole avg buffer after the streaming launch that reads `rec`"""
    want = avg_host.copy()
    if rec["apply"]:
        for s, w in zip(sl, ws):
            want[s] = R.update(avg_host[s], w.reshape(-1), rec)
    return want


# ------------------------------------------------------------------------------------------------------------------ 1. every form
@pytest.mark.parametrize("start,every", [(0, 1), (1, 2)])
@pytest.mark.parametrize("form", list(FORMS))
def test_every_form_bit_for_bit(form, start, every):
    from mi_seg_amd.hip import lib as L
    from mi_seg_amd.hip import ops
    params, arena, opt = _arena()
    try:
        kw = dict(FORMS[form], start=start, every=every)
        sl = _slices(arena)
        g = torch.Generator().manual_seed(7 + start)
        avg = torch.full((arena.flat.numel(),), float("nan"), device=DEV)          # the first apply must not read it
        rec = torch.zeros(8, dtype=torch.int32, device=DEV)
        want_rec, applied = R.new_record(), 0
        for call in range(6):
            ws = _new_weights(params, g)
            before = avg.cpu().numpy().copy()
            want_rec = R.tick(want_rec, kw["mode"], kw["decay"], kw.get("warmup", False), start, every)
            want = _expect(before, ws, want_rec, sl)
            ops._call("miseg_weight_average", _params(L, opt, avg, rec, **kw))
            torch.cuda.synchronize()
            got, got_rec = avg.cpu().numpy(), _record(rec)
            bad = _bits(got) != _bits(want)
            assert not bad.any(), f"{form} call {call}: avg differs in {int(bad.sum())} elements, first at {int(np.argmax(bad))}"
            if not want_rec["apply"]:
                assert (_bits(got) == _bits(before)).all()
            applied += want_rec["apply"]
            for k in ("calls", "n_averaged", "apply", "first"):
                assert got_rec[k] == want_rec[k], (form, call, k, got_rec, want_rec)
            if applied:          # (coef is written by applying calls only)
                assert got_rec["coef"].tobytes() == np.float32(want_rec["coef"]).tobytes(), (form, call, got_rec["coef"], want_rec["coef"])
            for p, w in zip(params, ws):          # the parameters are never written
                assert (_bits(p.detach().cpu().numpy()) == _bits(w)).all()
        assert applied == (6 if (start, every) == (0, 1) else 3) and got_rec["calls"] == 6
        for s in sl:
            assert np.isfinite(got[s]).all()
        pad = np.ones(got.size, dtype=bool)
        for s in sl:
            pad[s] = False
        assert pad.any() and np.isnan(got[pad]).all()          # the padding between the slots keeps its bits
    finally:
        arena.detach()


# ------------------------------------------------------------------------------------------------------------------ 2. the guard
def test_a_skipped_step_is_not_averaged():
    from mi_seg_amd.hip import lib as L
    from mi_seg_amd.hip import ops
    params, arena, opt = _arena()
    try:
        sl = _slices(arena)
        g = torch.Generator().manual_seed(17)
        runs = {}
        for tag in ("record", "none"):
            avg = torch.full((arena.flat.numel(),), float("nan"), device=DEV)
            rec = torch.zeros(8, dtype=torch.int32, device=DEV)
            clip = torch.zeros(8, dtype=torch.int32, device=DEV) if tag == "record" else None
            g.manual_seed(17)
            want_rec, out = R.new_record(), []
            for call, skip in enumerate([0, 1, 0, 1] if tag == "record" else [0, 0]):
                ws = _new_weights(params, g) if not skip else [p.detach().cpu().numpy().copy() for p in params]
                if clip is not None:
                    clip[3] = skip
                before, rec_before = avg.cpu().numpy().copy(), rec.cpu().clone()
                want_rec = R.tick(want_rec, R.EMA, 0.9, skip=bool(skip))
                want = before if skip else _expect(before, ws, want_rec, sl)
                ops._call("miseg_weight_average", _params(L, opt, avg, rec, clip=clip))
                torch.cuda.synchronize()
                got = avg.cpu().numpy()
                assert (_bits(got) == _bits(want)).all(), (tag, call)
                if skip:
                    assert torch.equal(rec.cpu(), rec_before), (tag, call)          # no counter moved
                else:
                    out.append((got.copy(), rec.cpu().clone()))
                gr = _record(rec)
                assert (gr["calls"], gr["n_averaged"]) == (want_rec["calls"], want_rec["n_averaged"])
            runs[tag] = out
        # with skip 0 a call behaves as without a record: the two unskipped calls of either run leave the same bits
        assert len(runs["record"]) == len(runs["none"]) == 2
        for (a, ra), (b, rb) in zip(runs["record"], runs["none"]):
            assert (_bits(a) == _bits(b)).all() and torch.equal(ra, rb)
    finally:
        arena.detach()


# ------------------------------------------------------------------------------------------------------------------ 3. the swap
def test_swap_exchanges_and_a_second_call_restores():
    from mi_seg_amd.hip import lib as L
    from mi_seg_amd.hip import ops
    params, arena, opt = _arena()
    try:
        sl = _slices(arena)
        g = torch.Generator().manual_seed(23)
        w0 = _new_weights(params, g)
        avg = torch.randn(arena.flat.numel(), generator=g).to(DEV)
        a0 = avg.cpu().numpy().copy()
        version = torch.tensor([41], dtype=torch.int64, device=DEV)
        p = L.WeightSwap(C.sizeof(L.WeightSwap), opt._table.data_ptr(), len(params), opt._blocks, avg.data_ptr(), version.data_ptr())
        ops._call("miseg_weight_swap", p)
        torch.cuda.synchronize()
        a1 = avg.cpu().numpy().copy()
        want = a0.copy()
        for s, w in zip(sl, w0):
            want[s] = w.reshape(-1)
        assert (_bits(a1) == _bits(want)).all()          # the slots hold the weights, the padding its old bits
        for q, s in zip(params, sl):
            assert (_bits(q.detach().cpu().numpy().reshape(-1)) == _bits(a0[s])).all()
        assert int(version) == 42
        ops._call("miseg_weight_swap", p)
        torch.cuda.synchronize()
        assert (_bits(avg.cpu().numpy()) == _bits(a0)).all() and int(version) == 43
        for q, w in zip(params, w0):
            assert (_bits(q.detach().cpu().numpy()) == _bits(w)).all()
        # without a version word: the same exchange
        ops._call("miseg_weight_swap", L.WeightSwap(C.sizeof(L.WeightSwap), opt._table.data_ptr(), len(params), opt._blocks, avg.data_ptr(), None))
        torch.cuda.synchronize()
        assert (_bits(avg.cpu().numpy()) == _bits(a1)).all() and int(version) == 43
    finally:
        arena.detach()


# ------------------------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_come_before_any_launch():
    """each wrong call returns the error code with miseg_last_error naming the condition, on real buffers: whatever a launch would have
    written - avg, the record, the parameters, the version word - keeps its bits"""
    from mi_seg_amd.hip import lib as L
    from mi_seg_amd.hip import ops
    so = L.load()
    params, arena, opt = _arena()
    try:
        avg = torch.randn(arena.flat.numel() + 4, device=DEV)          # (+ 4: a misaligned avg still lies inside the buffer)
        rec = torch.zeros(8, dtype=torch.int32, device=DEV)
        version = torch.tensor([5], dtype=torch.int64, device=DEV)
        good = dict(descs_dev=opt._table.data_ptr(), ndesc=len(params), total_blocks=opt._blocks, avg=avg.data_ptr())

        def state():
            torch.cuda.synchronize()
            return [avg.clone(), rec.clone(), version.clone()] + [p.detach().clone() for p in params]
        before = state()
        cases, ok_avg = TC.average_refusals(L, record=rec.data_ptr(), **good)
        for what, p in cases:
            assert so.miseg_weight_average(C.byref(p), ops._stream()) == -1, what
            assert what in so.miseg_last_error().decode(), (what, so.miseg_last_error())
            with pytest.raises(ValueError, match="weight_average"):
                ops._call("miseg_weight_average", p)
        cases, ok_swap = TC.swap_refusals(L, params_version=version.data_ptr(), **good)
        for what, p in cases:
            assert so.miseg_weight_swap(C.byref(p), ops._stream()) == -1, what
            assert what in so.miseg_last_error().decode(), (what, so.miseg_last_error())
        after = state()
        assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
                   for a, b in zip(before, after))
        # ... and the calls that are right in every field go through
        ops._call("miseg_weight_average", ok_avg)
        ops._call("miseg_weight_swap", ok_swap)
        torch.cuda.synchronize()
        assert _record(rec)["calls"] == 1 and int(version) == 6
    finally:
        arena.detach()


# ------------------------------------------------------------------------------------------------------------------ 5. the captured step
def _net_and_step(averager_kw, opt_kw=None, **step_kw):
    """the small bf16 C-UNet of test_hip_grad_accum.py's end-to-end test (3x3x3 conv weights: the fused pack launch is in play) under a
    GraphedTrainStep with a WeightAverager whose `avg` starts as NaN"""
    from mi_seg_amd.runtime.arena import ParamArena
    from mi_seg_amd.runtime.graph import GraphedTrainStep
    from mi_seg_amd.training.optim import ArenaOptimizer, WeightAverager
    m = TA._small_unet(torch.bfloat16, (8, 16, 32), (1, 2, 2))
    arena = ParamArena([p for p in m.parameters() if p.requires_grad], torch.bfloat16)
    opt = ArenaOptimizer(arena, "adamw", lr=2e-3, weight_decay=1e-5, **(opt_kw or {}))
    avg = WeightAverager(opt, **averager_kw)
    avg.prepare()
    avg.avg.fill_(float("nan"))
    gts = GraphedTrainStep(m, TA._criterion(), opt, (1, 1, 32, 32, 32), (1, 1, 32, 32, 32), arena, weight_averager=avg, **step_kw)
    return m, arena, opt, avg, gts


def _snapshot(arena):
    torch.cuda.synchronize()
    return [p.detach().cpu().numpy().copy().reshape(-1) for p in arena.params]


def _assert_avg(avg, arena, want, what):
    """the slots of avg.avg against the restatement's per-parameter average, bit for bit; the padding still holds the NaN it was given"""
    got = avg.avg.cpu().numpy()
    pad = np.ones(got.size, dtype=bool)
    for i, s in enumerate(_slices(arena)):
        pad[s] = False
        bad = _bits(got[s]) != _bits(want[i])
        assert not bad.any(), f"{what}: parameter {i} differs in {int(bad.sum())} of {bad.size} elements"
    assert np.isnan(got[pad]).all()


@pytest.mark.parametrize("form,start,every", [("ema", 0, 1), ("swa", 1, 2), ("ema_warmup", 0, 1)])
def test_captured_step_averages_the_weights_it_leaves(form, start, every):
    f = FORMS[form]
    mode = {R.EMA: "ema", R.MEAN: "swa"}[f["mode"]]
    m, arena, opt, avg, gts = _net_and_step(dict(mode=mode, decay=f["decay"] if mode == "ema" else 0.999, warmup=f.get("warmup", False), start_step=start,
                                                 every=every))
    try:
        xs, ys = TA._samples(4, 32)
        w_start = _snapshot(arena)
        snaps = []
        for x, y in zip(xs, ys):
            loss = float(gts(x, y, [0]))
            assert loss == loss
            snaps.append(_snapshot(arena))
        assert opt.__dict__.get("_fused") is not None and opt._fused[1] is not None, "the fused conv-pack launch must be in play"
        assert any((a != b).any() for a, b in zip(w_start, snaps[0])) and any((a != b).any() for a, b in zip(snaps[2], snaps[3]))
        want, recs = R.run(snaps, f["mode"], f["decay"], f.get("warmup", False), start, every)
        _assert_avg(avg, arena, want, form)
        st = avg.stats()
        assert st["calls"] == 4 and st["n_averaged"] == recs[-1]["n_averaged"] == (4 if every == 1 else 2) and avg.n_averaged == st["n_averaged"]
        assert np.float32(st["coef"]).tobytes() == np.float32(recs[-1]["coef"]).tobytes()
        assert len(gts.graphs) == 1          # one capture, four replays of it
    finally:
        arena.detach()


def test_captured_step_with_accumulation_averages_on_closing_micro_batches_only():
    m, arena, opt, avg, gts = _net_and_step(dict(mode="ema", decay=0.5), accumulate_grad_batches=2)
    try:
        xs, ys = TA._samples(4, 32)
        closing, prev = [], None
        for j, (x, y) in enumerate(zip(xs, ys)):
            gts(x, y, [0])
            snap = _snapshot(arena)
            now = avg.avg.cpu().numpy().copy()
            if j % 2 == 0:          # a micro-batch that does not close: neither the weights' average nor its counters move
                assert avg.n_averaged == j // 2
                if prev is not None:
                    assert (_bits(now) == _bits(prev)).all()
                else:
                    assert np.isnan(now).all()
            else:
                closing.append(snap)
            prev = now
        want, recs = R.run(closing, R.EMA, 0.5)
        _assert_avg(avg, arena, want, "accumulating")
        assert avg.stats()["calls"] == 2 and avg.n_averaged == 2
        assert sorted(k[-1] for k in gts.graphs) == ["fold", "fold_step"]
    finally:
        arena.detach()


def test_captured_step_the_guard_skips_the_average_too():
    m, arena, opt, avg, gts = _net_and_step(dict(mode="swa"), opt_kw=dict(skip_nonfinite=True))
    try:
        xs, ys = TA._samples(3, 32)
        xs[1] = xs[1].clone()
        xs[1].view(-1)[12345] = float("inf")          # a non-finite loss and gradient: the step is skipped (no fault: an inf is a number)
        snaps, kept = [], []
        for j, (x, y) in enumerate(zip(xs, ys)):
            before = (_snapshot(arena), avg.avg.cpu().numpy().copy(), avg.stats())
            gts(x, y, [0])
            snap = _snapshot(arena)
            if j == 1:
                assert opt.clip_stats()["skipped"] == 1 and opt.clip_stats()["finite"] == 0
                assert all((_bits(a) == _bits(b)).all() for a, b in zip(before[0], snap))          # the step wrote no weight ...
                assert (_bits(avg.avg.cpu().numpy()) == _bits(before[1])).all() and avg.stats() == before[2]          # ... and the average did not move
            else:
                kept.append(snap)
            snaps.append(snap)
        want, _ = R.run(kept, R.MEAN)
        _assert_avg(avg, arena, want, "guarded")
        assert avg.n_averaged == 2 and avg.stats()["calls"] == 2 and opt.clip_stats()["seen"] == 3
    finally:
        arena.detach()


# ------------------------------------------------------------------------------------------------------------------ 6. applied()
def test_applied_computes_on_the_averaged_weights_and_restores_the_training_ones():
    from mi_seg_amd.runtime.arena import ParamArena
    m, arena, opt, avg, gts = _net_and_step(dict(mode="ema", decay=0.5))
    arena2 = None
    try:
        xs, ys = TA._samples(3, 32)
        x = xs[0]
        with pytest.raises(RuntimeError, match="nothing has been averaged"):
            with avg.applied():
                pass
        for xx, yy in zip(xs, ys):
            gts(xx, yy, [0])
        assert avg.n_averaged == 3
        w_before = _snapshot(arena)
        a_before = avg.avg.cpu().numpy().copy()

        def logits(model, ar):
            ar.refresh_weights()
            with torch.no_grad():
                return model(x, [0]).detach().float().clone()
        y_train = logits(m, arena)
        sd = avg.averaged_state_dict(m)
        assert list(sd) == list(m.state_dict())
        with avg.applied() as inside:
            assert inside is avg
            with torch.no_grad():
                y_avg = m(x, [0]).detach().float().clone()
            sd_inside = avg.averaged_state_dict(m)          # inside the context the average sits in the parameters: the same dict
            with pytest.raises(RuntimeError, match="inside applied"):
                avg.update()
        y_after = logits(m, arena)
        assert all(torch.equal(sd[k], sd_inside[k]) for k in sd)
        # the twin: a fresh model loaded strictly from the averaged state dict, with an arena of its own, refreshed
        twin = TA._small_unet(torch.bfloat16, (8, 16, 32), (1, 2, 2))
        twin.load_state_dict(sd, strict=True)
        arena2 = ParamArena([p for p in twin.parameters() if p.requires_grad], torch.bfloat16)
        logits(twin, arena2)                                  # (the first forward registers the re-layouts)
        y_twin = logits(twin, arena2)
        assert not torch.equal(y_avg, y_train), "the averaged weights must differ from the training weights"
        assert torch.equal(y_avg, y_twin), f"stale cast or conv pack inside applied(): max diff {float((y_avg - y_twin).abs().max())}"
        assert torch.equal(y_after, y_train), f"stale cast or conv pack after applied(): max diff {float((y_after - y_train).abs().max())}"
        assert all((_bits(a) == _bits(b)).all() for a, b in zip(w_before, _snapshot(arena)))          # the training weights hold their exact bits
        assert (_bits(avg.avg.cpu().numpy()) == _bits(a_before)).all()
        # training goes on from there: the next replay steps and averages
        gts(xs[0], ys[0], [0])
        assert avg.n_averaged == 4
    finally:
        arena.detach()
        if arena2 is not None:
            arena2.detach()
