"""The rules of weight averaging (EMA / SWA), without a GPU: the numpy restatement tests/weight_avg_ref.py (which the GPU tests hold the
kernels to bit for bit) against torch.optim.swa_utils.AveragedModel in float64, the host API of training/optim.py::WeightAverager, the
command-line flags, the checkpoint round trip and the refusals of the two C entry points."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

import weight_avg_ref as R

SHAPES = [(48, 48, 3, 3, 3), (7,), (4097,), (96, 33)]
T = 8


class _Net(torch.nn.Module):
    def __init__(self, dtype, seed=3):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s, generator=g, dtype=dtype)) for s in SHAPES])


def _trajectory(seed=11):
    """T sets of randomly perturbed float64 weights: a random walk from a standard-normal start, steps of a tenth"""
    g = torch.Generator().manual_seed(seed)
    w = [torch.randn(*s, generator=g, dtype=torch.float64) for s in SHAPES]
    out = []
    for _ in range(T):
        w = [t + 0.1 * torch.randn(*t.shape, generator=g, dtype=torch.float64) for t in w]
        out.append(w)
    return out


def _bound(traj):
    """|err| <= 6 T 2^-24 M: an update rounds the float32 weight, the difference, the product and the sum, each on a magnitude of at most
    2 M (M = the largest |w| seen), and the error of the steps before contracts by 1 - c"""
    m = max(float(t.abs().max()) for ws in traj for t in ws)
    return 6 * T * 2.0 ** -24 * m, m


# ------------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("form", ["swa", "ema0.9", "ema0.999"])
def test_restatement_against_averaged_model_in_float64(form):
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    traj = _trajectory()
    net = _Net(torch.float64)
    if form == "swa":
        am, mode, decay = AveragedModel(net), R.MEAN, 0.0
    else:
        decay = float(form[3:])
        am, mode = AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(decay)), R.EMA
    for ws in traj:
        with torch.no_grad():
            for p, w in zip(net.ps, ws):
                p.copy_(w)
        am.update_parameters(net)
    assert int(am.n_averaged) == T
    got, recs = R.run([[w.numpy().astype(np.float32) for w in ws] for ws in traj], mode, decay)
    assert [r["n_averaged"] for r in recs] == list(range(1, T + 1)) and all(r["apply"] for r in recs)
    bound, m = _bound(traj)
    worst = 0.0
    for g, want in zip(got, am.module.ps):
        assert g.dtype == np.float32
        worst = max(worst, float(np.max(np.abs(g.astype(np.float64) - want.detach().numpy()))))
    print(f"{form}: worst |restatement - AveragedModel(float64)| = {worst:.3e}, bound {bound:.3e} (M = {m:.3f})")
    assert worst <= bound


@pytest.mark.parametrize("decay", [0.9, 0.999])
def test_restatement_with_warm_up_against_the_formula_in_float64(decay):
    """no torch counterpart: the same recurrence in float64 Python arithmetic, d_n = min(decay, (1 + n) / (10 + n))"""
    traj = _trajectory(seed=13)
    want = None
    for n, ws in enumerate(traj):
        if want is None:
            want = [w.clone() for w in ws]
        else:
            c = 1.0 - min(decay, (1.0 + n) / (10.0 + n))
            want = [a + c * (w - a) for a, w in zip(want, ws)]
    got, recs = R.run([[w.numpy().astype(np.float32) for w in ws] for ws in traj], R.EMA, decay, warmup=True)
    bound, m = _bound(traj)
    worst = max(float(np.max(np.abs(g.astype(np.float64) - w.numpy()))) for g, w in zip(got, want))
    print(f"ema {decay} with warm-up: worst error {worst:.3e}, bound {bound:.3e} (M = {m:.3f})")
    assert worst <= bound
    # the warm-up really bites: the early coefficients are those of (1 + n) / (10 + n), not of the decay
    assert float(recs[1]["coef"]) == float(np.float32(1) - np.float32(2) / np.float32(11))


def test_the_tick():
    """the schedule, the coefficient of the three forms, the skip"""
    f = np.float32
    # (start, every) = (1, 2): calls 1, 3, 5 apply
    rec, seen = R.new_record(), []
    for t in range(6):
        rec = R.tick(rec, R.MEAN, start=1, every=2)
        seen.append((rec["calls"], rec["apply"], rec["first"], rec["n_averaged"]))
    assert seen == [(1, 0, 1, 0), (2, 1, 1, 1), (3, 0, 0, 1), (4, 1, 0, 2), (5, 0, 0, 2), (6, 1, 0, 3)]
    assert rec["coef"] == f(1) / f(3) and rec["coef"].dtype == np.float32
    assert R.coef(R.MEAN, 0) == 1 and R.coef(R.MEAN, 6) == f(1) / f(7)
    assert R.coef(R.EMA, 5, 0.999) == f(1) - f(0.999) and R.coef(R.EMA, 0, 0.0) == 1
    assert R.coef(R.EMA, 0, 0.999, True) == f(1) - f(1) / f(10)
    assert R.coef(R.EMA, 100000, 0.999, True) == f(1) - f(0.999)          # the warm-up ends where (1 + n) / (10 + n) passes the decay
    # a skipped call moves nothing - not even `calls` - and the call after it is the one the skipped one would have been
    rec = R.tick(R.new_record(), R.EMA, 0.9)
    assert R.tick(rec, R.EMA, 0.9, skip=True) == rec
    nxt = R.tick(R.tick(rec, R.EMA, 0.9, skip=True), R.EMA, 0.9)
    assert (nxt["calls"], nxt["n_averaged"], nxt["first"]) == (2, 2, 0)
    # the update: first copies (avg is not looked at), a non-applying record leaves avg alone
    w, a = np.array([1.0, -2.0], dtype=f), np.array([np.nan, np.nan], dtype=f)
    np.testing.assert_array_equal(R.update(a, w, dict(apply=1, first=1, coef=f(0.5))), w)
    assert np.isnan(R.update(a, w, dict(apply=0, first=1, coef=f(0.5)))).all()
    np.testing.assert_array_equal(R.update(np.zeros(2, dtype=f), w, dict(apply=1, first=0, coef=f(0.25))), np.array([0.25, -0.5], dtype=f))


# ------------------------------------------------------------------------------------------------------------------ host API
def test_constructor_refuses_what_the_kernel_would():
    from mi_seg_amd.training.optim import WeightAverager
    for kw in (dict(mode="mean"), dict(mode=None), dict(decay=1.0), dict(decay=-0.1), dict(decay=float("nan")), dict(decay=float("inf")), dict(decay=1.5),
               dict(decay=1.0 - 1e-12),          # rounds to 1 in float32, which is what the kernel would see
               dict(start_step=-1), dict(start_step=1.5), dict(every=0), dict(every=-2), dict(every=2.5), dict(mode="swa", every=0)):
        with pytest.raises(ValueError):
            WeightAverager(None, **kw)          # refused before the optimiser is looked at
    a = WeightAverager(None)                     # ... and a good one touches neither the library nor a device
    assert (a.mode, a.decay, a.warmup, a.start_step, a.every) == ("ema", 0.999, False, 0, 1) and a.avg is None and a.n_averaged == 0
    b = WeightAverager(None, "swa", start_step=10, every=5)
    assert (b.mode, b.start_step, b.every) == ("swa", 10, 5)
    assert WeightAverager(None, "ema", decay=0.0, warmup=True).warmup is True


def test_flags_and_their_defaults():
    from mi_seg_amd.utils import parser as P
    p = P.add_trainer_argparse_args(argparse.ArgumentParser())
    a = p.parse_args([])
    assert a.weight_averaging == "none" and a.ema_decay == 0.999 and a.ema_warmup is False and a.weight_averaging_start == 0
    assert a.weight_averaging_every == 1 and a.no_validate_averaged is False
    a = p.parse_args(["--weight_averaging", "ema", "--ema_decay", "0.99", "--ema_warmup", "--weight_averaging_start", "100", "--weight_averaging_every", "4",
                      "--no_validate_averaged"])
    assert (a.weight_averaging, a.ema_decay, a.ema_warmup, a.weight_averaging_start, a.weight_averaging_every, a.no_validate_averaged) == (
        "ema", 0.99, True, 100, 4, True)
    assert p.parse_args(["--weight_averaging", "swa"]).weight_averaging == "swa"
    for bad in (["--weight_averaging", "mean"], ["--weight_averaging_every", "0"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    q = P.add_tune_argparse_args(P.add_data_argparse_args(P.add_model_argparse_args(argparse.ArgumentParser())))
    assert not hasattr(q.parse_args([]), "weight_averaging")
    from mi_seg_amd.training.predict import build_parser
    assert build_parser().parse_args([]).use_averaged_weights is False and build_parser().parse_args(["--use_averaged_weights"]).use_averaged_weights is True


class _Model(torch.nn.Module):
    """trainable weights, a frozen one and a buffer"""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(5, 3)
        self.frozen = torch.nn.Linear(3, 3)
        for p in self.frozen.parameters():
            p.requires_grad_(False)
        self.b = torch.nn.Linear(3, 2, bias=False)
        self.register_buffer("table", torch.arange(6, dtype=torch.float32))


def _cpu_averager(model, mode="ema", n_averaged=3, **kw):
    """a WeightAverager over a CPU arena whose average holds 2 w + 1 and whose counters say `n_averaged` updates (no kernel runs on a CPU:
    the state arrives the way a checkpoint's does)"""
    from mi_seg_amd.runtime.arena import ParamArena
    from mi_seg_amd.training.optim import ArenaOptimizer, WeightAverager
    arena = ParamArena([p for p in model.parameters() if p.requires_grad], torch.float32)
    opt = ArenaOptimizer(arena, "sgd", lr=1e-3)
    avg = WeightAverager(opt, mode, **kw)
    avg.prepare()
    keep = avg.avg
    avg.prepare()
    assert avg.avg is keep                       # allocated once
    flat = torch.full_like(arena.flat, float("nan"))
    for p, o in zip(arena.params, arena._offs):
        flat[o:o + p.numel()] = 2 * p.detach().reshape(-1) + 1
    sd = avg.state_dict()
    assert sd["n_averaged"] == 0 and sd["calls"] == 0 and sd["numel"] == arena.flat.numel()
    sd.update(avg=flat, n_averaged=n_averaged, calls=n_averaged + 2)
    avg.load_state_dict(sd)
    return arena, opt, avg


def test_averaged_state_dict_has_the_models_keys_and_passes_frozen_tensors_through():
    m = _Model()
    arena, opt, avg = _cpu_averager(m)
    try:
        assert avg.n_averaged == 3 and avg.stats()["calls"] == 5
        want = m.state_dict()
        got = avg.averaged_state_dict(m)
        assert list(got) == list(want)
        for k, v in want.items():
            assert got[k].shape == v.shape and got[k].dtype == v.dtype, k
            if k.startswith("frozen.") or k == "table":
                assert torch.equal(got[k], v), k
            else:
                assert torch.equal(got[k], 2 * v + 1), k
        twin = _Model()
        twin.load_state_dict(got, strict=True)          # a strict loader takes it
        assert torch.equal(twin.b.weight, 2 * m.b.weight + 1)
    finally:
        arena.detach()


def test_nothing_averaged_yet_raises():
    m = _Model()
    arena, opt, avg = _cpu_averager(m, n_averaged=0)
    try:
        with pytest.raises(RuntimeError, match="nothing has been averaged"):
            avg.averaged_state_dict(m)
        with pytest.raises(RuntimeError, match="nothing has been averaged"):
            with avg.applied():
                pass
    finally:
        arena.detach()


def test_state_round_trip_and_mismatches():
    from mi_seg_amd.runtime.arena import ParamArena
    from mi_seg_amd.training.optim import ArenaOptimizer, WeightAverager
    m = _Model()
    arena, opt, avg = _cpu_averager(m, "ema", decay=0.99, warmup=True, start_step=2, every=3)
    try:
        sd = avg.state_dict()
        assert (sd["mode"], sd["decay"], sd["warmup"], sd["start_step"], sd["every"], sd["n_averaged"], sd["calls"]) == ("ema", 0.99, True, 2, 3, 3, 5)
        other = WeightAverager(opt, "ema")
        other.load_state_dict(sd)
        assert (other.decay, other.warmup, other.start_step, other.every, other.n_averaged, other.stats()["calls"]) == (0.99, True, 2, 3, 3, 5)
        assert torch.equal(other.avg.view(torch.int32), avg.avg.view(torch.int32)) and other.avg is not avg.avg
        with pytest.raises(ValueError, match="'swa'"):
            WeightAverager(opt, "swa").load_state_dict(sd)
        small = ParamArena([torch.nn.Parameter(torch.zeros(3))], torch.float32)
        try:
            with pytest.raises(ValueError, match="does not match"):
                WeightAverager(ArenaOptimizer(small, "sgd"), "ema").load_state_dict(sd)
        finally:
            small.detach()
    finally:
        arena.detach()


def test_checkpoint_round_trip(tmp_path):
    from mi_seg_amd.data.checkpoint import export_state, load_model_state
    m = _Model()
    arena, opt, avg = _cpu_averager(m, "swa")
    try:
        for lightning in (False, True):
            path = export_state(m, str(tmp_path / f"ck{int(lightning)}.pt"), epoch=7, averager=avg, lightning=lightning)
            obj = torch.load(path, map_location="cpu", weights_only=False)
            assert list(obj["averaged_state_dict"]) == list(obj["state_dict"])
            assert obj["weight_averager"]["mode"] == "swa" and obj["weight_averager"]["n_averaged"] == 3
            plain, averaged = _Model(), _Model()
            meta = load_model_state(plain, path)
            assert meta["epoch"] == 7 and "averaged_state_dict" not in meta and "weight_averager" in meta
            load_model_state(averaged, path, averaged=True)
            assert torch.equal(plain.a.weight, m.a.weight) and torch.equal(averaged.a.weight, 2 * m.a.weight + 1)
            assert torch.equal(averaged.frozen.weight, m.frozen.weight) and torch.equal(averaged.table, m.table)
            # a resume continues the average
            resumed = type(avg)(opt, "swa")
            resumed.load_state_dict(meta["weight_averager"])
            assert resumed.n_averaged == 3 and torch.equal(resumed.avg.view(torch.int32), avg.avg.view(torch.int32))
        bare = export_state(m, str(tmp_path / "bare.pt"))
        with pytest.raises(KeyError, match="no averaged weights"):
            load_model_state(_Model(), bare, averaged=True)
        load_model_state(_Model(), bare)
        # an averager that has not averaged yet exports its state but no averaged weights
        arena2, opt2, avg2 = _cpu_averager(_Model(), n_averaged=0)
        try:
            early = export_state(m, str(tmp_path / "early.pt"), averager=avg2)
            assert "averaged_state_dict" not in torch.load(early, map_location="cpu", weights_only=False)
            with pytest.raises(KeyError, match="no averaged weights"):
                load_model_state(_Model(), early, averaged=True)
        finally:
            arena2.detach()
    finally:
        arena.detach()


def test_lit_monai_builds_the_averager_from_its_kwargs():
    from mi_seg_amd.networks.lightning_monai import LitMonai
    from mi_seg_amd.runtime.arena import ParamArena
    from mi_seg_amd.training.optim import ArenaOptimizer
    net = torch.nn.Linear(2, 2)
    arena = ParamArena(list(net.parameters()), torch.float32)
    try:
        opt = ArenaOptimizer(arena, "sgd")
        off = LitMonai(net, 2)
        assert off.configure_weight_averager(opt) is None and off.weight_averager is None
        assert LitMonai(net, 2, weight_averaging="none").configure_weight_averager(opt) is None
        lit = LitMonai(net, 2, weight_averaging="ema", ema_decay=0.99, ema_warmup=True, weight_averaging_start=5, weight_averaging_every=2)
        a = lit.configure_weight_averager(opt)
        assert a is lit.weight_averager and (a.mode, a.decay, a.warmup, a.start_step, a.every) == ("ema", 0.99, True, 5, 2) and lit.validate_averaged is True
        lit = LitMonai(net, 2, weight_averaging="swa", no_validate_averaged=True)
        assert lit.configure_weight_averager(opt).mode == "swa" and lit.validate_averaged is False
        with pytest.raises(ValueError):
            LitMonai(net, 2, weight_averaging="ema", ema_decay=1.0).configure_weight_averager(opt)
    finally:
        arena.detach()


# ------------------------------------------------------------------------------------------------------------------ the C entry points
def average_refusals(L, **good):
    """(what, params) of every call of miseg_weight_average that is wrong in exactly one way; `good`: the fields of a call that is right"""
    def params(**kw):
        d = dict(struct_size=C.sizeof(L.WeightAverage), mode=L.AVG_EMA, clip_record=None, decay=0.9, warmup=0, start=0, every=1)
        d.update(good)
        d.update(kw)
        return L.WeightAverage(**d)
    size = C.sizeof(L.WeightAverage)
    cases = [("struct_size", dict(struct_size=size - 8)), ("struct_size", dict(struct_size=0)), ("null pointer", dict(descs_dev=None)),
             ("null pointer", dict(avg=None)), ("null pointer", dict(record=None)), ("empty table", dict(ndesc=0)), ("empty table", dict(ndesc=-3)),
             ("empty table", dict(total_blocks=0)), ("mode", dict(mode=2)), ("mode", dict(mode=-1)), ("decay", dict(decay=1.0)), ("decay", dict(decay=-0.25)),
             ("decay", dict(decay=float("nan"))), ("decay", dict(decay=float("inf"))), ("decay", dict(mode=L.AVG_MEAN, decay=2.0)), ("every", dict(every=0)),
             ("every", dict(every=-1)), ("start", dict(start=-1)), ("16-byte aligned", dict(avg=good["avg"] + 4)), ("16-byte aligned", dict(avg=good["avg"] + 8))]
    return [(what, params(**kw)) for what, kw in cases], params()


def swap_refusals(L, **good):
    def params(**kw):
        d = dict(struct_size=C.sizeof(L.WeightSwap), params_version=None)
        d.update(good)
        d.update(kw)
        return L.WeightSwap(**d)
    cases = [("struct_size", dict(struct_size=C.sizeof(L.WeightSwap) + 8)), ("struct_size", dict(struct_size=0)), ("null pointer", dict(descs_dev=None)),
             ("null pointer", dict(avg=None)), ("empty table", dict(ndesc=0)), ("empty table", dict(total_blocks=0)), ("empty table", dict(total_blocks=-1)),
             ("16-byte aligned", dict(avg=good["avg"] + 4))]
    return [(what, params(**kw)) for what, kw in cases], params()


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """every call is wrong in exactly one way and must come back MISEG_E_BADARG (-1) from the host-side checks: nothing is launched, so the
    stand-in addresses are never read"""
    from mi_seg_amd.hip import lib as L
    so = L.load()
    A = 1 << 20          # a stand-in for device buffers (16-byte aligned)
    assert so.miseg_abi_struct_size(b"miseg_weight_average_record") == C.sizeof(L.WeightAverageRecord) == 32
    assert (L.AVG_EMA, L.AVG_MEAN) == (R.EMA, R.MEAN) and L.AVG_MODES == R.MODES
    cases, _ = average_refusals(L, descs_dev=A, ndesc=1, total_blocks=1, avg=A, record=A)
    for what, p in cases:
        assert so.miseg_weight_average(C.byref(p), None) == -1, what
        assert what in so.miseg_last_error().decode() and so.miseg_last_error().decode().startswith("weight_average"), (what, so.miseg_last_error())
    assert so.miseg_weight_average(None, None) == -1
    cases, _ = swap_refusals(L, descs_dev=A, ndesc=1, total_blocks=1, avg=A)
    for what, p in cases:
        assert so.miseg_weight_swap(C.byref(p), None) == -1, what
        assert what in so.miseg_last_error().decode() and so.miseg_last_error().decode().startswith("weight_swap"), (what, so.miseg_last_error())
    assert so.miseg_weight_swap(None, None) == -1
