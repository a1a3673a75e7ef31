"""numpy float32 restatement of miseg_weight_average (include/miseg_hip.h): the tick - the schedule, the coefficient of the three forms, the
skip - and the per-element update, every operation rounded on its own.  tests/test_weight_avg_cpu.py holds it to
torch.optim.swa_utils.AveragedModel in float64; tests/test_hip_weight_avg.py holds the kernels to it bit for bit."""
import numpy as np

F = np.float32
EMA, MEAN = 0, 1          # MISEG_AVG_*
MODES = {"ema": EMA, "swa": MEAN}


def new_record():
    """the record as the caller zeroes it once"""
    return {"apply": 0, "first": 0, "coef": F(0.0), "calls": 0, "n_averaged": 0}


def coef(mode, n, decay=0.999, warmup=False):
    """the coefficient c of the update that makes n_averaged n + 1"""
    if mode == MEAN:
        return F(1.0) / F(n + 1)
    dn = F(decay)
    if warmup:
        dn = np.minimum(dn, (F(1.0) + F(n)) / (F(10.0) + F(n)))
    return F(F(1.0) - dn)


def tick(rec, mode, decay=0.999, warmup=False, start=0, every=1, skip=False):
    """the record after one call (a new dict).  skip: the clip record's flag - the whole call changes nothing."""
    if skip:
        return dict(rec)
    t, n = rec["calls"], rec["n_averaged"]
    apply = int(t >= start and (t - start) % every == 0)
    out = dict(rec, calls=t + 1, apply=apply, first=int(n == 0))
    if apply:
        out["coef"] = coef(mode, n, decay, warmup)
        out["n_averaged"] = n + 1
    return out


def update(avg, w, rec):
    """avg after the streaming launch that reads `rec` (float32 arrays of one shape; avg is not looked at when rec says first)"""
    w = np.asarray(w, dtype=F)
    if not rec["apply"]:
        return np.asarray(avg, dtype=F).copy()
    if rec["first"]:
        return w.copy()
    avg = np.asarray(avg, dtype=F)
    c = F(rec["coef"])
    diff = (w - avg).astype(F)
    step = (c * diff).astype(F)
    return (avg + step).astype(F)


def run(weights, mode, decay=0.999, warmup=False, start=0, every=1, skips=None):
    """the average after a sequence of calls: weights[t][i] = parameter i at call t.  Returns (avg per parameter or None, records per call)."""
    rec, avg, recs = new_record(), None, []
    for t, ws in enumerate(weights):
        skip = bool(skips[t]) if skips is not None else False
        rec = tick(rec, mode, decay, warmup, start, every, skip)
        recs.append(rec)
        if not skip and rec["apply"]:
            avg = [update(None if avg is None else avg[i], w, rec) for i, w in enumerate(ws)]
    return avg, recs
