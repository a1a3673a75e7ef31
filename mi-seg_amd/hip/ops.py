"""Tensor-level wrappers over the C ABI (no autograd here).  torch is only the allocator / stream provider.

Activations are "channels-last rows": any tensor whose last dim is the channel dim with stride 1 and whose leading
dims collapse to one uniform row stride (e.g. a contiguous [B, D, H, W, C] tensor or a channel slice of one).
"""
import ctypes as C
import os
import threading

import torch

from . import lib as L


def _dt(t):
    if t.dtype == torch.float32:
        return L.F32
    if t.dtype == torch.bfloat16:
        return L.BF16
    raise ValueError(f"unsupported dtype {t.dtype} (float32 / bfloat16 only)")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


STAMPS = {} if os.environ.get("MISEG_STEP_STAMPS") in ("1", "2", "3") else None      # measurement aid (bench.py prints them): name -> slot of _STAMP_BUF
STAMPS_FINE = os.environ.get("MISEG_STEP_STAMPS") == "1"      # "2": only the stamps at the ends of the passes (every stamp is a graph node and
                                                              # the nodes around a fork change how the executor cuts the graph into chains)
STAMPS_BRANCH = os.environ.get("MISEG_STEP_STAMPS") == "3"   # "3": also one stamp behind every launch of the side branch's backward pass and of the
                                                              # end-of-pass flush on either stream (name@stream#n): where the tail of the step goes
_STAMP_BUF = None
_FLUSHING = False


def _stamp_launch(fn_name):
    if STAMPS_BRANCH and (_FLUSHING or in_branch_backward()) and len(STAMPS) < 1000:
        on = "b" if (_BRANCH_STREAM is not None and torch.cuda.current_stream() == _BRANCH_STREAM) else "m"
        stamp(f"{fn_name.replace('miseg_', '')}@{on}#{len(STAMPS)}")


def stamp(name, stream=None, fine=False):
    """record the device wall clock when `stream` (default: the current one) gets here (miseg_debug_stamp; capture-safe); off unless
    MISEG_STEP_STAMPS=1.  read_stamps() returns {name: microseconds} of the last run / replay."""
    global _STAMP_BUF
    if STAMPS is None or (fine and not STAMPS_FINE):
        return
    if _STAMP_BUF is None:
        _STAMP_BUF = torch.zeros(1024, dtype=torch.int64, device="cuda")
    slot = STAMPS.setdefault(name, len(STAMPS))
    st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    L.check(L.load().miseg_debug_stamp(C.c_void_p(_STAMP_BUF.data_ptr() + 8 * slot), st), "debug_stamp")


def read_stamps():
    v = _STAMP_BUF.cpu().tolist()
    return {k: v[i] / 100.0 for k, i in STAMPS.items()}      # 100 MHz


def rows(t):
    """(ld, nrows, C) of a channels-last row view; raises if the leading dims are not uniformly strided."""
    if not t.is_cuda:
        raise L.MisegHipError("miseg ops need CUDA/HIP tensors: the MI355X path has no CPU fallback")
    if t.dim() < 2:
        raise ValueError("need at least [rows, C]")
    if t.stride(-1) != 1 and t.shape[-1] != 1:
        raise ValueError(f"channel dim must be contiguous, got strides {t.stride()}")
    ld = t.stride(-2)
    n = t.shape[-2]
    for i in range(t.dim() - 3, -1, -1):
        if t.shape[i] != 1 and t.stride(i) != ld * n:
            raise ValueError(f"rows are not uniformly strided: shape {tuple(t.shape)} strides {t.stride()}")
        n *= t.shape[i]
    return ld, n, t.shape[-1]


def _fp32(t):
    if t is None:
        return None
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError("parameters / gradients must be contiguous float32")
    return t


PROFILE_HOOK = None   # bench.py roofline leg: list collecting (kernel name, flops, algorithmic bytes) per hooked call; its index is the tag
                      # the library's in-situ timing records with every kernel launch of that call (miseg_prof_arm, csrc/common.cpp)


class _ProfRegion:
    """roofline leg only: every kernel the library launches inside the region records its own begin / end timestamps under one tag - once,
    where the step issues it, on its own stream, beside whatever else is running (side branch, grouped launches: the schedule that is timed)"""

    def __init__(self, name, flops=0.0, nbytes=0.0):
        self.on = PROFILE_HOOK is not None
        if self.on:
            PROFILE_HOOK.append((name, float(flops), float(nbytes)))
            self.tag = len(PROFILE_HOOK) - 1

    def __enter__(self):
        if self.on:
            L.load().miseg_prof_arm(self.tag)
        return self

    def __exit__(self, *exc):
        if self.on:
            L.load().miseg_prof_arm(-1)
        return False


def _call(fn_name, params, prof=None, extra=()):
    lib = L.load()
    if PROFILE_HOOK is not None and prof is not None:
        with _ProfRegion(prof[0], prof[1], prof[2] if len(prof) > 2 else 0.0):
            L.check(getattr(lib, fn_name)(C.byref(params), *extra, _stream()), fn_name)
        return
    L.check(getattr(lib, fn_name)(C.byref(params), *extra, _stream()), fn_name)
    if STAMPS_BRANCH:
        _stamp_launch(fn_name)


def _nb(*tensors):
    """bytes of the given tensors (None skipped): the algorithmic traffic of a launch that touches each of them once"""
    return float(sum(t.numel() * t.element_size() for t in tensors if t is not None))


# ------------------------------------------------------------------------------------------ instance norm
class _ZeroPool:
    """fp64 statistics buffers of a step come from one pre-zeroed pool (one fill instead of ~100 small memsets).

    Lifetime rules.  Every statistics tensor handed out is a VIEW of a chunk, so a chunk lives as long as anything (an autograd node's
    saved tensors) still uses it; the pool itself only decides where the NEXT buffers come from:
      * `begin_step()` (a training arena / GraphedStep owns the step and has enqueued the previous backward pass): the current chunk is
        zero-filled in place and reused - captured hipGraphs rely on these fixed addresses, so a chunk that a graph was captured on is
        never dropped (`pin()`; GraphedStep pins what it captured);
      * `fresh()` (a model forward that nobody manages - LitMonai's eager loop, sliding-window validation, unit tests): the pool lets go
        of its chunk and starts a new one sized by the high-water mark, so earlier forwards whose backward is still pending keep their
        statistics, and 700 inference windows do not grow anything;
      * overflow inside a step: a new chunk is started; the old one stays alive through its views and through `_pinned`."""

    def __init__(self, numel=1 << 20):
        self.numel, self.buf, self.off, self.high = numel, None, 0, 0
        self.spilled = 0         # doubles of this step that live in chunks an overflow has left behind
        self._pinned = []
        self._filled = None      # (event recorded behind the zero fill of the current chunk, streams already ordered behind it)

    def take(self, n, device):
        n = (n + 1) & ~1
        if self.buf is None or self.buf.device != device or self.off + n > self.buf.numel():
            capturing = torch.cuda.is_current_stream_capturing()
            if self.buf is not None:
                self.spilled += self.off
                if capturing:
                    # Overflow INSIDE a hipGraph capture: the graph being recorded holds raw pointers into the chunk that is left behind, so it
                    # must never be freed.  Round 3 found this the hard way: a GraphedForward captured as the first GPU work of a process (the
                    # 1 M-double first chunk overflows several times in a batch-4 fs=48 forward) kept only its LAST chunk alive; the others
                    # went back to the allocator, were handed to the window batches of the sliding-window loop, and every replay after the
                    # first normalised with statistics that other tensors had been written over (logits 43 % off, finite, unnoticed by a
                    # finiteness check; tests/test_hip_training.py::test_full_volume_sliding_window_of_the_headline_model).
                    self.pin()
            # the next chunk holds what the WHOLE step has needed so far, not just the chunk that overflowed: one overflow per step at most
            self.high = max(self.high, self.spilled + n)
            self.buf = torch.empty(max(self.numel, n, int(self.high * 1.5)), dtype=torch.float64, device=device)
            lib = L.load()
            L.check(lib.miseg_fill32(_ptr(self.buf), 0, self.buf.numel() * 2, _stream()), "fill32")
            self.off = 0
            self._filled = None
            if not capturing:
                ev = torch.cuda.Event()
                ev.record()
                self._filled = (ev, {torch.cuda.current_stream().cuda_stream})
        elif self._filled is not None and not torch.cuda.is_current_stream_capturing():
            # A chunk is zero-filled on the stream that happened to need it first.  A model's side branch (SwinUNETR / UNETR) takes buffers of
            # the same chunk on ANOTHER stream: ordered behind the fill only if that stream happened to wait for the first one after the
            # fill was queued - true for the chunk a forward starts with, not for one that an overflow starts in the middle of a branch.
            # Every other stream waits for the fill once, and the allocator learns that the chunk is in use there.
            cs = torch.cuda.current_stream()
            if cs.cuda_stream not in self._filled[1]:
                cs.wait_event(self._filled[0])
                self.buf.record_stream(cs)
                self._filled[1].add(cs.cuda_stream)
        t = self.buf[self.off:self.off + n]
        self.off += n
        self.high = max(self.high, self.spilled + self.off)
        return t

    def begin_step(self):
        """call once per training step, after the previous step's backward has been enqueued: recycles the pool."""
        # The WHOLE chunk is zeroed, not the part the previous step used: a chunk an overflow started late in the warm-up step holds only
        # that step's tail ([0, off)), while the step being captured takes its buffers from the chunk's beginning and walks past `off` into
        # memory that was zero when the chunk was created - and never again: every replay after the first added its statistics to the
        # previous replay's (round 3, found with a GraphedForward captured as the first GPU work of a process; see take()).
        if self.buf is not None:
            lib = L.load()
            L.check(lib.miseg_fill32(_ptr(self.buf), 0, self.buf.numel() * 2, _stream()), "fill32")
            self.off = 0
        self.spilled = 0

    def fresh(self):
        """start the next forward on a new chunk (unless the current one is untouched); see the class docstring"""
        if self.buf is not None and self.off > 0 and not torch.cuda.is_current_stream_capturing():
            self.buf, self.off, self._filled = None, 0, None
        if not torch.cuda.is_current_stream_capturing():
            self.spilled = 0

    def pin(self):
        """keep the current chunk alive for good: a captured hipGraph holds raw pointers into it"""
        if self.buf is not None and not any(b is self.buf for b in self._pinned):
            self._pinned.append(self.buf)


DEFAULT_POOL = _ZeroPool()
STAT_POOL = DEFAULT_POOL      # the ACTIVE pool: every ParamArena owns one (round 3) and makes it the active one for its step / its model's forward
                              # (use_pool); models without an arena share DEFAULT_POOL.  Two models in one process no longer recycle each other's chunk.


def use_pool(pool=None):
    global STAT_POOL
    STAT_POOL = pool if pool is not None else DEFAULT_POOL


def begin_step():
    """start of a training step whose previous backward pass has been enqueued.  Under hipGraph capture the current chunk is recycled in
    place (fixed addresses are what a graph replays); eagerly the step simply moves to a fresh chunk, so statistics that some other
    pending autograd graph still holds are never zero-filled under it."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        STAT_POOL.begin_step()
    else:
        STAT_POOL.fresh()
    DROP.advance()
    check_no_pending()


def begin_forward(params=()):
    """called by the nets at the top of `forward`: when no training arena manages the step (its begin_step() recycles the pool), the
    statistics of this forward go to a fresh chunk, so an un-managed loop neither grows the pool nor clobbers statistics that an earlier,
    not yet back-propagated forward still needs."""
    arena = None
    for p in params:
        arena = getattr(p, "_miseg_arena", None)
        break
    use_pool(getattr(arena, "pool", None))
    if torch.cuda.is_current_stream_capturing():
        return
    if torch.is_grad_enabled() and arena is not None:
        return
    STAT_POOL.fresh()
    DROP.advance()


def instnorm_stats(x, B, S):
    """x: rows view of [B*S, C].  Returns stat: float64 [R, B, C, 2]; summed over the R replicas = (sum x, sum x^2)."""
    ld, n, Cc = rows(x)
    assert n == B * S, (n, B, S)
    stat = STAT_POOL.take(L.load().miseg_instnorm_stat_bytes(B, Cc) // 8, x.device).view(-1, B, Cc, 2)
    _call("miseg_instnorm_stats", L.InstnormStats(_ptr(x), ld, B, S, Cc, _dt(x), _ptr(stat)), prof=("instnorm", 0.0, _nb(x)))
    return stat


def _style_arrays(tensors, n):
    arr = (C.c_void_p * L.MAX_STYLES)()
    for i in range(L.MAX_STYLES):
        arr[i] = tensors[i].data_ptr() if (tensors is not None and i < n and tensors[i] is not None) else None
    return arr


def rank1_stats(x1, w):
    """instance-norm statistics of round(x1[row] * w[c]) without storing it (one sample): x1 rows view [.., 1], w [C] / [C, 1] in x1.dtype"""
    ld, n, one = rows(x1)
    assert one == 1 and w.dtype == x1.dtype and w.is_contiguous()
    Cc = w.numel()
    stat = STAT_POOL.take(L.load().miseg_instnorm_stat_bytes(1, Cc) // 8, x1.device).view(-1, 1, Cc, 2)
    L.check(L.load().miseg_rank1_stats(_ptr(x1), ld, _ptr(w), 1, n, Cc, _dt(x1), _ptr(stat), _stream()), "rank1_stats")
    return stat


def instnorm_apply(x, B, S, stat, styles, gammas, betas, res=None, act=L.ACT_NONE, slope=0.01, eps=1e-5, out=None, res_stat=None,
                   res_gammas=None, res_betas=None, r1=None):
    """res_stat: `res` is the RAW input of a second instance norm (statistics res_stat, affine rows res_gammas / res_betas) applied on the fly.
    r1 = (x1, w): that raw input is round(x1[row] * w[c]) and is not stored (res=None; res_stat from rank1_stats)."""
    ld, n, Cc = rows(x)
    y = out if out is not None else torch.empty(x.shape, dtype=x.dtype, device=x.device)
    ldy, ny, Cy = rows(y)
    assert ny == n and Cy == Cc
    ldr = rows(res)[0] if res is not None else 0
    ns = len(gammas) if gammas is not None else 1
    p = L.InstnormApply(_ptr(x), ld, _ptr(res), ldr, _ptr(y), ldy, B, S, Cc, _dt(x), _ptr(stat), eps, _ptr(styles), ns,
                        _style_arrays(gammas, ns), _style_arrays(betas, ns), act, slope, _ptr(res_stat), _style_arrays(res_gammas, ns),
                        _style_arrays(res_betas, ns))
    if r1 is not None:
        assert res is None and rows(r1[0])[1] == n and r1[1].numel() == Cc and r1[1].dtype == x.dtype
        p.r1x, p.ldr1x, p.r1w = _ptr(r1[0]), rows(r1[0])[0], _ptr(r1[1])
    _call("miseg_instnorm_apply", p, prof=("instnorm", 0.0, _nb(x, res, y, r1[0] if r1 is not None else None)))
    return y


def instnorm_fwd(x, B, S, styles, gammas, betas, res=None, act=L.ACT_NONE, slope=0.01, eps=1e-5, out=None):
    """statistics + normalisation (one register-resident launch for tensors of <= 2048 rows per sample); returns (y, stat)."""
    ld, n, Cc = rows(x)
    assert n == B * S, (n, B, S)
    stat = STAT_POOL.take(L.load().miseg_instnorm_stat_bytes(B, Cc) // 8, x.device).view(-1, B, Cc, 2)
    y = out if out is not None else torch.empty(x.shape, dtype=x.dtype, device=x.device)
    ldr = rows(res)[0] if res is not None else 0
    ns = len(gammas) if gammas is not None else 1
    p = L.InstnormApply(_ptr(x), ld, _ptr(res), ldr, _ptr(y), rows(y)[0], B, S, Cc, _dt(x), _ptr(stat), eps, _ptr(styles), ns,
                        _style_arrays(gammas, ns), _style_arrays(betas, ns), act, slope)
    _call("miseg_instnorm_fwd", p, prof=("instnorm", 0.0, _nb(x, res, y)))      # (statistics are stored, not accumulated: repeatable)
    return y, stat


def instnorm_fwd_slabs(x, pending, B, S, styles, gammas, betas, res=None, act=L.ACT_NONE, slope=0.01, eps=1e-5, out=None):
    """instnorm_fwd on the output `x` of a split convolution that is still `pending` (PendingSlabs): ONE launch sums the slabs, writes x,
    and normalises; returns (y, stat)."""
    ld, n, Cc = rows(x)
    assert n == B * S and ld == Cc, (n, B, S, ld, Cc)
    stat = STAT_POOL.take(L.load().miseg_instnorm_stat_bytes(B, Cc) // 8, x.device).view(-1, B, Cc, 2)
    y = out if out is not None else torch.empty(x.shape, dtype=x.dtype, device=x.device)
    ldr = rows(res)[0] if res is not None else 0
    ns = len(gammas) if gammas is not None else 1
    p = L.InstnormApply(_ptr(x), ld, _ptr(res), ldr, _ptr(y), rows(y)[0], B, S, Cc, _dt(x), _ptr(stat), eps, _ptr(styles), ns,
                        _style_arrays(gammas, ns), _style_arrays(betas, ns), act, slope)
    _call("miseg_instnorm_fwd_slabs", p, prof=("instnorm", 0.0, _nb(x, res, y) + 4.0 * pending.n * pending.stride), extra=(_ptr(pending.ws), pending.n, pending.stride))
    return y, stat


def instnorm_bwd(dy, y, x, B, S, stat, styles, gammas, dgammas, dbetas, act=L.ACT_NONE, slope=0.01, eps=1e-5, want_dres=False, gadd=None, betas=None,
                 pending=None):
    """y=None with a LeakyReLU: valid when no residual entered the activation; the kernels recompute its sign from x (needs betas).
    pending (PendingSlabs): dy is the unwritten output of a split data-gradient convolution - the one-launch kernel sums its slabs itself."""
    ld, n, Cc = rows(x)
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    dres = torch.empty(x.shape, dtype=x.dtype, device=x.device) if want_dres else None
    dstat = STAT_POOL.take(L.load().miseg_instnorm_stat_bytes(B, Cc) // 8, x.device)
    ns = len(gammas) if gammas is not None else 1
    p = L.InstnormBwd(_ptr(dy), rows(dy)[0], _ptr(y), rows(y)[0] if y is not None else 0, _ptr(x), ld, _ptr(dx), rows(dx)[0],
                      _ptr(dres), rows(dres)[0] if dres is not None else 0, B, S, Cc, _dt(x), _ptr(stat), eps, _ptr(dstat), _ptr(styles), ns,
                      _style_arrays(gammas, ns), _style_arrays(dgammas, ns), _style_arrays(dbetas, ns), act, slope,
                      _ptr(gadd), rows(gadd)[0] if gadd is not None else 0, _style_arrays(betas, ns))
    if pending is not None:
        _call("miseg_instnorm_bwd_slabs", p, prof=("instnorm", 0.0, _nb(y, x, dx, dres, gadd) + 4.0 * pending.n * pending.stride),
              extra=(_ptr(pending.ws), pending.n, pending.stride))
        return dx, dres
    _call("miseg_instnorm_bwd", p, prof=("instnorm", 0.0, _nb(dy, y, x, dx, dres, gadd)))
    return dx, dres


def instnorm_bwd_apply(dy, x, B, S, stat, dstat, styles, gammas, dgammas, dbetas, eps=1e-5, gadd=None):
    """the apply half of instnorm_bwd with the backward sums already in `dstat` (the GEMM that produced dy added them in its epilogue)"""
    ld, n, Cc = rows(x)
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    ns = len(gammas) if gammas is not None else 1
    p = L.InstnormBwd(_ptr(dy), rows(dy)[0], None, 0, _ptr(x), ld, _ptr(dx), rows(dx)[0], None, 0, B, S, Cc, _dt(x), _ptr(stat), eps, _ptr(dstat), _ptr(styles), ns,
                      _style_arrays(gammas, ns), _style_arrays(dgammas, ns), _style_arrays(dbetas, ns), L.ACT_NONE, 0.0,
                      _ptr(gadd), rows(gadd)[0] if gadd is not None else 0, _style_arrays(None, ns))
    # (roofline leg: a second pass would add the affine gradients twice - the profiled step's numbers are discarded anyway)
    _call("miseg_instnorm_bwd_apply", p, prof=("instnorm", 0.0, _nb(dy, x, dx, gadd)))
    return dx


def instnorm_bwd_reduce(dy, x, B, S, stat, eps=1e-5):
    """dstat [R, B, C, 2] fp64 whose replicas sum to (sum dy, sum dy * xhat) per (sample, channel); xhat from `stat` (group / batch norms)"""
    ld, n, Cc = rows(x)
    assert n == B * S and rows(dy)[1] == n
    dstat = STAT_POOL.take(L.load().miseg_instnorm_stat_bytes(B, Cc) // 8, x.device).view(-1, B, Cc, 2)
    p = L.InstnormBwd(_ptr(dy), rows(dy)[0], None, 0, _ptr(x), ld, None, 0, None, 0, B, S, Cc, _dt(x), _ptr(stat), eps, _ptr(dstat), None, 1,
                      _style_arrays(None, 1), _style_arrays(None, 1), _style_arrays(None, 1), L.ACT_NONE, 0.0, None, 0, _style_arrays(None, 1))
    _call("miseg_instnorm_bwd_reduce", p)
    return dstat


def affine2(a, x, coef, B, S):
    """y[b, s, c] = coef[b, c, 0] * a + coef[b, c, 1] * x + coef[b, c, 2]; a, x rows views of [B * S, C], coef fp32 [B, C, 3]"""
    lda, n, Cc = rows(a)
    assert n == B * S and rows(x)[1] == n and coef.dtype == torch.float32 and coef.is_contiguous() and tuple(coef.shape) == (B, Cc, 3)
    y = torch.empty(a.shape, dtype=a.dtype, device=a.device)
    _call("miseg_affine2", L.Affine2(C.sizeof(L.Affine2), _ptr(a), lda, _ptr(x), rows(x)[0], _ptr(y), rows(y)[0], _ptr(coef), B, S, Cc, _dt(a)))
    return y


def instnorm_pair_bwd(dy, y, xa, xb, B, S, stat_a, stat_b, styles, gammas_a, gammas_b, dgammas_a, dbetas_a, dgammas_b, dbetas_b, slope=0.01, eps=1e-5,
                      betas_a=None, betas_b=None, r1=None):
    """backward of LeakyReLU(norm_a(xa) + norm_b(xb)): (dxa, dxb) in one reduction + one apply launch.
    y=None: the kernels recompute the activation's sign from xa / xb (needs the betas of affine norms)."""
    ld, n, Cc = rows(xa)
    dxa = torch.empty(xa.shape, dtype=xa.dtype, device=xa.device)
    # r1 = (x1, w, dw): xb = round(x1[row] * w[c]) is not stored (xb = y = None), dw [C] fp32 receives (+=) the 1x1x1 weight gradient
    dxb = torch.empty(xb.shape, dtype=xb.dtype, device=xb.device) if r1 is None else None
    nb = L.load().miseg_instnorm_stat_bytes(B, Cc) // 8
    dsa, dsb = STAT_POOL.take(nb, xa.device), STAT_POOL.take(nb, xa.device)
    ns = len(gammas_a) if gammas_a is not None else 1
    if r1 is not None:
        assert xb is None and y is None and rows(r1[0])[1] == n and r1[1].numel() == Cc and r1[2].numel() == Cc and r1[2].dtype == torch.float32
    p = L.InstnormPairBwd(_ptr(dy), rows(dy)[0], _ptr(y), rows(y)[0] if y is not None else 0, _ptr(xa), ld, _ptr(xb), rows(xb)[0] if xb is not None else 0,
                          _ptr(dxa), rows(dxa)[0], _ptr(dxb), rows(dxb)[0] if dxb is not None else 0,
                          B, S, Cc, _dt(xa), _ptr(stat_a), _ptr(stat_b), eps, _ptr(dsa), _ptr(dsb), _ptr(styles), ns,
                          _style_arrays(gammas_a, ns), _style_arrays(gammas_b, ns), _style_arrays(dgammas_a, ns), _style_arrays(dbetas_a, ns),
                          _style_arrays(dgammas_b, ns), _style_arrays(dbetas_b, ns), slope, _style_arrays(betas_a, ns), _style_arrays(betas_b, ns))
    if r1 is not None:
        p.r1x, p.ldr1x, p.r1w, p.r1dw = _ptr(r1[0]), rows(r1[0])[0], _ptr(r1[1]), _ptr(r1[2])
    _call("miseg_instnorm_pair_bwd", p, prof=("instnorm", 0.0, _nb(dy, y, xa, xb, dxa, dxb, r1[0] if r1 is not None else None)))
    return dxa, dxb


def layernorm_fwd(x, gamma, beta, eps=1e-5):
    ld, n, Cc = rows(x)
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    mean = torch.empty(n, dtype=torch.float32, device=x.device)
    rstd = torch.empty(n, dtype=torch.float32, device=x.device)
    _call("miseg_layernorm_fwd", L.LayernormFwd(_ptr(x), ld, _ptr(y), rows(y)[0], n, Cc, _dt(x), eps, _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(rstd)))
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta):
    ld, n, Cc = rows(x)
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    _call("miseg_layernorm_bwd", L.LayernormBwd(_ptr(dy), rows(dy)[0], _ptr(x), ld, _ptr(dx), rows(dx)[0], n, Cc, _dt(x), _ptr(gamma), _ptr(mean),
                                               _ptr(rstd), _ptr(dgamma), _ptr(dbeta)))
    return dx


# ------------------------------------------------------------------------------------------ GEMM family
# Hand-offs between a producer op and the op right behind it are PER THREAD (the forward pass runs on the caller's thread, the backward pass on
# the autograd engine's device thread; two models stepped from two threads never see each other's): the statistics a GEMM left for the norm
# that consumes its output, and the slab sums a split data-gradient convolution left to the norm backward behind it
_TLS = threading.local()
_ALL_PENDING = []          # every thread's pending-slab table (check_no_pending looks at all of them from the stepping thread)
_ALL_PENDING_LOCK = threading.Lock()


def _set_gemm_stat(out, stat):
    """(key of the output, statistics tensor) of the gemm_nt / mlp_fwd call that just fused them, or None"""
    _TLS.gemm_stat = None if out is None else ((out.data_ptr(), out.numel(), out.dtype), stat)


def pop_gemm_stat(y):
    """the statistics the last gemm_nt / mlp_fwd of THIS thread produced for `y` in its epilogue (handed over once), or None"""
    st = getattr(_TLS, "gemm_stat", None)
    _TLS.gemm_stat = None
    return st[1] if st is not None and st[0] == (y.data_ptr(), y.numel(), y.dtype) else None


class NormRef:
    """a (conditional) instance norm whose apply pass a consumer kernel folds into its operand load (one sample): statistics of the norm's
    raw input + affine rows (miseg_norm_ref, include/miseg_hip.h)"""
    __slots__ = ("stat", "styles", "gammas", "betas", "eps")

    def __init__(self, stat, styles, gammas, betas, eps):
        self.stat, self.styles, self.gammas, self.betas, self.eps = stat, styles, gammas, betas, float(eps)

    def fill(self, ref):
        ns = len(self.gammas) if self.gammas is not None else 1
        ref.stat, ref.styles, ref.num_styles, ref.eps = _ptr(self.stat), _ptr(self.styles), ns, self.eps
        ref.gamma, ref.beta = _style_arrays(self.gammas, ns), _style_arrays(self.betas, ns)


FOLD_NORMS = True      # False: the Swin block's norm apply / norm-backward reduce as launches of their own (the tests' reference path)
# the norm-backward sums in the epilogue of the SMALL-M data-gradient GEMM (<= 2048 rows: the deep Swin stages): the kernels have it (tested),
# the step does not use it - there the norm backward is ONE register-resident launch already, the fold would trade it for an apply launch
# (same launch count; measured 153.0 / 153.4 with it against 152.9 / 153.2 without: nothing); the forward folds stay on at every stage
SMALL_BSTAT = False


def gemm_nt_folds(a, w, anorm=None, bstat_x=None, act=L.ACT_NONE, res=None):
    """would gemm_nt(a, w, anorm=...) / gemm_nt(..., bstat=...) run fused for these operands?  (one sample is the caller's business)"""
    if not FOLD_NORMS or a.dtype != torch.bfloat16:
        return False
    lda, M, K = rows(a)
    N = w.shape[0]
    if bstat_x is not None and M <= 2048 and not SMALL_BSTAT:
        return False
    # (the output will be a fresh [M, N] tensor: A's pointer stands in for its alignment, and for the not-yet-allocated statistics)
    p = L.Gemm(_ptr(a), lda, _ptr(w), K, _ptr(a), N, M, N, K, 0, 0, _dt(a), _dt(a), None, act, 0, 1, None, _ptr(res), rows(res)[0] if res is not None else 0, None, 0, 0, 0, None)
    if anorm is not None:
        anorm.fill(p.an)
        return bool(L.load().miseg_gemm_fuses_anorm(C.byref(p)))
    p.stat, p.stat_mode, p.bs_x, p.ld_bs_x, p.bs_stat = _ptr(a), 2, _ptr(bstat_x), rows(bstat_x)[0], _ptr(a)
    return bool(L.load().miseg_gemm_fuses_bstat(C.byref(p)))


def gemm_nt(a, w, bias=None, act=L.ACT_NONE, out=None, out_dtype=None, split_k=1, res=None, preact_out=None, gelu_grad_of=None, want_stat=False, anorm=None,
            anorm_out=False, bstat=None):
    """out[M,N] = act(a[M,K] @ w[N,K]^T + bias) + res ; a rows view, w contiguous [N,K] in a.dtype.
    preact_out: tensor that receives the pre-activation z (for a later GELU backward); gelu_grad_of: pre-activation h of the
    layer in front, the result is multiplied by gelu'(h) (GELU backward folded into this data-gradient GEMM).
    anorm (NormRef; check gemm_nt_folds first): `a` is the RAW input of that instance norm, normalised as it is loaded; anorm_out: also return
    norm(a) - result (out, norm_a).  bstat = (x, stat, eps): `out` is the gradient with respect to the output of the instance norm whose raw
    input is x (forward statistics `stat`); its backward sums are left for pop_gemm_stat(out) (dstat layout of instnorm_bwd)."""
    lda, M, K = rows(a)
    N, Kw = w.shape
    if not (Kw == K and w.is_contiguous() and w.dtype == a.dtype):
        raise ValueError(f"gemm_nt: weight {tuple(w.shape)} {w.dtype} does not match activations K={K} {a.dtype}")
    odt = out_dtype or a.dtype
    if out is None:
        out = torch.empty(a.shape[:-1] + (N,), dtype=odt, device=a.device)
    ldc, Mo, No = rows(out)
    assert Mo == M and No == N
    assert preact_out is None or gelu_grad_of is None
    aux = preact_out if preact_out is not None else gelu_grad_of
    for t in (res, aux):
        if t is not None:
            _, Mt, Nt = rows(t)
            if Mt != M or Nt != N or t.dtype != out.dtype:
                raise ValueError("gemm_nt: res / aux must be [M, N] row views in the output dtype")
    p = L.Gemm(_ptr(a), lda, _ptr(w), K, _ptr(out), ldc, M, N, K, 0, 0, _dt(a), _dt(out), _ptr(_fp32(bias)), act, 0, split_k, None,
               _ptr(res), rows(res)[0] if res is not None else 0, _ptr(aux), rows(aux)[0] if aux is not None else 0,
               1 if preact_out is not None else 2 if gelu_grad_of is not None else 0, 0, None)
    _set_gemm_stat(None, None)
    xn = None
    if anorm is not None:
        assert not want_stat and bstat is None
        anorm.fill(p.an)
        if anorm_out:
            xn = torch.empty(a.shape, dtype=a.dtype, device=a.device)
            p.an_out, p.ld_an_out = xn.data_ptr(), rows(xn)[0]
    if bstat is not None:
        assert not want_stat
        bx, bst, beps = bstat
        dstat = STAT_POOL.take(L.load().miseg_instnorm_stat_bytes(1, N) // 8, a.device)
        p.stat, p.stat_mode, p.bs_x, p.ld_bs_x, p.bs_stat, p.bs_eps = dstat.data_ptr(), 2, _ptr(bx), rows(bx)[0], _ptr(bst), float(beps)
        _set_gemm_stat(out, dstat)
    if want_stat and L.load().miseg_gemm_fuses_stat(C.byref(p)):
        # all M rows are one sample (the caller checked): the kernel leaves the norm statistics of the output in `stat`
        stat = STAT_POOL.take(L.load().miseg_instnorm_stat_bytes(1, N) // 8, a.device).view(-1, 1, N, 2)
        p.stat = stat.data_ptr()
        _set_gemm_stat(out, stat)
    _call("miseg_gemm", p, prof=("gemm_nt", 2.0 * M * N * K, _nb(a, w, out, res, aux, xn, bstat[0] if bstat is not None else None)))      # (no accumulating output on the NT side: repeatable)
    return (out, xn) if anorm_out else out


def mlp_fused(x, hid):
    """the fused MLP kernels take this problem (bf16, 48 -> 192 -> 48 channels, >= 4096 tokens)"""
    _, M, Cc = rows(x)
    return x.dtype == torch.bfloat16 and bool(L.load().miseg_mlp_fused(M, Cc, hid, _dt(x)))


def mlp_fwd(x, w1, b1, w2, b2, res=None, want_stat=False, anorm=None, anorm_out=False):
    """y = w2 gelu(w1 x + b1) + b2 (+ res) in one launch, hidden activations never stored; w1 [HID, C], w2 [C, HID] contiguous in x.dtype.
    want_stat (all rows one sample): the instance-norm statistics of y are left for pop_gemm_stat(y).
    anorm (NormRef): x is the RAW input of that instance norm (one sample), normalised as it is loaded; anorm_out: also return norm(x)."""
    ldx, M, Cc = rows(x)
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    p = L.Mlp(C.sizeof(L.Mlp), M, Cc, w1.shape[0], _dt(x), _ptr(x), ldx, _ptr(w1), _ptr(_fp32(b1)), _ptr(w2), _ptr(_fp32(b2)),
              _ptr(res), rows(res)[0] if res is not None else 0, _ptr(y), rows(y)[0], None)
    xn = None
    if anorm is not None:
        anorm.fill(p.an)
        if anorm_out:
            xn = torch.empty(x.shape, dtype=x.dtype, device=x.device)
            p.an_out, p.ld_an_out = xn.data_ptr(), rows(xn)[0]
    _set_gemm_stat(None, None)
    if want_stat:
        stat = STAT_POOL.take(L.load().miseg_instnorm_stat_bytes(1, Cc) // 8, x.device).view(-1, 1, Cc, 2)
        p.stat = stat.data_ptr()
        _set_gemm_stat(y, stat)
    _call("miseg_mlp_fwd", p, prof=("gemm_nt", 4.0 * M * Cc * w1.shape[0], _nb(x, y, res, xn)))
    return (y, xn) if anorm_out else y


def mlp_bwd(x, dy, w1, b1, w2t, w1t, need_dx=True, bstat=None):
    """(dz, h, dx) of the fused MLP: dz = (dy w2) * gelu'(z), h = gelu(z) with z = w1 x + b1 recomputed, dx = dz w1.
    w2t [HID, C] = w2 transposed, w1t [C, HID] = w1 transposed (cast_matrix(..., transpose=True)).
    bstat = (x_raw, stat, eps): x is norm(x_raw); dx is the gradient with respect to that norm's output and its backward sums come back as a
    fourth result (dstat layout of instnorm_bwd)."""
    ldx, M, Cc = rows(x)
    hid = w1.shape[0]
    dz = torch.empty(x.shape[:-1] + (hid,), dtype=x.dtype, device=x.device)
    h = torch.empty_like(dz)
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device) if need_dx else None
    p = L.Mlp(C.sizeof(L.Mlp), M, Cc, hid, _dt(x), _ptr(x), ldx, _ptr(w1), _ptr(_fp32(b1)), None, None, None, 0, None, 0, None,
              _ptr(dy), rows(dy)[0], _ptr(w2t), _ptr(w1t), _ptr(dz), rows(dz)[0], _ptr(h), rows(h)[0], _ptr(dx), rows(dx)[0] if dx is not None else 0)
    dstat = None
    if bstat is not None and dx is not None:
        bx, bst, beps = bstat
        dstat = STAT_POOL.take(L.load().miseg_instnorm_stat_bytes(1, Cc) // 8, x.device)
        p.bs_x, p.ld_bs_x, p.bs_stat, p.bs_eps, p.bs_dstat = _ptr(bx), rows(bx)[0], _ptr(bst), float(beps), dstat.data_ptr()
    _call("miseg_mlp_bwd", p, prof=("gemm_nt", 8.0 * M * Cc * hid, _nb(x, dy, dz, h, dx)))
    return (dz, h, dx, dstat) if bstat is not None else (dz, h, dx)


def gemm_nt_scatter(a, w, dst, grid):
    """The GEMM of a ConvTranspose3d(k2, s2) with its 2x2x2 scatter as the store: a = the voxels of `grid` = (B, d, h, w) as rows [.., Cin],
    w = [(j, co)][ci] (j = 4 jd + 2 jh + jw), dst = rows view [B, 2d, 2h, 2w, co] (e.g. the left half of a concat buffer).
    Returns False where the kernel path has no scattered store (caller: gemm_nt + channel_to_space)."""
    lda, M, K = rows(a)
    N, Kw = w.shape
    ldc, Md, Cout = rows(dst)
    B, d, h, wd = grid
    if not (Kw == K and w.is_contiguous() and w.dtype == a.dtype and dst.dtype == a.dtype and N == 8 * Cout and Md == 8 * M and M == B * d * h * wd):
        raise ValueError("gemm_nt_scatter: operand shapes")
    p = L.Gemm(_ptr(a), lda, _ptr(w), K, _ptr(dst), ldc, M, N, K, 0, 0, _dt(a), _dt(dst), None, L.ACT_NONE, 0, 1, None, None, 0, None, 0, 0, 0, None,
               d, h, wd, Cout)
    if not L.load().miseg_gemm_fuses_scatter(C.byref(p)):
        return False
    _call("miseg_gemm", p)
    return True


def gemm_tn_regroups(a, b, out):
    """can gemm_tn(a, b, out, accumulate=..., regroup=...) run for these operands?  (needs a step queue: the regrouped store lives in the
    grouped launch / the batched partial-tile sum at the end of the backward pass)"""
    if _queues(out) is None:
        return False
    lda, K, M = rows(a)
    N = rows(b)[2]
    p = L.Gemm(_ptr(a), lda, _ptr(b), rows(b)[0], _ptr(out), N, M, N, K, 1, 1, _dt(a), L.F32, None, L.ACT_NONE, 1, 0, None, None, 0, None, 0, 0, 0)
    splits = L.load().miseg_gemm_tn_splits(C.byref(p))
    return splits == 0 or splits > 1      # grouped launch (no streaming kernel), or streaming kernel with partial tiles: their deferred sum regroups


def gemm_tn(a, b, out=None, accumulate=False, split_k=0, regroup=0, colsum_out=None):
    """out[M,N] (fp32) (+)= a[K,M]^T @ b[K,N]; a, b row views sharing the row count K (weight gradients).
    regroup = c > 0 (accumulate mode, after gemm_tn_regroups said yes): column j * c + i of the product is stored at column i * (N / c) + j.
    colsum_out (fp32 [M], accumulate mode): += the column sums of a - with a = dy the bias gradient of the linear layer whose weight gradient
    this is.  On the streaming path they ride in the product's launch (miseg_gemm_params.tn_colsum); elsewhere this is colsum(a, colsum_out,
    accumulate=True)."""
    lda, K, M = rows(a)
    ldb, Kb, N = rows(b)
    assert K == Kb and a.dtype == b.dtype
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
        accumulate = False
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == M * N
    q = _queues(out) if accumulate else None
    assert not regroup or (q is not None and split_k <= 0 and N % regroup == 0)
    if q is not None:
        q.writes[out.data_ptr()] = q.writes.get(out.data_ptr(), 0) + 1      # step-wide writer count of the slot (direct and queued, main and side)
    split_k = max(0, split_k)          # 0: the library picks the kernel and the split over the reduction rows
    # (the direct kernels always add: "known zero" only saves the grouped launch its read of the slot)
    p = L.Gemm(_ptr(a), lda, _ptr(b), ldb, _ptr(out), N, M, N, K, 1, 1, _dt(a), L.F32, None, L.ACT_NONE, int(bool(accumulate)), split_k, None, None, 0, None, 0, 0, 0)
    lib = L.load()
    if q is not None and split_k == 0 and lib.miseg_gemm_tn_splits(C.byref(p)) == 0:
        q.lists().gemm_tn.append((a, b, out, int(accumulate) == 2, int(regroup)))      # no streaming kernel: grouped launch at the end of the backward pass
        if colsum_out is not None:
            colsum(a, colsum_out, accumulate=True)
        return out
    if q is not None and TN_STREAM_GROUP and split_k == 0:
        # the streaming kernel: the product waits for the other tall products of its block and shares ONE launch with them (tn_stream_close)
        cs = None
        if colsum_out is not None:
            if colsum_out.dtype == torch.float32:
                cs = colsum_out
            else:
                colsum(a, colsum_out, accumulate=True)
        _tn_stream_enqueue(q.lists(), (a, b, out, int(accumulate), int(regroup), cs))
        return out
    if colsum_out is not None:
        if split_k == 0 and colsum_out.dtype == torch.float32 and lib.miseg_gemm_tn_fuses_colsum(C.byref(p)):
            p.tn_colsum = colsum_out.data_ptr()
        else:
            colsum(a, colsum_out, accumulate=True)
    wsb = lib.miseg_gemm_workspace_bytes(C.byref(p))
    if wsb:
        ws = torch.empty(wsb // 4, dtype=torch.float32, device=a.device)
        p.workspace = ws.data_ptr()
        if q is not None:      # the per-split partial tiles are summed by one batched launch later
            p.defer_reduce = 1
            q.lists().tn_reduce.append((ws, out, N, M, N, lib.miseg_gemm_tn_splits(C.byref(p)), int(regroup)))
    assert not regroup or p.defer_reduce, "gemm_tn: regroup on a path without a deferred sum (ask gemm_tn_regroups first)"
    _call("miseg_gemm", p)
    return out


TN_STREAM_GROUP = True           # False: every streaming TN product is a launch of its own where it is issued (the tests' reference path)
TN_STREAM_GROUP_LAUNCHES = 0     # running count of grouped streaming launches (one per closed group)


def tn_stream_group_launch(items, reduces):
    """ONE launch for up to lib.TN_STREAM_GROUP_CAP streaming TN products on the current stream.  items: (a, b, out, accumulate, regroup,
    colsum_out) as gemm_tn takes them (accumulate 0: out is overwritten); every product the plan splits - and every regrouped one - leaves its
    partial tiles to the batched sum: one (ws, out, ldc, M, N, splits, regroup) entry is appended to `reduces` for each (_flush_tn_reduces)."""
    global TN_STREAM_GROUP_LAUNCHES
    lib = L.load()
    n = len(items)
    descs, plans = (L.GemmTnStreamDesc * n)(), (L.GemmTnStreamPlan * n)()
    shapes = []
    for j, (a, b, out, acc, regroup, cs) in enumerate(items):
        lda, K, M = rows(a)
        ldb, _, N = rows(b)
        descs[j] = L.GemmTnStreamDesc(_ptr(a), lda, _ptr(b), ldb, _ptr(out), N, None, _ptr(cs), M, N, K, 1 if acc else 0)
        shapes.append((M, N, K))
    L.check(lib.miseg_gemm_tn_stream_group_plan(descs, n, plans), "gemm_tn_stream_group_plan")
    for j, (a, b, out, acc, regroup, cs) in enumerate(items):
        M, N, K = shapes[j]
        if plans[j].splits > 1 or regroup:
            ws = torch.empty(plans[j].splits * M * N, dtype=torch.float32, device=a.device)
            descs[j].partial = ws.data_ptr()
            if not acc:
                fill32(out)          # the batched sum adds
            reduces.append((ws, out, N, M, N, plans[j].splits, int(regroup)))
    fl = sum(2.0 * M * N * K for M, N, K in shapes)
    nb = sum(2.0 * K * (M + N) + 4.0 * M * N * plans[j].splits for j, (M, N, K) in enumerate(shapes))
    with _ProfRegion("gemm_tn_stream_group", fl, nb):
        L.check(lib.miseg_gemm_tn_stream_group(descs, n, _stream()), "gemm_tn_stream_group")
    _stamp_launch("gemm_tn_stream_group")
    TN_STREAM_GROUP_LAUNCHES += 1


def _tn_stream_enqueue(lst, item):
    cur = torch.cuda.current_stream()
    if lst.tn_stream and lst.tn_stream_on != cur:      # a group never mixes products issued on different streams
        _close_tn_stream(lst)
    lst.tn_stream_on = cur
    lst.tn_stream.append(item)
    if len(lst.tn_stream) >= L.TN_STREAM_GROUP_CAP:
        _close_tn_stream(lst)


def _close_tn_stream(lst):
    """plan and issue the open group of `lst` (a StepQueues or its side queue) on the stream its products were issued on"""
    if lst is None or not lst.tn_stream:
        return
    items = list(lst.tn_stream)
    lst.tn_stream.clear()
    on, lst.tn_stream_on = lst.tn_stream_on, None
    if on != torch.cuda.current_stream():
        with torch.cuda.stream(on):
            tn_stream_group_launch(items, lst.tn_reduce)
    else:
        tn_stream_group_launch(items, lst.tn_reduce)


def _all_queues():
    return list(QUEUES.values()) + ([DEFAULT_QUEUES] if DEFAULT_QUEUES is not None else [])


def tn_stream_close():
    """the backward pass leaves a block: its queued streaming weight-gradient products go out now, as one launch, where they are in the
    chain - leaf work never piles into the tail and the queued operands live no longer than one block"""
    for q in _all_queues():
        _close_tn_stream(q.lists())


def permute3(src, dst, n, strides, accumulate=False):
    lib = L.load()
    L.check(lib.miseg_permute3(_ptr(src), _ptr(dst), n[0], n[1], n[2], strides[0], strides[1], strides[2], int(accumulate), _stream()), "permute3")
    return dst


_WGRAD_KEEP = []      # operands of branch-stream launches, kept alive until the join (join_wgrad)
_BRANCH_STREAM = None
BACKGROUND_LAUNCHES = 0        # running count of launches issued in background form (bench.py reports the per-step figure)
BACKGROUND_WORKGROUPS = 32     # cap of the branch's own background weight-gradient launch (each workgroup owns a CU).  Step against no branch,
                               # two boxes, before the deferral below: 256 (no cap) -0.4 %, 128 +1.0, 64 +1.4, 32 +2.0 / +2.4, 16 +2.0, 8 -3.8
DEFERRED_WORKGROUPS = 64       # cap of the main stream's deferred weight gradients (defer_to_branch).  (own cap, this cap) on one box, no branch =
                               # 132.6, branch alone 134.5: (24, 48) 136.9, (24, 64) 140.8, (24, 96) 139.8, (48, 64) 140.6, (64, 64) 140.7, (32, 32) 128.9
DEFERRED_WORKGROUPS_SPLIT = 96      # the same launches inside the first half of a split step (flush_deferred_on_branch)
DEFER_MIN_ROWS = 400000        # 96^3 layers only (the smaller ones are grouped into one launch at the end of the backward pass)
# (round 3: the queue of deferred launches itself lives on the training arena's StepQueues - `branch_deferred` - and is found through the
# gradient slot a launch accumulates into, like the other per-step queues: two models in one process no longer share it)


def branch_stream(device):
    """the stream of a model's side branch (SwinUNETR: the two image-resolution encoder blocks).  Autograd replays the branch's backward
    pass on it - beside the latency-bound launches of the deep stages - and `join_branch` joins it."""
    global _BRANCH_STREAM
    if _BRANCH_STREAM is None or _BRANCH_STREAM.device != device:
        _BRANCH_STREAM = torch.cuda.Stream(device=device)
    return _BRANCH_STREAM


def open_branch_deferral(params):
    """a model's forward opens the deferral for this step: full-size conv weight gradients of the MAIN stream (SwinUNETR: decoder1's two 96^3
    layers) wait for the side branch's backward pass and run at its head, in background form.  Needs a training arena (the queue lives on
    its StepQueues); returns False without one."""
    q = _arena_queues(params)
    if q is None:
        return False
    q.branch_deferred = []
    return True


def close_branch_deferral(params):
    q = _arena_queues(params)
    if q is not None:
        q.branch_deferred = None


def _arena_queues(params):
    for p in params:
        arena = getattr(p, "_miseg_arena", None)
        return QUEUES.get(arena._qkey) if arena is not None else None
    return None


def defer_to_branch(x, dy, slot, mode):
    """True when the conv weight gradient (x, dy) -> slot was queued for the head of the side branch's backward pass: leaf work of the main
    stream's full-size kernels (0.3 ms per step on the critical path) that then runs beside the small-grid launches instead"""
    q = _queues(slot)
    if q is None or q.branch_deferred is None or in_branch_backward() or rows(x)[1] < DEFER_MIN_ROWS:
        return False
    q.branch_deferred.append((x, dy, slot, mode))
    return True


def flush_branch_deferred(q, cap=None):
    """launch what `defer_to_branch` queued on the current stream (the branch's, in background form; join_branch's as a fallback)"""
    global BACKGROUND_WORKGROUPS
    if q is None or not q.branch_deferred:
        if q is not None:
            q.branch_deferred = None
        return
    items, q.branch_deferred = q.branch_deferred, None
    keep, BACKGROUND_WORKGROUPS = BACKGROUND_WORKGROUPS, (cap or DEFERRED_WORKGROUPS)
    try:
        for x, dy, slot, mode in items:
            conv3_wgrad(x, dy, dw=slot, accumulate=mode)
    finally:
        BACKGROUND_WORKGROUPS = keep
    _WGRAD_KEEP.extend(t for it in items for t in it[:2])      # alive until join_wgrad



def flush_deferred_on_branch(params):
    """(gradient hook) issue what defer_to_branch queued so far on the BRANCH stream, behind everything the main stream has issued (see
    SwinUNETR.forward: the first half of a split step)"""
    q = _arena_queues(params)
    if q is None or not q.branch_deferred or _BRANCH_STREAM is None:
        return
    cur = torch.cuda.current_stream()
    if cur == _BRANCH_STREAM:
        return
    _BRANCH_STREAM.wait_stream(cur)
    with torch.cuda.stream(_BRANCH_STREAM):
        # (alone on the branch stream, with ~0.8 ms of the main stream's decoder chain to hide behind: 96 workgroups finish in time where
        # the one-graph step's 64 left the first half waiting - single-rank RCCL step 135.4 / 138.5 / 138.1 / 137.1 patches/s at 64 / 96 / 128 / 192)
        flush_branch_deferred(q, cap=DEFERRED_WORKGROUPS_SPLIT)


def join_branch(flush_deferred=True, queues=None, flush_main=False):
    """the current stream waits for the branch stream: before anything that consumes what the branch's backward produced (the side queue's
    launches of arena.end_backward, the optimiser, the end of a hipGraph capture).  queues: the arena's StepQueues whose
    deferred launches are issued here when the branch's backward never ran (nothing in it needed a gradient).
    flush_main: the main stream's own queued launches go out BEFORE the wait (they read nothing of the branch's).
    The branch stream is forked once (the model's forward) and joined once (here), and the end-of-pass launches below ride behind its last
    kernel: one fork and one join per side stream is what a captured step replays concurrently.  A second edge main -> branch inside the
    step (round 3: the grouped conv weight gradients issued early, at the tail of the branch's backward pass, behind a wait for the main
    stream) made the hipGraph executor run the WHOLE branch behind the main stream's segment, 146.5 -> 114.0 patches/s, and so did a third
    stream forked for that launch (147 -> 118)."""
    global _FLUSHING
    for q in ([queues] if queues is not None else _all_queues()):      # an open group goes out on its own stream, in front of the sums of its partial tiles
        _close_tn_stream(q)
        _close_tn_stream(q.side)
    if flush_deferred:
        for q in ([queues] if queues is not None else list(QUEUES.values())):
            if q.branch_deferred:
                flush_branch_deferred(q)
    stamp("main_chain_end")
    _FLUSHING = True
    if flush_main and queues is not None:
        cur = torch.cuda.current_stream() if _BRANCH_STREAM is not None else None      # (no side stream: the CPU ranks of the gloo tests)
        if queues.side is not None and _BRANCH_STREAM is not None and cur != _BRANCH_STREAM:
            # what the branch's backward queued goes out on the BRANCH stream, behind its last kernel: the branch ends ~0.3 ms before the main
            # chain (step stamps), so these launches run beside the main stream's last kernels instead of behind the join.  The main stream's
            # grouped GEMM weight gradients, partial-tile sums and column sums follow them there (after a wait for the main chain), beside
            # the main stream's grouped conv weight gradients: that launch holds one 96 KB workgroup per CU and leaves the rest of the CU idle
            with torch.cuda.stream(_BRANCH_STREAM):
                queues.side.flush()
            if queues.gemm_tn or queues.tn_reduce or queues.colsum:
                for lst in (queues.gemm_tn, queues.tn_reduce, queues.colsum):      # operands of the main stream, read on the branch: alive until join_wgrad
                    _WGRAD_KEEP.extend(t for it in lst for t in it if isinstance(t, torch.Tensor))
                _BRANCH_STREAM.wait_stream(cur)
                with torch.cuda.stream(_BRANCH_STREAM):
                    _flush_gemm_tn(queues.gemm_tn, queues.writes)
                    _flush_tn_reduces(queues.tn_reduce)
                    _flush_colsums(queues.colsum)
            if queues.on_branch_end is not None and cur != _BRANCH_STREAM:
                # round 5 (runtime/graph.py::GraphedTrainStep): work that only needs what the main CHAIN has produced - the optimiser update of the
                # parameters whose gradients were written inline (StepQueues.inline_final) - goes out on the branch stream here, beside the
                # main stream's grouped launches below, instead of behind the whole pass
                _BRANCH_STREAM.wait_stream(cur)
                with torch.cuda.stream(_BRANCH_STREAM):
                    queues.on_branch_end()
        queues.flush(side=False)
        stamp("main_flushed")
    if _BRANCH_STREAM is not None:
        if STAMPS is not None and not torch.cuda.current_stream() == _BRANCH_STREAM:
            stamp("branch_end", _BRANCH_STREAM)
        torch.cuda.current_stream().wait_stream(_BRANCH_STREAM)
        stamp("joined")
    _FLUSHING = False


def in_branch_backward():
    return _BRANCH_STREAM is not None and torch._C._current_graph_task_id() >= 0 and torch.cuda.current_stream() == _BRANCH_STREAM


def _background():
    """> 0 (the workgroup cap) when this launch belongs to the branch's BACKWARD pass: the 3x3x3 convolution kernels then run in their
    background form (miseg_conv3_params.background, miseg_conv3_wgrad_params.max_workgroups) so that the main stream's small-grid
    launches keep finding free CUs.  The branch's forward runs right in front of its join, beside nothing: normal form."""
    if not in_branch_backward():
        return 0
    global BACKGROUND_LAUNCHES
    BACKGROUND_LAUNCHES += 1
    return BACKGROUND_WORKGROUPS


def join_wgrad():
    """the current stream waits for the branch stream; call once after the backward pass (arena.end_backward)."""
    join_branch()
    _WGRAD_KEEP.clear()


class StepQueues:
    """launch-bound tails of ONE model's backward pass, queued by the host and issued as grouped launches at the end of it
    (runtime/arena.py::end_backward): bias-gradient column sums, the small weight-gradient GEMMs, the partial-tile sums of the
    streaming ones, the conv weight gradients of the 48^3-and-smaller layers - and, block by block DURING the pass, the open group of
    streaming weight-gradient GEMMs (tn_stream: one launch per block, tn_stream_close).  One instance per training arena, found through the
    storage of the gradient slot a kernel accumulates into - two models (two arenas) in one process do not share anything."""

    def __init__(self, side=True, writes=None):
        self.colsum, self.gemm_tn, self.tn_reduce, self.conv_wgrad = [], [], [], []
        self.tn_stream, self.tn_stream_on = [], None      # the open group of streaming TN products (gemm_tn / tn_stream_close) and the stream they were issued on
        self.unzeroed = set()        # data_ptr of arena slots the step's fill left out (their weight-gradient kernel overwrites them whole: arena.begin_step);
                                     # conv3_wgrad zero-fills one first if the launch it is about to issue would read or only add to it
        self.inline_final = []       # arena slots whose ONLY write of the step happened inline, as a plain store (the tiny-volume conv weight gradients):
                                     # final as soon as the main chain of the backward pass is through
        self.on_branch_end = None    # callable issued on the branch stream where join_branch sends the end-of-pass small launches (see there)
        # gradient slot (data_ptr) -> how many weight-gradient GEMMs of this step write it, direct launches and both queues together: a
        # grouped launch may STORE into a slot ("known zero", miseg_gemm_tn_desc.zeroed) only when it is the slot's one writer of the step -
        # a tied weight's second use, wherever it was issued, would otherwise be overwritten or overwrite
        self.writes = {} if writes is None else writes
        self.branch_deferred = None      # while the model's side branch is open: [(x, dy, slot, mode)], see defer_to_branch
        # what the side branch's backward pass queues (it reads tensors the BRANCH stream produced) is kept apart: the main stream issues
        # its own grouped launches as soon as its chain ends - beside the branch's last full-size kernels, which run in background form on
        # a fraction of the CUs - and only the branch's few wait for the join (arena.end_backward)
        self.side = StepQueues(side=False, writes=self.writes) if side else None

    def lists(self):
        """the queue a launch issued NOW belongs to"""
        return self.side if (self.side is not None and in_branch_backward()) else self

    def flush_small(self):
        """the queued GEMM weight gradients, partial-tile sums and column sums only (the grouped conv weight gradients keep waiting): what
        completes the small parameters of a range whose conv weights were written inline (tiny-volume layers), cheaply, mid-chain"""
        _close_tn_stream(self)
        _flush_gemm_tn(self.gemm_tn, self.writes)
        _flush_tn_reduces(self.tn_reduce)
        _flush_colsums(self.colsum)

    def flush(self, side=True):
        _close_tn_stream(self)
        _flush_conv_wgrads(self.conv_wgrad)
        _flush_gemm_tn(self.gemm_tn, self.writes)
        _flush_tn_reduces(self.tn_reduce)
        _flush_colsums(self.colsum)
        if side and self.side is not None:
            self.side.flush()


QUEUES = {}             # data_ptr of an arena's flat gradient storage -> its StepQueues while a step of that arena is open
DEFAULT_QUEUES = None   # tests / micro-benchmarks: queue accumulate-mode launches whose destination belongs to no arena


def _queues(out):
    if out is None:
        return None
    if QUEUES:
        q = QUEUES.get(out.untyped_storage().data_ptr())
        if q is not None:
            return q
    return DEFAULT_QUEUES


def _flush_tn_reduces(q):
    if not q:
        return
    lib = L.load()
    for i in range(0, len(q), 32):
        chunk = q[i:i + 32]
        descs = (L.TnReduceDesc * len(chunk))()
        for j, (ws, out, ldc, M, N, splits, regroup) in enumerate(chunk):
            descs[j] = L.TnReduceDesc(_ptr(ws), _ptr(out), ldc, M, N, splits, 0, regroup, 0)
        L.check(lib.miseg_gemm_tn_reduce_batch(descs, len(chunk), _stream()), "gemm_tn_reduce_batch")
        _stamp_launch("gemm_tn_reduce_batch")
    q.clear()


def _flush_gemm_tn(q, writes=None):
    if not q:
        return
    lib = L.load()
    once = writes
    if once is None:      # (no step-wide count: at least the problems of this launch)
        once = {}
        for it in q:      # a slot written by two problems of the same launch (a shared weight) is never "known zero" for either
            once[it[2].data_ptr()] = once.get(it[2].data_ptr(), 0) + 1
    for dt in {it[0].dtype for it in q}:
        items = [it for it in q if it[0].dtype == dt]
        for i in range(0, len(items), 24):
            chunk = items[i:i + 24]
            descs = (L.GemmTnDesc * len(chunk))()
            for j, (a, b, out, zeroed, regroup) in enumerate(chunk):
                lda, K, M = rows(a)
                ldb, _, N = rows(b)
                descs[j] = L.GemmTnDesc(_ptr(a), lda, _ptr(b), ldb, _ptr(out), N, M, N, K, 1 if (zeroed and once.get(out.data_ptr(), 2) == 1) else 0, regroup, 0)
            L.check(lib.miseg_gemm_tn_group(descs, len(chunk), _dt(chunk[0][0]), _stream()), "gemm_tn_group")
            _stamp_launch("gemm_tn_group")
    q.clear()


def _flush_colsums(q):
    """issue the queued accumulate-mode column sums in batches of lib.MISEG_COLSUM_BATCH (one launch each)."""
    if not q:
        return
    lib = L.load()
    for dt in {t.dtype for t, _ in q}:
        items = [(t, o) for t, o in q if t.dtype == dt]
        for i in range(0, len(items), 32):
            chunk = items[i:i + 32]
            descs = (L.ColsumDesc * len(chunk))()
            for j, (t, o) in enumerate(chunk):
                ld, n, Cc = rows(t)
                descs[j] = L.ColsumDesc(_ptr(t), ld, n, _ptr(o), Cc, 0)
            L.check(lib.miseg_colsum_batch(descs, len(chunk), _dt(chunk[0][0]), _stream()), "colsum_batch")
            _stamp_launch("colsum_batch")
    q.clear()


def colsum(x, out=None, accumulate=False):
    ld, n, Cc = rows(x)
    q = _queues(out) if (out is not None and accumulate) else None
    if q is not None:
        q.lists().colsum.append((x, out))          # keeps x alive until the flush
        return out
    if out is None:
        out = torch.empty(Cc, dtype=torch.float32, device=x.device)
        accumulate = False
    _call("miseg_colsum", L.Colsum(_ptr(x), ld, n, Cc, _dt(x), _ptr(out), int(accumulate)))
    return out


def cast_matrix(w, dtype, transpose=False, regroup=None):
    """fp32 [R, C] parameter -> compute dtype, optionally transposed to [C, R].  regroup=(inner, outer) additionally
    renumbers the C index c -> (c % inner) * outer + c // inner (ConvTranspose3d k2s2 weights: (co, tap) -> (tap, co)).
    With a training arena (runtime/arena.py) the result is the copy refreshed by the step's batched kernel."""
    inner, outer = regroup if regroup is not None else (1, 1)
    if dtype == torch.float32 and not transpose and inner == 1:
        return _fp32(w).reshape(w.shape[0], -1)
    arena = getattr(w, "_miseg_arena", None)
    if arena is not None and arena.dtype == dtype:
        sh = arena.shadow(w, transpose, inner, outer)
        if sh is not None:
            return sh
    w2 = _fp32(w).reshape(w.shape[0], -1)
    R, Cc = w2.shape
    if inner != 1:
        # one-off path (first step / no arena): regroup in fp32 with the permute kernel, then cast
        tmp = torch.empty((Cc, R) if transpose else (R, Cc), dtype=torch.float32, device=w.device)
        if transpose:   # tmp[(j, o)][r] = w2[r][o * inner + j]
            permute3(w2, tmp, (inner, outer, R), (1, inner, Cc))
        else:           # tmp[r][(j, o)] = w2[r][o * inner + j]
            permute3(w2, tmp, (R, inner, outer), (Cc, 1, inner))
        if dtype == torch.float32:
            return tmp
        w2, transpose = tmp, False
        R, Cc = w2.shape
    out = torch.empty((Cc, R) if transpose else (R, Cc), dtype=dtype, device=w.device)
    _call("miseg_cast_matrix", L.Cast(_ptr(w2), _ptr(out), R, Cc, L.F32 if dtype == torch.float32 else L.BF16, int(transpose)))
    return out


# ------------------------------------------------------------------------------------------ conv 3x3x3
def pack_conv3(w, dtype, want_fwd=True, want_bwd=True):
    """packs of a 3x3x3 weight for the forward (x side) and data-gradient (dy side) kernels; with a training arena the
    packs refreshed by the step's batched kernel (runtime/arena.py)."""
    arena = getattr(w, "_miseg_arena", None)
    if arena is not None and arena.dtype == dtype:
        pk = arena.conv_packs(w)
        if pk is not None:
            return pk
    Cout, Cin = w.shape[0], w.shape[1]
    lib = L.load()
    dt = L.F32 if dtype == torch.float32 else L.BF16
    fwd = torch.empty(lib.miseg_pack_conv3_elems(Cin, Cout, dt, 0), dtype=dtype, device=w.device) if want_fwd else None
    bwd = torch.empty(lib.miseg_pack_conv3_elems(Cin, Cout, dt, 1), dtype=dtype, device=w.device) if want_bwd else None
    _call("miseg_pack_conv3_weight", L.PackConv3(_ptr(_fp32(w)), _ptr(fwd), _ptr(bwd), Cin, Cout, dt))
    return fwd, bwd


def _vol(x):
    assert x.dim() == 5, "expected [B, D, H, W, C]"
    return x.shape[0], x.shape[1], x.shape[2], x.shape[3]


def _pending():
    """this thread's table: key of a data gradient whose split convolution left its slabs to the norm backward that consumes it -> PendingSlabs"""
    d = getattr(_TLS, "pending", None)
    if d is None:
        d = _TLS.pending = {}
        with _ALL_PENDING_LOCK:
            _ALL_PENDING.append(d)
    return d


def pending_dx_put(dx, pend):
    _pending()[(dx.data_ptr(), dx.numel(), dx.dtype)] = pend


def pending_dx_take(dy):
    d = getattr(_TLS, "pending", None)
    return d.pop((dy.data_ptr(), dy.numel(), dy.dtype), None) if d else None


def check_no_pending():
    """every deferred slab sum must have been taken by its consumer (the instance-norm backward right behind the data-gradient convolution):
    a gradient tensor that reached anything else would have been read unwritten"""
    with _ALL_PENDING_LOCK:
        n = sum(len(d) for d in _ALL_PENDING)
        for d in _ALL_PENDING:
            d.clear()
    check_tn_stream_closed()
    if n:
        raise RuntimeError(f"{n} deferred data-gradient slab sum(s) were never consumed (conv3(..., dx_to_norm=True) in front of something that is no instance norm)")


def check_tn_stream_closed(queues=None):
    """no streaming weight-gradient product may still wait for its group's launch at the end of a pass (every flush closes the open group)"""
    for q in ([queues] if queues is not None else _all_queues()):
        n = len(q.tn_stream) + (len(q.side.tn_stream) if q.side is not None else 0)
        if n:
            q.tn_stream.clear()
            if q.side is not None:
                q.side.tn_stream.clear()
            raise RuntimeError(f"{n} streaming weight-gradient product(s) were queued and never launched (tn_stream_close / flush)")


FRESH = 256      # stand-in pointer of a buffer that is not allocated yet (fresh allocations are 256-byte aligned): the plans test pointers for NULL / alignment only


def _rows_ptr(t):
    """(pointer, ld, C, dtype) of a rows view; (like, C) stands for a fresh contiguous [B, D, H, W, C] tensor over like's volume"""
    return (FRESH, t[1], t[1], _dt(t[0])) if isinstance(t, tuple) else (_ptr(t), rows(t)[0], t.shape[-1], _dt(t))


def _plan(fn, p, plan):
    """the library's plan of a launch (miseg_conv3_fwd_plan / miseg_conv3_wgrad_plan / miseg_winattn_fwd_plan / _bwd_plan) from the launch's own params"""
    L.check(getattr(L.load(), fn)(C.byref(p), C.byref(plan)), fn)
    return plan


def conv3_fwd_plan(x, Cout, **pieces):
    """the plan (L.Conv3Plan) of conv3_fwd(x, ..., Cout) with these fields of miseg_conv3_params set (x: a tensor or a (like, C) stand-in)"""
    ptr, ld, Cin, dt = _rows_ptr(x)
    p = L.Conv3(ptr, ld, FRESH, Cout, FRESH, *_vol(x[0] if isinstance(x, tuple) else x), Cin, Cout, dt, **pieces)
    return _plan("miseg_conv3_fwd_plan", p, L.Conv3Plan())


def conv3_fuses_shortcut(x, Cout, g, w=None):
    """can conv3_fwd(x, ..., Cout, sc=(g, w)) take the 1x1x1 term along (miseg_conv3_params.sc_x)?  x: a tensor or a (like, C) stand-in;
    g: the [.., Csc] rows, or Csc for fresh ones; w: the [Cout, Csc] matrix, None for a fresh one"""
    gp, ldg, Csc, gdt = _rows_ptr((x[0] if isinstance(x, tuple) else x, g) if isinstance(g, int) else g)
    if gdt != _rows_ptr(x)[3] or (w is not None and not (w.is_contiguous() and _dt(w) == gdt)):
        return False
    return bool(conv3_fwd_plan(x, Cout, sc_x=gp, ld_sc_x=ldg, sc_w=_ptr(w) if w is not None else FRESH, sc_C=Csc).sc)


def conv3_fuses_s2c(x, Cout, C_left):
    """can conv3_fwd(x, ..., Cout, s2c=<a fresh tensor>) store its first C_left output channels in space-to-channel order (miseg_conv3_params.s2c_out)?"""
    return bool(conv3_fwd_plan(x, Cout, s2c_out=FRESH, s2c_C=C_left).s2c)


def conv3_fuses_fwd_shortcut(x, Cout, w=None):
    """can conv3_fwd(x, ..., Cout, fs=(w, ..)) produce the 1x1x1 convolution of x as a second output (miseg_conv3_params.fs_w)?  w: the
    [Cout, Cin] matrix, None for a fresh one"""
    if w is not None and not (w.is_contiguous() and w.dtype == x.dtype):
        return False
    return bool(conv3_fwd_plan(x, Cout, fs_w=_ptr(w) if w is not None else FRESH, fs_y=FRESH, ld_fs_y=Cout).fs)


def conv3_fwd(x, wpk, Cout, out=None, res=None, want_stat=False, defer=False, sc=None, s2c=None, fs=None):
    """x [B,D,H,W,Cin] rows view; wpk [Cout][27][CinP].  res: rows view added to the result in the epilogue (falls back to a separate
    add where the kernel path cannot fuse it).  want_stat: returns (out, stat) with stat the instance-norm statistics of `out`
    ([16, B, Cout, 2] fp64, from the kernel's epilogue) or None where that is not available (the caller's norm then computes them).
    sc = (g, w) (after conv3_fuses_shortcut said yes): out += g @ w^T, g a rows view over the same voxels, w [Cout, Csc] contiguous in x's
    dtype - the 1x1x1 shortcut term of a residual block's data gradient.
    s2c = tensor [B, D/2, H/2, W/2, 8 * C_left] (after conv3_fuses_s2c said yes): the first C_left output channels are stored THERE, in
    space-to-channel order (block j = 4 (d&1) + 2 (h&1) + (w&1)), and not in `out`.
    fs = (w [Cout, Cin] contiguous in x's dtype, want_stat2) (after conv3_fuses_fwd_shortcut said yes; not with defer): the launch also produces
    y2 = x @ w^T - a residual block's 1x1x1 shortcut convolution - and the return value is (out, stat | None, y2, stat2 | None)."""
    B, D, H, W = _vol(x)
    ld, n, Cin = rows(x)
    if out is None:
        out = torch.empty(B, D, H, W, Cout, dtype=x.dtype, device=x.device)
    ldy = rows(out)[0]
    lib = L.load()
    # want_stat == "defer" (the caller's next op is an instance norm that can take the partial slabs: instnorm_fwd_slabs): a split launch
    # over <= 2048 rows per sample stops after its slabs and the norm's ONE launch sums them, writes `out`, and normalises
    defer_req = bool(defer) or want_stat == "defer"      # (defer without want_stat: the data-gradient direction, returns (out, PendingSlabs | None))
    scx, scw, ldsc, Csc = None, None, 0, 0
    if sc is not None:
        scx, scw = sc
        ldsc, nsc, Csc = rows(scx)
        assert nsc == n and scw.is_contiguous() and tuple(scw.shape) == (Cout, Csc) and scw.dtype == x.dtype == scx.dtype
    fsw = None
    if fs is not None:
        fsw, want2 = fs
        assert not defer_req and fsw.is_contiguous() and tuple(fsw.shape) == (Cout, Cin) and fsw.dtype == x.dtype
    # the launch's own params, asked first: FRESH stands in for the statistics and the second output until the plan serves them
    p = L.Conv3(_ptr(x), ld, _ptr(out), ldy, _ptr(wpk), B, D, H, W, Cin, Cout, _dt(x), None, _ptr(res) if res is not None and res.dtype == x.dtype else None,
                rows(res)[0] if res is not None else 0, FRESH if want_stat else None, 0,
                int(defer_req and D * H * W <= lib.miseg_instnorm_fused_max_rows() and ldy == Cout),
                _ptr(scx), ldsc, _ptr(scw), Csc, _ptr(s2c), (s2c.shape[-1] // 8) if s2c is not None else 0,
                _ptr(fsw), FRESH if fs is not None else None, Cout if fs is not None else 0, None)
    plan = _plan("miseg_conv3_fwd_plan", p, L.Conv3Plan())
    if plan.kernel != L.CONV3_GENERIC and _background():
        p.background = 1
        plan = _plan("miseg_conv3_fwd_plan", p, L.Conv3Plan())
    fuse_res, defer = bool(plan.res), bool(plan.defer_slabs)      # (the roofline leg times the launches exactly as the step issues them)
    if not fuse_res:
        p.res, p.ldres = None, 0
    ws = torch.empty(plan.workspace_bytes // 4, dtype=torch.float32, device=x.device) if plan.workspace_bytes else None
    stat = STAT_POOL.take(lib.miseg_instnorm_stat_bytes(B, Cout) // 8, x.device).view(-1, B, Cout, 2) if plan.stat else None
    p.workspace, p.stat = _ptr(ws), _ptr(stat)
    name = (f"conv3_fwd{('', '96', '_tiny')[plan.kernel]}_kernel<{'bf16' if x.dtype == torch.bfloat16 else 'f32'}>"
            + (" (background)" if p.background else ""))
    flops = 2.0 * B * D * H * W * 27 * Cin * Cout
    # algorithmic bytes: x read once, y written once, the weight pack, the fused residual read once
    nbytes = float(x.element_size()) * (B * D * H * W * (Cin + Cout + (Cout if fuse_res else 0)) + wpk.numel())
    if sc is not None:
        flops += 2.0 * n * Csc * Cout
        nbytes += float(x.element_size()) * (n * Csc + scw.numel())
    y2 = stat2 = None
    if fs is not None:
        y2 = torch.empty(B, D, H, W, Cout, dtype=x.dtype, device=x.device)
        if want2:
            stat2 = STAT_POOL.take(lib.miseg_instnorm_stat_bytes(B, Cout) // 8, x.device).view(-1, B, Cout, 2)
        p.fs_y, p.fs_stat = _ptr(y2), _ptr(stat2)
        flops += 2.0 * n * Cin * Cout
        nbytes += float(x.element_size()) * (n * Cout + fsw.numel())
    _call("miseg_conv3_fwd", p, prof=(name, flops, nbytes))
    if fs is not None:
        assert res is None or fuse_res
        return out, stat, y2, stat2
    if res is not None and not fuse_res:
        out = add(out, res)
    if defer:
        return out, PendingSlabs(ws, plan.splits, B * D * H * W * Cout)
    if defer_req and not want_stat:
        return out, None
    return (out, stat) if want_stat else out


class PendingSlabs:
    """what conv3_fwd(..., want_stat="defer") returns in place of the statistics: its output tensor is NOT written yet - the fp32 partial
    slabs of the split launch wait in `ws` for instnorm_fwd_slabs"""
    __slots__ = ("ws", "n", "stride")

    def __init__(self, ws, n, stride):
        self.ws, self.n, self.stride = ws, n, stride


CONV_WGRAD_GROUP_VOXELS = 48 ** 3   # layers up to this many voxels are queued: alone they fill a fraction of the chip for 40-85 us each


def _flush_conv_wgrads(q):
    if not q:
        return
    lib = L.load()
    for dt in {it[0].dtype for it in q}:
        items = [it for it in q if it[0].dtype == dt]
        for i in range(0, len(items), 24):
            chunk = items[i:i + 24]
            descs = (L.Conv3Wgrad * len(chunk))()
            for j, (x, dy, dw, acc) in enumerate(chunk):
                B, D, H, W = _vol(x)
                ldx, _, Cin = rows(x)
                lddy, _, Cout = rows(dy)
                descs[j] = L.Conv3Wgrad(_ptr(x), ldx, _ptr(dy), lddy, _ptr(dw), B, D, H, W, Cin, Cout, _dt(x), acc, None, 0)
            wsb = lib.miseg_conv3_wgrad_group_workspace_bytes(descs, len(chunk))
            ws = torch.empty(max(wsb // 4, 1), dtype=torch.float32, device=chunk[0][0].device)
            fl = sum(2.0 * 27 * it[0].shape[-1] * it[1].shape[-1] * (it[0].numel() // it[0].shape[-1]) for it in chunk)
            with _ProfRegion("conv3_wgrad_group_kernel", fl):
                L.check(lib.miseg_conv3_wgrad_group(descs, len(chunk), _ptr(ws), _stream()), "conv3_wgrad_group")
            _stamp_launch("conv3_wgrad_group")
    q.clear()


def _conv3_wgrad_params(x, dy, dw, accumulate):
    (ldx, n, Cin), (lddy, n2, Cout) = rows(x), rows(dy)
    assert n == n2
    return L.Conv3Wgrad(_ptr(x), ldx, _ptr(dy), lddy, _ptr(dw), *_vol(x), Cin, Cout, _dt(x), int(accumulate), None, 0)


def conv3_wgrad_plan(x, dy):
    """the plan (L.Conv3WgradPlan) of conv3_wgrad(x, dy): the kernel and its workspace"""
    return _plan("miseg_conv3_wgrad_plan", _conv3_wgrad_params(x, dy, None, 0), L.Conv3WgradPlan())


def _conv3_wgrad_launch(p, device, name):
    wsb = _plan("miseg_conv3_wgrad_plan", p, L.Conv3WgradPlan()).workspace_bytes
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=device) if wsb else None
    p.workspace = _ptr(ws)
    _call("miseg_conv3_wgrad", p, prof=(name, 2.0 * p.B * p.D * p.H * p.W * 27 * p.Cin * p.Cout))


def conv3_wgrad(x, dy, dw=None, accumulate=False):
    """accumulate: False / True, or 2 = `dw` is known to hold zeros (a fresh arena slot): single-producer layers then store instead
    of read-modify-write and the others skip their zero fill."""
    if dw is None:
        dw = torch.empty(rows(dy)[2], rows(x)[2], 3, 3, 3, dtype=torch.float32, device=x.device)
        accumulate = False
    p = _conv3_wgrad_params(x, dy, dw, accumulate)
    kernel = _plan("miseg_conv3_wgrad_plan", p, L.Conv3WgradPlan()).kernel
    q = _queues(dw) if accumulate else None
    # (narrow bf16 layers - 16 / 32 channels on both sides - have a kernel of their own that finishes a 48^3 layer in ~10 us: never queued)
    # tiny volumes (3^3 / 6^3, hundreds of channels: encoder10 / decoder5): the write-bound kernel of their own, launched where the backward
    # pass reaches them (round 5: queued for the end of the pass, on the branch stream beside the grouped launch, 154.2 / 154.2 patches/s
    # against 155.2 / 154.5 - four write-bound launches, 176 MB, lengthen the tail by more than the 80 us they take off the chain)
    tiny = kernel == L.CONV3_WGRAD_TINY
    if q is not None and q.unzeroed and dw.data_ptr() in q.unzeroed:
        q.unzeroed.discard(dw.data_ptr())
        if not (tiny and int(accumulate) == 2):      # anything but the overwriting launch reads (or only adds to) the slot: it gets its zeros now
            fill32(dw)
    if q is not None and p.B * p.D * p.H * p.W <= CONV_WGRAD_GROUP_VOXELS and kernel not in (L.CONV3_WGRAD_NARROW, L.CONV3_WGRAD_TINY):
        q.lists().conv_wgrad.append((x, dy, dw, int(accumulate)))      # keeps x and dy alive until the flush
        return dw
    if tiny and q is not None and int(accumulate) == 2:
        q.inline_final.append(dw)      # written here, once, by plain stores: nothing queued will touch the slot again
    p.max_workgroups = bg = _background()
    _conv3_wgrad_launch(p, x.device, f"conv3_wgrad_kernel<{'bf16' if x.dtype == torch.bfloat16 else 'f32'}>" + (" (background)" if bg else ""))
    return dw


def conv3_thin_fwd(x_ncdhw, w, dtype):
    B, Cin, D, H, W = x_ncdhw.shape
    assert x_ncdhw.dtype == torch.float32 and x_ncdhw.is_contiguous()
    Cout = w.shape[0]
    y = torch.empty(B, D, H, W, Cout, dtype=dtype, device=x_ncdhw.device)
    _call("miseg_conv3_thin_fwd", L.Conv3Thin(_ptr(x_ncdhw), _ptr(y), Cout, _ptr(_fp32(w)), B, Cin, D, H, W, Cout, _dt(y)))
    return y


def conv3_thin_wgrad(x_ncdhw, dy, dw):
    B, Cin, D, H, W = x_ncdhw.shape
    Cout = dy.shape[-1]
    p = L.Conv3ThinWgrad(_ptr(x_ncdhw), _ptr(dy), rows(dy)[0], _ptr(dw), B, Cin, D, H, W, Cout, _dt(dy), None)
    nb = L.load().miseg_conv3_thin_wgrad_workspace_bytes(C.byref(p))
    ws = torch.empty(nb // 4, dtype=torch.float32, device=dy.device) if nb else None
    p.workspace = _ptr(ws)
    _call("miseg_conv3_thin_wgrad", p)
    return dw


def ncdhw_to_rows(x_ncdhw, dtype):
    """NCDHW fp32 image -> channels-last rows with one 16-byte vector per voxel (channels >= Cin zero)."""
    B, Cin, D, H, W = x_ncdhw.shape
    assert x_ncdhw.dtype == torch.float32 and x_ncdhw.is_contiguous()
    CP = 16 // torch.empty(0, dtype=dtype).element_size()
    y = torch.empty(B, D, H, W, CP, dtype=dtype, device=x_ncdhw.device)
    lib = L.load()
    L.check(lib.miseg_ncdhw_to_rows(_ptr(x_ncdhw), _ptr(y), B, Cin, D * H * W, CP, _dt(y), _stream()), "ncdhw_to_rows")
    return y


def resample2(x, up, fine_shape=None):
    """up=False: keep the even voxels of x [B,D,H,W,C] (the stride-2 pick); up=True: zero insertion into a grid of
    fine_shape = (D, H, W) (ceil(./2) must be x's grid)."""
    B, d, h, w = _vol(x)
    ld, n, Cc = rows(x)
    if up:
        D, H, W = fine_shape
        assert ((D + 1) // 2, (H + 1) // 2, (W + 1) // 2) == (d, h, w), (fine_shape, x.shape)
        out = torch.empty(B, D, H, W, Cc, dtype=x.dtype, device=x.device)
    else:
        D, H, W = d, h, w
        out = torch.empty(B, (D + 1) // 2, (H + 1) // 2, (W + 1) // 2, Cc, dtype=x.dtype, device=x.device)
    _call("miseg_resample2", L.Resample2(_ptr(x), ld, _ptr(out), rows(out)[0], B, D, H, W, Cc, _dt(x), int(up)))
    return out


def upsample_cat(skip, x, factor):
    """cat([skip, nearest_upsample(x, factor)], channel) in one launch (reference unet_vanilla.py:162-169): skip [B,D,H,W,Cs] and x
    [B,D/f,H/f,W/f,Cu] row views of one dtype, factor 1 or 2 -> a new [B,D,H,W,Cs+Cu]."""
    factor = int(factor)
    if factor not in (1, 2):
        raise NotImplementedError(f"upsample_cat: scale factor {factor} (1 or 2)")
    B, D, H, W = _vol(skip)
    if x.dim() != 5 or x.shape[0] != B or tuple(factor * v for v in x.shape[1:4]) != (D, H, W):
        raise ValueError(f"upsample_cat: x {tuple(x.shape)} upsampled by {factor} does not match the skip {tuple(skip.shape)}")
    if x.dtype != skip.dtype:
        raise ValueError(f"upsample_cat: dtypes {skip.dtype} / {x.dtype}")
    lds, _, Cs = rows(skip)
    ldx, _, Cu = rows(x)
    out = torch.empty(B, D, H, W, Cs + Cu, dtype=x.dtype, device=x.device)
    _call("miseg_upsample_cat", L.UpsampleCat(_ptr(skip), lds, _ptr(x), ldx, _ptr(out), Cs + Cu, B, D, H, W, Cs, Cu, factor, _dt(x)),
          prof=("upsample_cat", 0.0, _nb(skip, x, out)))
    return out


def upsample_cat_bwd(dcat_right, factor):
    """gradient of x in upsample_cat: dcat_right is the right half of the concat's gradient ([B,D,H,W,Cu] row view, its own leading dimension);
    returns [B,D/f,H/f,W/f,Cu], each entry the fp32 sum of its f^3 fine children in a fixed order, rounded once"""
    factor = int(factor)
    if factor not in (1, 2):
        raise NotImplementedError(f"upsample_cat_bwd: scale factor {factor} (1 or 2)")
    B, D, H, W = _vol(dcat_right)
    if D % factor or H % factor or W % factor:
        raise ValueError(f"upsample_cat_bwd: grid {(D, H, W)} is not {factor} x a coarse grid")
    ld, _, Cu = rows(dcat_right)
    dx = torch.empty(B, D // factor, H // factor, W // factor, Cu, dtype=dcat_right.dtype, device=dcat_right.device)
    _call("miseg_upsample_cat_bwd", L.UpsampleCatBwd(_ptr(dcat_right), ld, _ptr(dx), Cu, B, D, H, W, Cu, factor, _dt(dx)),
          prof=("upsample_cat", 0.0, _nb(dcat_right, dx)))
    return dx


def rowbias_add(x, bias):
    ld, n, Cc = rows(x)
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    _call("miseg_rowbias_add", L.Rowbias(_ptr(x), ld, _ptr(_fp32(bias)), _ptr(y), rows(y)[0], n, Cc, _dt(x)))
    return y


def prelu_fwd(x, slope):
    ld, n, Cc = rows(x)
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    _call("miseg_prelu_fwd", L.PreluFwd(_ptr(x), ld, _ptr(_fp32(slope)), _ptr(y), rows(y)[0], n, Cc, _dt(x)))
    return y


def prelu_bwd(dy, x, slope, dslope):
    ld, n, Cc = rows(x)
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    scratch = STAT_POOL.take(2, x.device) if dslope is not None else None      # zeroed fp64 (sum, arrival ticket) of the slope-gradient reduction
    _call("miseg_prelu_bwd", L.PreluBwd(_ptr(dy), rows(dy)[0], _ptr(x), ld, _ptr(_fp32(slope)), _ptr(dx), rows(dx)[0], _ptr(dslope), n, Cc, _dt(x), _ptr(scratch)))
    return dx


def rows_to_ncdhw(x):
    """channels-last [B,D,H,W,C] in the compute dtype -> NCDHW fp32 (the network output layout)."""
    B, D, H, W = _vol(x)
    ld, n, Cc = rows(x)
    y = torch.empty(B, Cc, D, H, W, dtype=torch.float32, device=x.device)
    lib = L.load()
    L.check(lib.miseg_layout_ncdhw(_ptr(x), ld, _ptr(y), B, Cc, D * H * W, _dt(x), 0, _stream()), "layout_ncdhw")
    return y


def ncdhw_to_rows_exact(g, dtype):
    """NCDHW fp32 -> channels-last rows of exactly C channels in `dtype` (gradient of rows_to_ncdhw)."""
    B, Cc, D, H, W = g.shape
    assert g.dtype == torch.float32 and g.is_contiguous()
    y = torch.empty(B, D, H, W, Cc, dtype=dtype, device=g.device)
    lib = L.load()
    L.check(lib.miseg_layout_ncdhw(_ptr(y), Cc, _ptr(g), B, Cc, D * H * W, _dt(y), 1, _stream()), "layout_ncdhw")
    return y


def im2col3(x, adjoint=False, C_out=None):
    """forward: x [B,D,H,W,C] -> col [B,D,H,W,27*C];  adjoint: col -> [B,D,H,W,C]."""
    B, D, H, W = _vol(x)
    ld, n, Cc = rows(x)
    if not adjoint:
        out = torch.empty(B, D, H, W, 27 * Cc, dtype=x.dtype, device=x.device)
        _call("miseg_im2col3", L.Im2col3(_ptr(x), ld, _ptr(out), 27 * Cc, B, D, H, W, Cc, _dt(x)))
    else:
        Co = Cc // 27
        out = torch.empty(B, D, H, W, Co, dtype=x.dtype, device=x.device)
        _call("miseg_col2im3", L.Im2col3(_ptr(x), ld, _ptr(out), Co, B, D, H, W, Co, _dt(x)))
    return out


# ------------------------------------------------------------------------------------------ attention
def winattn_params(qkv, out, qkv_bias, table, lse, heads, window, shift, tw, scale, drop=None):
    """drop = (p, (seed, stream_id, step_dev)) puts dropout on the attention probabilities; the key is DROP.next_key's"""
    B, D, H, W = _vol(qkv)
    ldq, n, C3 = rows(qkv)
    Cc = C3 // 3
    dp, (seed, sid, step) = drop if drop else (0.0, (0, 0, None))
    return L.Winattn(_ptr(qkv), ldq, _ptr(out), rows(out)[0], _ptr(qkv_bias), _ptr(table), _ptr(lse), B, D, H, W, Cc, heads, _dt(qkv),
                     window[0], window[1], window[2], shift[0], shift[1], shift[2], tw, scale, float(dp), seed, sid, _ptr(step))


def winattn_fwd_plan(p):
    """the plan (L.WinattnPlan) of miseg_winattn_fwd on these winattn_params; raises what the launch would raise for a call it refuses"""
    return _plan("miseg_winattn_fwd_plan", p, L.WinattnPlan())


def winattn_bwd_plan(p):
    """the plan (L.WinattnPlan) of miseg_winattn_bwd on this L.WinattnBwd (winattn_params in .f)"""
    return _plan("miseg_winattn_bwd_plan", p, L.WinattnPlan())


def _windows_tokens(qkv, window):
    """(windows over the padded grid, tokens per window)"""
    B, D, H, W = _vol(qkv)
    return B * -(-D // window[0]) * -(-H // window[1]) * -(-W // window[2]), window[0] * window[1] * window[2]


def winattn_fwd(qkv, qkv_bias, table, heads, window, shift, tw, scale, drop=None):
    B, D, H, W = _vol(qkv)
    Cc = qkv.shape[-1] // 3
    out = torch.empty(B, D, H, W, Cc, dtype=qkv.dtype, device=qkv.device)
    nw, n = _windows_tokens(qkv, window)
    lse = torch.empty(nw, heads, n, dtype=torch.float32, device=qkv.device)
    _call("miseg_winattn_fwd", winattn_params(qkv, out, qkv_bias, table, lse, heads, window, shift, tw, scale, drop),
          prof=("winattn", 4.0 * nw * heads * n * n * (Cc // heads), _nb(qkv, out, lse)))
    return out, lse


def winattn_bwd(qkv, out, lse, dout, qkv_bias, table, heads, window, shift, tw, scale, dqkv_bias, dtable, drop=None):
    dqkv = torch.empty(qkv.shape, dtype=qkv.dtype, device=qkv.device)
    f = winattn_params(qkv, out, qkv_bias, table, lse, heads, window, shift, tw, scale, drop)
    p = L.WinattnBwd(f, _ptr(dout), rows(dout)[0], _ptr(dqkv), rows(dqkv)[0], _ptr(dqkv_bias), _ptr(dtable))
    nw, n = _windows_tokens(qkv, window)
    _call("miseg_winattn_bwd", p, prof=("winattn", 10.0 * nw * heads * n * n * (qkv.shape[-1] // 3 // heads), _nb(qkv, out, lse, dout, dqkv)))
    return dqkv


# ------------------------------------------------------------------------------------------ elementwise / movement
def add(a, b, out=None):
    lda, n, Cc = rows(a)
    y = out if out is not None else torch.empty(a.shape, dtype=a.dtype, device=a.device)
    _call("miseg_add", L.Add(_ptr(a), lda, _ptr(b), rows(b)[0], _ptr(y), rows(y)[0], n, Cc, _dt(a)))
    return y


def copy2d(src, dst):
    lds, n, Cc = rows(src)
    ldd, n2, C2 = rows(dst)
    assert n == n2 and Cc == C2
    _call("miseg_copy2d", L.Copy2d(_ptr(src), lds, _dt(src), _ptr(dst), ldd, _dt(dst), n, Cc))
    return dst


def gelu_fwd(x):
    ld, n, Cc = rows(x)
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    _call("miseg_gelu_fwd", L.GeluFwd(_ptr(x), ld, _ptr(y), rows(y)[0], n, Cc, _dt(x)))
    return y


def gelu_bwd(dy, x):
    ld, n, Cc = rows(x)
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    _call("miseg_gelu_bwd", L.GeluBwd(_ptr(dy), rows(dy)[0], _ptr(x), ld, _ptr(dx), rows(dx)[0], n, Cc, _dt(x)))
    return dx


def _offs(offsets):
    arr = (C.c_int8 * 24)()
    flat = [v for o in offsets for v in o]
    assert len(flat) == 24
    for i, v in enumerate(flat):
        arr[i] = v
    return arr


def space_to_channel(fine, offsets, out=None):
    """fine [B,D,H,W,C] -> coarse [B,ceil(D/2),ceil(H/2),ceil(W/2),8C] with block j taken at offsets[j]."""
    B, D, H, W = _vol(fine)
    ld, n, Cc = rows(fine)
    if out is None:
        out = torch.empty(B, (D + 1) // 2, (H + 1) // 2, (W + 1) // 2, 8 * Cc, dtype=fine.dtype, device=fine.device)
    _call("miseg_space_to_channel", L.S2C(_ptr(fine), ld, _ptr(out), rows(out)[0], B, D, H, W, Cc, _dt(fine), _offs(offsets)))
    return out


def channel_to_space(coarse, offsets, fine_shape, out=None):
    """adjoint of space_to_channel: coarse [B,D2,H2,W2,8C] -> fine [B,D,H,W,C] (sum over blocks referencing a voxel)."""
    B, D, H, W, Cc = fine_shape
    if out is None:
        out = torch.empty(B, D, H, W, Cc, dtype=coarse.dtype, device=coarse.device)
    _call("miseg_channel_to_space", L.S2C(_ptr(coarse), rows(coarse)[0], _ptr(out), rows(out)[0], B, D, H, W, Cc, _dt(coarse), _offs(offsets)))
    return out


def patch_embed_fwd(x_ncdhw, w, bias, dtype):
    B, Cin, D, H, W = x_ncdhw.shape
    assert x_ncdhw.dtype == torch.float32 and x_ncdhw.is_contiguous()
    Cout = w.shape[0]
    y = torch.empty(B, D // 2, H // 2, W // 2, Cout, dtype=dtype, device=x_ncdhw.device)
    _call("miseg_patch_embed_fwd", L.PatchEmbed(_ptr(x_ncdhw), _ptr(y), Cout, _ptr(_fp32(w)), _ptr(_fp32(bias)), B, Cin, D, H, W, Cout, _dt(y)))
    return y


def patch_embed_bwd(x_ncdhw, dy, dw, dbias):
    B, Cin, D, H, W = x_ncdhw.shape
    Cout = dy.shape[-1]
    p = L.PatchEmbedBwd(_ptr(x_ncdhw), _ptr(dy), rows(dy)[0], _ptr(dw), _ptr(dbias), B, Cin, D, H, W, Cout, _dt(dy), None)
    ws = torch.empty(L.load().miseg_patch_embed_bwd_workspace_bytes(C.byref(p)) // 4, dtype=torch.float32, device=dy.device)
    p.workspace = ws.data_ptr()
    _call("miseg_patch_embed_bwd", p)


def head_fwd(x, w, bias):
    B, D, H, W = _vol(x)
    ld, n, Cin = rows(x)
    Cout = w.shape[0]
    y = torch.empty(B, Cout, D, H, W, dtype=torch.float32, device=x.device)
    _call("miseg_head_fwd", L.Head(_ptr(x), ld, _ptr(y), _ptr(_fp32(w)), _ptr(_fp32(bias)), B, D * H * W, Cin, Cout, _dt(x)))
    return y


def head_bwd(x, dy_ncdhw, w, dw, dbias, want_dx=True):
    B, D, H, W = _vol(x)
    ld, n, Cin = rows(x)
    Cout = w.shape[0]
    assert dy_ncdhw.dtype == torch.float32 and dy_ncdhw.is_contiguous()
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device) if want_dx else None
    _call("miseg_head_bwd", L.HeadBwd(_ptr(x), ld, _ptr(dy_ncdhw), _ptr(dx), rows(dx)[0] if dx is not None else 0, _ptr(_fp32(w)), _ptr(dw), _ptr(dbias),
                                      B, D * H * W, Cin, Cout, _dt(x)))
    return dx


def fill32(t, word=0):
    lib = L.load()
    assert t.is_contiguous() and t.element_size() == 4
    L.check(lib.miseg_fill32(_ptr(t), word, t.numel(), _stream()), "fill32")
    return t


def fill32_ranges(t, ranges, word=0):
    """t[off : off + n] = word for every (off, n) of `ranges` (element offsets into the contiguous 4-byte tensor t, multiples of 4) in one launch
    per L.FILL_RANGES ranges"""
    lib = L.load()
    assert t.is_contiguous() and t.element_size() == 4
    ranges = [(int(o), int(n)) for o, n in ranges if n > 0]
    for i in range(0, len(ranges), L.FILL_RANGES):
        chunk = ranges[i:i + L.FILL_RANGES]
        arr = (C.c_uint64 * (2 * len(chunk)))(*[v for r in chunk for v in r])
        L.check(lib.miseg_fill32_ranges(_ptr(t), word, arr, len(chunk), _stream()), "fill32_ranges")
    return t


def zeros_f32(shape, device):
    return fill32(torch.empty(shape, dtype=torch.float32, device=device))


# ------------------------------------------------------------------------------------------ after the path: loss, metric, optimiser, stitching
def _label(label):
    """class-id labels [B, 1, ...] (any of float32 / int32 / int64 / uint8, as the data pipeline delivers them) -> (tensor, MISEG_LABEL_*)"""
    kinds = {torch.float32: L.LABEL_F32, torch.int32: L.LABEL_I32, torch.int64: L.LABEL_I64, torch.uint8: L.LABEL_U8}
    if label.dtype not in kinds:
        label = label.to(torch.int32)
    return label.contiguous(), kinds[label.dtype]


GDICE_WEIGHT_TYPES = {"square": L.GDICE_W_SQUARE, "simple": L.GDICE_W_SIMPLE, "uniform": L.GDICE_W_UNIFORM}


def gdice_weight_type(name):
    """MONAI's w_type / weight_type name -> MISEG_GDICE_W_*"""
    if name not in GDICE_WEIGHT_TYPES:
        raise ValueError(f"Unsupported weight type: {name}, available options are {list(GDICE_WEIGHT_TYPES)}.")
    return GDICE_WEIGHT_TYPES[name]


class SegLossCfg:
    """DiceFocalLoss / DiceCELoss hyper-parameters as LitMonai builds them (reference lightning_monai.py:48-65); weight_type (a MISEG_GDICE_W_*)
    belongs to GeneralizedDiceFocalLoss (reference utils/training_utils.py:26-33), whose lambda_dice is its lambda_gdl"""

    def __init__(self, kind, include_background, squared_pred, smooth_nr, smooth_dr, gamma=2.0, lambda_dice=1.0, lambda_other=1.0, weight_type=L.GDICE_W_SQUARE):
        self.kind, self.include_background, self.squared_pred = kind, bool(include_background), bool(squared_pred)
        self.weight_type = int(weight_type)
        self.smooth_nr, self.smooth_dr, self.gamma, self.lambda_dice, self.lambda_other = float(smooth_nr), float(smooth_dr), float(gamma), float(lambda_dice), float(lambda_other)


def _seg_loss_params(logits, label, cfg, sums, ws):
    if not logits.is_cuda:
        raise L.MisegHipError("miseg ops need CUDA/HIP tensors: the MI355X path has no CPU fallback")
    if logits.dtype != torch.float32 or not logits.is_contiguous() or logits.dim() < 3:
        raise ValueError("seg_loss: logits must be contiguous float32 [B, C, ...]")
    B, Cc = logits.shape[0], logits.shape[1]
    S = logits.numel() // (B * Cc)
    if label.numel() != B * S:
        raise ValueError(f"seg_loss: label {tuple(label.shape)} does not match logits {tuple(logits.shape)} ([B, 1, ...] class ids)")
    lab, ldt = _label(label)
    p = L.SegLoss(C.sizeof(L.SegLoss), cfg.kind, _ptr(logits), _ptr(lab), ldt, B, Cc, S, int(cfg.include_background), int(cfg.squared_pred), cfg.smooth_nr,
                  cfg.smooth_dr, cfg.gamma, cfg.lambda_dice, cfg.lambda_other, _ptr(ws), _ptr(sums), None, None, None, cfg.weight_type)
    return p, lab, (B, Cc, S)


def seg_loss_fwd(logits, label, cfg):
    """-> (loss: 0-dim fp32 device tensor, sums: fp64 [3 B C + 1] saved for the backward pass)"""
    B, Cc = logits.shape[0], logits.shape[1]
    S = logits.numel() // (B * Cc)
    lib = L.load()
    ws = torch.empty(lib.miseg_seg_loss_workspace_bytes(B, Cc, S) // 8, dtype=torch.float64, device=logits.device)
    sums = torch.empty(3 * B * Cc + 1, dtype=torch.float64, device=logits.device)
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    p, lab, _ = _seg_loss_params(logits, label, cfg, sums, ws)
    p.loss = _ptr(loss)
    _call("miseg_seg_loss_fwd", p)
    return loss, sums


def seg_loss_bwd(logits, label, cfg, sums, gscale=None):
    """d(loss)/d(logits) * gscale (a 0-dim fp32 device tensor or None)"""
    dlogits = torch.empty_like(logits)
    ws = torch.empty(1, dtype=torch.float64, device=logits.device)      # not used by the backward pass
    p, lab, _ = _seg_loss_params(logits, label, cfg, sums, ws)
    if gscale is not None:
        gscale = gscale.to(torch.float32).contiguous()
        p.gscale = _ptr(gscale)
    p.dlogits = _ptr(dlogits)
    _call("miseg_seg_loss_bwd", p)
    return dlogits


def dice_metric(logits, label, gdice=None):
    """[B, C] Dice per class after argmax (NaN where the class is absent from the label).  gdice = (include_background, weight_type name): also the
    generalized Dice score [B] from the same counts (one pass over the volume) -> (dice, score)"""
    if logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError("dice_metric: logits must be contiguous float32 [B, C, ...]")
    B, Cc = logits.shape[0], logits.shape[1]
    S = logits.numel() // (B * Cc)
    if label.numel() != B * S:
        raise ValueError("dice_metric: label does not match logits")
    lab, ldt = _label(label)
    counts = torch.empty(B * Cc * 3, dtype=torch.int64, device=logits.device)
    dice = torch.empty(B, Cc, dtype=torch.float32, device=logits.device)
    if gdice is None:
        _call("miseg_dice_metric", L.DiceMetric(C.sizeof(L.DiceMetric), _ptr(logits), _ptr(lab), ldt, B, Cc, S, _ptr(counts), _ptr(dice), None, 1, 0))
        return dice
    score = torch.empty(B, dtype=torch.float32, device=logits.device)
    _call("miseg_dice_metric", L.DiceMetric(C.sizeof(L.DiceMetric), _ptr(logits), _ptr(lab), ldt, B, Cc, S, _ptr(counts), _ptr(dice), _ptr(score), int(bool(gdice[0])),
                                            gdice_weight_type(gdice[1])))
    return dice, score


def _surface_args(who, label, logits, pred, num_classes):
    """the checked arguments both surface entry points share: (logits, pred as an int32 class map, label, label dtype code, B, C, D, H, W, device)"""
    if (logits is None) == (pred is None):
        raise ValueError(f"{who}: exactly one of logits / pred")
    if logits is not None:
        if logits.dtype != torch.float32 or not logits.is_contiguous() or logits.dim() != 5:
            raise ValueError(f"{who}: logits must be contiguous float32 [B, C, D, H, W]")
        B, Cc, D, H, W = logits.shape
        dev = logits.device
    else:
        if num_classes is None:
            raise ValueError(f"{who}: a class map needs num_classes")
        B, Cc = pred.shape[0], int(num_classes)
        if pred.dim() == 5 and pred.shape[1] == 1:
            pred = pred[:, 0]
        if pred.dim() != 4:
            raise ValueError(f"{who}: pred must be a class map [B, (1,) D, H, W]")
        D, H, W = pred.shape[1:]
        pred = pred.to(torch.int32).contiguous()
        dev = pred.device
    if label.numel() != B * D * H * W:
        raise ValueError(f"{who}: label does not match the prediction")
    lab, ldt = _label(label.to(dev))
    return logits, pred, lab, ldt, B, Cc, D, H, W, dev


def _surface_launch(who, label, logits, pred, num_classes, include_background, symmetric, pct, directed, want, class_thresholds):
    """one launch set of csrc/surface.hip through the smallest entry point that computes `want`: miseg_surface_dice with "nsd",
    miseg_surface_metrics with "hd" and no "nsd", miseg_surface_distance for ("asd",) alone (the header guarantees the same bits from all
    three); the fp64 [B, C'] tensors named in `want`, in that order.  Each parameter struct is a prefix of the next: `tail` is what follows
    the workspace."""
    logits, pred, lab, ldt, B, Cc, D, H, W, dev = _surface_args(who, label, logits, pred, num_classes)
    cp = max(Cc - (0 if include_background else 1), 0)
    out = {w: torch.empty(B, cp, dtype=torch.float64, device=dev) for w in want}
    name, struct, tail = "miseg_surface_metrics", L.SurfaceMetrics, [_ptr(out.get("asd")), _ptr(out.get("hd")), pct, int(bool(directed))]
    if "nsd" in want:
        if class_thresholds is None:
            raise ValueError(f"{who}: 'nsd' needs class_thresholds")
        taus = [float(t) for t in class_thresholds]
        if len(taus) != cp:
            raise ValueError(f"{who}: number of classes ({cp}) does not match number of class thresholds ({len(taus)}).")
        if any(not 0.0 <= t < float("inf") for t in taus):
            raise ValueError(f"{who}: all class thresholds need to be finite and >= 0, got {taus}.")
        name, struct, tail = "miseg_surface_dice", L.SurfaceDice, tail + [_ptr(out["nsd"]), (C.c_double * max(len(taus), 1))(*taus)]
    elif "hd" not in want:
        name, struct, tail = "miseg_surface_distance", L.SurfaceDistance, tail[:1]
    nbytes = getattr(L.load(), name + "_workspace_bytes")(B, Cc, D, H, W)
    ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
    _call(name, struct(C.sizeof(struct), _ptr(logits), _ptr(pred), _ptr(lab), ldt, B, Cc, D, H, W, int(bool(include_background)), int(bool(symmetric)),
                       _ptr(ws), *tail))
    return tuple(out[w] for w in want)


def surface_distance(label, logits=None, pred=None, num_classes=None, include_background=True, symmetric=True):
    """fp64 [B, C'] symmetric (or one-way) average surface distance per class after argmax of fp32 logits [B, C, D, H, W], or of an integer
    class map pred [B, (1,) D, H, W] with num_classes classes (miseg_surface_distance; C' = C - (0 if include_background else 1)).
    Synchronises the stream: the kernel reads the per-class boxes back to size its passes."""
    return _surface_launch("surface_distance", label, logits, pred, num_classes, include_background, symmetric, 0.0, False, ("asd",), None)[0]


def surface_metrics(label, logits=None, pred=None, num_classes=None, include_background=True, symmetric=True, percentile=None, directed=False,
                    want=("asd", "hd"), class_thresholds=None):
    """the average surface distance of surface_distance (`symmetric`), the Hausdorff distance (`percentile`: None or 0 for the maximum, else in
    (0, 100]; `directed`: pred -> label only) and / or the normalized surface Dice ("nsd": `class_thresholds`, one finite tolerance >= 0 in
    voxels per class after include_background) per class, from ONE launch set (_surface_launch picks the entry point): a tuple of the fp64
    [B, C'] tensors named in `want`, in that order.  Synchronises the stream like surface_distance."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in ("asd", "hd", "nsd") for w in want) or len(set(want)) != len(want):
        raise ValueError(f"surface_metrics: want {want!r} (some of 'asd', 'hd', 'nsd')")
    pct = 0.0 if percentile is None else float(percentile)
    if not 0.0 <= pct <= 100.0:
        raise ValueError(f"surface_metrics: percentile should be a value between 0 and 100, got {percentile}.")
    return _surface_launch("surface_metrics", label, logits, pred, num_classes, include_background, symmetric, pct, directed, want, class_thresholds)


_EXPORT_DTYPES = {torch.uint8: 1, torch.uint16: 2, torch.uint32: 4}


def first_max_argmax(x):
    """argmax over dim 0 under the kernels' rule: a strict `>` scan, so the FIRST maximum wins and a NaN after channel 0 never does (a NaN in
    channel 0 gives class 0).  torch.argmax differs only where NaNs are present."""
    arg = torch.zeros(x.shape[1:], dtype=torch.int64, device=x.device)
    mx = x[0]
    for c in range(1, x.shape[0]):
        up = x[c] > mx
        mx = torch.where(up, x[c], mx)
        arg = torch.where(up, torch.full_like(arg, c), arg)
    return arg


_MAP_DTYPES = {torch.uint8: 1, torch.int32: 4}


def _class_map_source(name, logits, pred, num_classes, applied_labels, connectivity, out_dtype):
    """the checked arguments the connected-component filters share: (logits, pred, src, B, Cc, D, H, W, applied, conn) - of logits (fp32
    [B, C, D, H, W]) / pred (uint8 or int32 [B, D, H, W]) the one that was given, contiguous, which is also src; the 64-bit set of applied
    classes; the connectivity 1..3"""
    from ..training import postprocess as PP
    if (logits is None) == (pred is None):
        raise ValueError(f"{name}: exactly one of logits / pred")
    if out_dtype not in _MAP_DTYPES:
        raise ValueError(f"{name}: out_dtype {out_dtype} (uint8 / int32)")
    conn = PP.check_connectivity(connectivity)
    if logits is not None:
        if logits.dtype != torch.float32 or logits.dim() != 5:
            raise ValueError(f"{name}: logits must be float32 [B, C, D, H, W]")
        B, Cc, D, H, W = logits.shape
        if num_classes is not None and int(num_classes) != Cc:
            raise ValueError(f"{name}: num_classes {num_classes} for logits of {Cc} channels")
        src = logits = logits.contiguous()
    else:
        if num_classes is None:
            raise ValueError(f"{name}: a class map needs num_classes")
        if pred.dim() == 5 and pred.shape[1] == 1:
            pred = pred[:, 0]
        if pred.dim() != 4 or pred.dtype.is_floating_point or pred.dtype == torch.bool:
            raise ValueError(f"{name}: pred must be an integer class map [B, (1,) D, H, W]")
        B, Cc = pred.shape[0], int(num_classes)
        D, H, W = pred.shape[1:]
        if pred.dtype not in _MAP_DTYPES:
            big = torch.iinfo(torch.int32).max
            pred = pred.clamp(-1, big).to(torch.int32)      # whatever does not fit is no class either way
        src = pred = pred.contiguous()
    applied = PP.applied_mask(applied_labels, Cc)
    if B < 1 or min(D, H, W) < 1 or max(D, H, W) > 65535 or D * H * W >= 2 ** 31:
        raise ValueError(f"{name}: batch {B} of {D}x{H}x{W} volumes (sides 1..65535, below 2^31 voxels)")
    return logits, pred, src, B, Cc, D, H, W, applied, conn


def _cpu_class_map(logits, pred, Cc, applied):
    """what the numpy restatements take for CPU tensors: (the class map as an array, the list of applied labels)"""
    cls = torch.stack([first_max_argmax(x) for x in logits]) if logits is not None else pred
    return cls.numpy(), [c for c in range(Cc) if (applied >> c) & 1]


def keep_largest_component(logits=None, pred=None, num_classes=None, applied_labels=None, independent=True, connectivity=None, out_dtype=torch.uint8,
                           stats=False):
    """Keep-largest-connected-component filter of a class map (miseg_keep_largest, csrc/components.hip; training/postprocess.py states the
    rules): [B, D, H, W] of out_dtype (uint8 / int32) in which every voxel of an applied class outside that class's largest component
    (independent) or outside the largest component of all applied classes together (independent=False) is 0.  The map is the first-maximum
    argmax of fp32 `logits` [B, C, D, H, W], or the integer map `pred` [B, (1,) D, H, W] with `num_classes` classes (values outside
    [0, num_classes) are copied through).  applied_labels: None = every class but 0.  connectivity 1 / 2 / 3 (None = 3).  stats=True also
    returns int64 [B, C, 3]: voxels of class c before, kept, components rooted in class c.  Only enqueues (no read-back): graph-capturable.
    CPU tensors take the numpy restatement (postprocess.keep_largest_numpy)."""
    from ..training import postprocess as PP
    logits, pred, src, B, Cc, D, H, W, applied, conn = _class_map_source("keep_largest_component", logits, pred, num_classes, applied_labels,
                                                                         connectivity, out_dtype)
    if not src.is_cuda:
        cls, labels = _cpu_class_map(logits, pred, Cc, applied)
        out, st = PP.keep_largest_numpy(cls, Cc, labels, independent, conn, return_stats=True)
        out = torch.from_numpy(out).to(out_dtype)
        return (out, torch.from_numpy(st)) if stats else out
    dev = src.device
    out = torch.empty(B, D, H, W, dtype=out_dtype, device=dev)
    st = torch.empty(B, Cc, 3, dtype=torch.int64, device=dev) if stats else None
    ws = torch.empty(max(int(L.load().miseg_keep_largest_workspace_bytes(B, D, H, W)), 1), dtype=torch.uint8, device=dev)
    _call("miseg_keep_largest", L.KeepLargest(C.sizeof(L.KeepLargest), _ptr(logits), _ptr(pred), _MAP_DTYPES[pred.dtype] if pred is not None else 0,
                                              B, Cc, D, H, W, applied, int(bool(independent)), conn, _ptr(ws), _ptr(out), _MAP_DTYPES[out_dtype], _ptr(st)))
    return (out, st) if stats else out


def fill_holes(logits=None, pred=None, num_classes=None, applied_labels=None, connectivity=None, out_dtype=torch.uint8, stats=False):
    """Fill-holes filter of a class map (miseg_fill_holes, csrc/components.hip; training/postprocess.py and DESIGN.md section 7.8 state the
    rules): [B, D, H, W] of out_dtype (uint8 / int32) in which, label after label in ascending order, every component of the voxels that are
    not the label and that touches no face of the volume has become the label.  The map is the first-maximum argmax of fp32 `logits`
    [B, C, D, H, W], or the integer map `pred` [B, (1,) D, H, W] with `num_classes` classes (a value outside [0, num_classes) is passable, is
    overwritten inside a hole and copied through elsewhere).  applied_labels: None = every class but 0; 0 is discarded.  connectivity 1 / 2 / 3
    (None = 3) is that of the hole.  stats=True also returns int64 [B, C]: voxels the pass of label c changed to c.  Only enqueues (no
    read-back): graph-capturable.  CPU tensors take the numpy restatement (postprocess.fill_holes_numpy)."""
    from ..training import postprocess as PP
    logits, pred, src, B, Cc, D, H, W, applied, conn = _class_map_source("fill_holes", logits, pred, num_classes, applied_labels, connectivity, out_dtype)
    applied &= ~1
    if not src.is_cuda:
        cls, labels = _cpu_class_map(logits, pred, Cc, applied)
        out, st = PP.fill_holes_numpy(cls, Cc, labels, conn, return_stats=True)
        out = torch.from_numpy(out).to(out_dtype)
        return (out, torch.from_numpy(st)) if stats else out
    dev = src.device
    out = torch.empty(B, D, H, W, dtype=out_dtype, device=dev)
    st = torch.empty(B, Cc, dtype=torch.int64, device=dev) if stats else None
    ws = torch.empty(max(int(L.load().miseg_fill_holes_workspace_bytes(B, D, H, W)), 1), dtype=torch.uint8, device=dev)
    _call("miseg_fill_holes", L.FillHoles(C.sizeof(L.FillHoles), _ptr(logits), _ptr(pred), _MAP_DTYPES[pred.dtype] if pred is not None else 0,
                                          B, Cc, D, H, W, applied, conn, _ptr(ws), _ptr(out), _MAP_DTYPES[out_dtype], _ptr(st)))
    return (out, st) if stats else out


def _export_tables(Cc, dims, dev, tables, axes, lut):
    """the checked arguments both forms of label_export share: (lut as int64 on dev, the three int32 tables, per logits axis (first index, count))"""
    if sorted(int(a) for a in axes) != [0, 1, 2] or len(tables) != 3:
        raise ValueError(f"label_export: axes {tuple(axes)} are not a permutation of (0, 1, 2)")
    if not 1 <= Cc <= 64:
        raise ValueError(f"label_export: {Cc} channels (1..64)")
    lut = torch.as_tensor(lut).to(device=dev, dtype=torch.int64)
    if lut.shape != (Cc,):
        raise ValueError(f"label_export: lut of shape {tuple(lut.shape)} for {Cc} classes")
    tabs, box = [], [None] * 3
    for a in range(3):
        t = torch.as_tensor(tables[a]).to(device=dev, dtype=torch.int32).contiguous()
        if t.dim() != 1 or t.numel() == 0:
            raise ValueError(f"label_export: table {'XYZ'[a]} must be a non-empty vector")
        lo, hi = (int(v) for v in t.aminmax())
        k = int(axes[a])
        if lo < 0 or hi >= dims[k]:
            raise ValueError(f"label_export: table {'XYZ'[a]} spans [{lo}, {hi}], outside the logits side {dims[k]}")
        tabs.append(t)
        box[k] = (lo, hi - lo + 1)
    return lut, tabs, box


def label_export(logits, tables, axes, lut, dtype=torch.uint16, pred=None):
    """[nz, ny, nx] label map (C-contiguous: a NIfTI file's Fortran order) of out[z][y][x] = lut[argmax_c logits[c][i_D][i_H][i_W]], the
    logits index along axes[a] being tables[a][coordinate a] for the output axes a = X, Y, Z (miseg_label_export).  logits fp32 [(1,) C, D, H,
    W]; tables three int32 vectors; axes a permutation of (0, 1, 2); lut int [C]; dtype uint8 / uint16 / uint32 (lut values truncated to it).
    First-maximum argmax (first_max_argmax).  CPU logits take the same arithmetic in torch.  pred= (with logits=None): an integer class map
    [(1,) D, H, W] of len(lut) classes instead of the logits' argmax, e.g. keep_largest_component's; a value outside the classes is written as 0."""
    if (logits is None) == (pred is None):
        raise ValueError("label_export: exactly one of logits / pred")
    if pred is not None:
        return _label_export_map(pred, tables, axes, lut, dtype)
    if logits.dim() == 5 and logits.shape[0] == 1:
        logits = logits[0]
    if logits.dim() != 4 or logits.dtype != torch.float32:
        raise ValueError("label_export: logits must be float32 [C, D, H, W]")
    if dtype not in _EXPORT_DTYPES:
        raise ValueError(f"label_export: dtype {dtype} (uint8 / uint16 / uint32)")
    Cc, dims, dev = logits.shape[0], logits.shape[1:], logits.device
    lut, tabs, box = _export_tables(Cc, dims, dev, tables, axes, lut)
    n = [t.numel() for t in tabs]
    mask = (1 << (8 * _EXPORT_DTYPES[dtype])) - 1
    if not logits.is_cuda:
        cls = first_max_argmax(logits)
        for k in range(3):
            a = [int(v) for v in axes].index(k)
            cls = cls.index_select(k, tabs[a].long())
        cls = cls.permute(int(axes[2]), int(axes[1]), int(axes[0]))
        return (lut & mask)[cls].to(dtype).contiguous()
    logits = logits.contiguous()
    out = torch.empty(n[2], n[1], n[0], dtype=dtype, device=dev)
    lut32 = (lut & mask).to(torch.int32)             # the kernel truncates lut[c] to the element width
    nbytes = L.load().miseg_label_export_workspace_bytes(box[0][1], box[1][1], box[2][1])
    ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
    _call("miseg_label_export", L.LabelExport(C.sizeof(L.LabelExport), _ptr(logits), Cc, *dims, box[0][0], box[1][0], box[2][0], box[0][1], box[1][1],
                                              box[2][1], *n, *(int(a) for a in axes), *(_ptr(t) for t in tabs), _ptr(lut32), _ptr(ws), _ptr(out),
                                              _EXPORT_DTYPES[dtype]))
    return out


def _label_export_map(pred, tables, axes, lut, dtype):
    """label_export of a given class map (miseg_label_export_params.cls): the gather reads the map in place, no argmax launch"""
    if pred.dim() == 4 and pred.shape[0] == 1:
        pred = pred[0]
    if pred.dim() != 3 or pred.dtype not in _MAP_DTYPES:
        raise ValueError("label_export: pred must be a uint8 / int32 class map [D, H, W]")
    if dtype not in _EXPORT_DTYPES:
        raise ValueError(f"label_export: dtype {dtype} (uint8 / uint16 / uint32)")
    Cc, dims, dev = int(torch.as_tensor(lut).numel()), pred.shape, pred.device
    lut, tabs, box = _export_tables(Cc, dims, dev, tables, axes, lut)
    n = [t.numel() for t in tabs]
    mask = (1 << (8 * _EXPORT_DTYPES[dtype])) - 1
    if not pred.is_cuda:
        cls = pred.long()
        for k in range(3):
            a = [int(v) for v in axes].index(k)
            cls = cls.index_select(k, tabs[a].long())
        cls = cls.permute(int(axes[2]), int(axes[1]), int(axes[0]))
        known = (cls >= 0) & (cls < Cc)
        return torch.where(known, (lut & mask)[cls.clamp(0, Cc - 1)], torch.zeros_like(cls)).to(dtype).contiguous()
    pred = pred.contiguous()
    out = torch.empty(n[2], n[1], n[0], dtype=dtype, device=dev)
    lut32 = (lut & mask).to(torch.int32)
    _call("miseg_label_export", L.LabelExport(C.sizeof(L.LabelExport), None, Cc, *dims, box[0][0], box[1][0], box[2][0], box[0][1], box[1][1],
                                              box[2][1], *n, *(int(a) for a in axes), *(_ptr(t) for t in tabs), _ptr(lut32), None, _ptr(out),
                                              _EXPORT_DTYPES[dtype], _ptr(pred), _MAP_DTYPES[pred.dtype]))
    return out


_PROB_DTYPES = {torch.float32: 4, torch.uint8: 1}


def _lerp(a, b, t):
    """the export's blend of one level, every operation rounded to fp32 on its own: where t == 0 it is `a` itself (b is not looked at)"""
    return torch.where(t == 0, a, a * (1 - t) + b * t)


def softmax_in_channel_order(x):
    """softmax over dim 0 as miseg_soft_export states it: the maximum by a strict `>` scan from channel 0, e = exp(x - max), the sum taken
    in channel order, e / sum"""
    mx = x[0]
    for c in range(1, x.shape[0]):
        mx = torch.where(x[c] > mx, x[c], mx)
    e = torch.exp(x - mx[None])
    total = torch.zeros_like(mx)
    for c in range(x.shape[0]):
        total = total + e[c]
    return e / total[None]


def quantize_unit(p):
    """fp32 in [0, 1] -> uint8 as the kernel writes it: min(255, floor(p * 255 + 0.5)), a NaN gives 0"""
    q = torch.floor(p * 255.0 + 0.5).clamp(0, 255)
    return torch.where(p == p, q, torch.zeros_like(q)).to(torch.uint8)


def soft_export(scores, tables, axes, lut, dtype=torch.uint16, softmax=True, want_labels=True, probabilities=None, unit_range=False):
    """(labels or None, prob or None): the class scores blended trilinearly onto the file's grid, then the first-maximum argmax through lut
    (miseg_soft_export).  scores fp32 [(1,) C, D, H, W]; tables[a] = (lo, hi, t) for the output axes a = X, Y, Z: the
    two taps along scores axis axes[a] (int32, lo <= hi <= lo + 1) and the weight of the hi tap (fp32), as
    data/preprocess.py::PredictionGeometry.lerp_tables builds them; lut int [C]; dtype uint8 / uint16 / uint32 of the labels [nz, ny, nx].
    softmax: the scores are logits and their softmax is what is blended.  probabilities: None | torch.float32 | torch.uint8, the element type of
    the blended scores [C, nz, ny, nx] (an [X, Y, Z, C] NIfTI's Fortran order); uint8 (floor(p * 255 + 0.5)) needs softmax, or unit_range=True:
    the caller declares the scores to lie in [0, 1].  Device tensors take the kernel; CPU tensors take the same arithmetic in torch fp32,
    operation by operation."""
    if scores.dim() == 5 and scores.shape[0] == 1:
        scores = scores[0]
    if scores.dim() != 4 or scores.dtype != torch.float32:
        raise ValueError("soft_export: scores must be float32 [C, D, H, W]")
    if dtype not in _EXPORT_DTYPES:
        raise ValueError(f"soft_export: dtype {dtype} (uint8 / uint16 / uint32)")
    if probabilities is not None and probabilities not in _PROB_DTYPES:
        raise ValueError(f"soft_export: probabilities {probabilities} (None / float32 / uint8)")
    if not want_labels and probabilities is None:
        raise ValueError("soft_export: nothing to return (want_labels=False and probabilities=None)")
    if probabilities == torch.uint8 and not (softmax or unit_range):
        raise ValueError("soft_export: uint8 probabilities need scores in [0, 1]: softmax=True, or unit_range=True for scores that already are")
    if len(tables) != 3 or any(len(t) != 3 for t in tables):
        raise ValueError("soft_export: tables must be three (lo, hi, t) triples, one per output axis X, Y, Z")
    Cc, dims, dev = scores.shape[0], scores.shape[1:], scores.device
    # the checks read the tables on the host, where lerp_tables built them (device tables are copied back once)
    host = [[torch.as_tensor(v).detach().cpu().contiguous() for v in t] for t in tables]
    host = [(lo.to(torch.int32), hi.to(torch.int32), t.to(torch.float32)) for lo, hi, t in host]
    for a, (lo, hi, t) in enumerate(host):
        if lo.dim() != 1 or lo.numel() == 0 or hi.shape != lo.shape or t.shape != lo.shape:
            raise ValueError(f"soft_export: table {'XYZ'[a]} must be three non-empty vectors of one length")
        if bool(((hi < lo) | (hi > lo + 1)).any()):
            raise ValueError(f"soft_export: table {'XYZ'[a]} has a hi outside [lo, lo + 1]")
    lut, _, box = _export_tables(Cc, dims, dev, [torch.cat([lo, hi]) for lo, hi, _ in host], axes, lut)
    axes = [int(a) for a in axes]
    n = [t[0].numel() for t in host]
    mask = (1 << (8 * _EXPORT_DTYPES[dtype])) - 1
    if not scores.is_cuda:
        x = softmax_in_channel_order(scores) if softmax else scores
        role = [axes.index(k) for k in range(3)]                  # the output axis that indexes scores axis k

        def taps(k, which):
            shape = [1, 1, 1, 1]
            shape[1 + k] = -1
            return host[role[k]][which].view(shape)

        def at(bd, bh, bw):
            v = x.index_select(1, host[role[0]][bd].long()).index_select(2, host[role[1]][bh].long())
            return v.index_select(3, host[role[2]][bw].long())

        tD, tH, tW = taps(0, 2), taps(1, 2), taps(2, 2)
        c = [[_lerp(at(bd, bh, 0), at(bd, bh, 1), tW) for bh in (0, 1)] for bd in (0, 1)]
        v = _lerp(_lerp(c[0][0], c[0][1], tH), _lerp(c[1][0], c[1][1], tH), tD)
        v = v.permute(0, 1 + axes[2], 1 + axes[1], 1 + axes[0]).contiguous()             # [C, nz, ny, nx]
        labels = (lut & mask)[first_max_argmax(v)].to(dtype).contiguous() if want_labels else None
        prob = None if probabilities is None else (v if probabilities == torch.float32 else quantize_unit(v))
        return labels, prob
    scores = scores.contiguous()
    devt = [tuple(v.to(dev) for v in t) for t in host]
    labels = torch.empty(n[2], n[1], n[0], dtype=dtype, device=dev) if want_labels else None
    prob = torch.empty(Cc, n[2], n[1], n[0], dtype=probabilities, device=dev) if probabilities is not None else None
    lut32 = (lut & mask).to(torch.int32)             # the kernel truncates lut[c] to the element width
    nbytes = int(L.load().miseg_soft_export_workspace_bytes(Cc, box[0][1], box[1][1], box[2][1], int(bool(softmax))))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    vp3 = C.c_void_p * 3
    _call("miseg_soft_export", L.SoftExport(
        C.sizeof(L.SoftExport), _ptr(scores), Cc, *dims, box[0][0], box[1][0], box[2][0], box[0][1], box[1][1], box[2][1], *n, *axes,
        vp3(*(_ptr(t[0]) for t in devt)), vp3(*(_ptr(t[1]) for t in devt)), vp3(*(_ptr(t[2]) for t in devt)),
        vp3(*(t[0].data_ptr() for t in host)), vp3(*(t[1].data_ptr() for t in host)), _ptr(lut32), int(bool(softmax)), int(bool(unit_range)),
        _ptr(ws), _ptr(labels), _EXPORT_DTYPES[dtype] if want_labels else 0, _ptr(prob), _PROB_DTYPES[probabilities] if prob is not None else 0))
    return labels, prob


def stitch_windows(win, out, starts, roi, count=None, slab=None, weight=None, wsum=None):
    """win fp32 [nd*nh*nw, C, rd, rh, rw] (the windows of the nd depth layers `starts[0]`, all resident), out fp32 [C, D, H, W];
    starts = (list_d, list_h, list_w).  slab = (d_begin, d_count): write only these depths of `out` from the resident layers (which then
    need not cover the whole depth axis, miseg_stitch_params).  weight: fp32 [rd, rh, rw] importance map of a window on win's device
    (MONAI mode="gaussian" / roi_weight_map): out = sum(weight * win) / sum(weight) instead of sum(win) / count; None is the constant blend.
    wsum (only with weight): fp32 [D, H, W], receives the summed weights."""
    nd, nh, nw = (len(s) for s in starts)
    Cc, D, H, W = out.shape
    assert win.dtype == torch.float32 and out.dtype == torch.float32 and win.is_contiguous() and out.is_contiguous()
    if tuple(win.shape) != (nd * nh * nw, Cc) + tuple(roi):
        raise ValueError(f"stitch_windows: window buffer {tuple(win.shape)} does not match {nd}x{nh}x{nw} windows of {tuple(roi)} x {Cc} channels")
    arr = [(C.c_int32 * len(s))(*s) for s in starts]
    if count is not None:
        assert count.dtype == torch.int16 and count.is_contiguous() and tuple(count.shape) == (D, H, W)
    if weight is not None:
        if tuple(weight.shape) != tuple(roi):
            raise ValueError(f"stitch_windows: weight map {tuple(weight.shape)} does not have the roi's shape {tuple(roi)}")
        if weight.dtype != torch.float32 or not weight.is_contiguous() or weight.device != win.device:
            raise ValueError(f"stitch_windows: the weight map must be a contiguous fp32 tensor on {win.device} (got {weight.dtype} on {weight.device})")
    if wsum is not None:
        if weight is None:
            raise ValueError("stitch_windows: wsum is the sum of the weights: it needs a weight map")
        if tuple(wsum.shape) != (D, H, W) or wsum.dtype != torch.float32 or not wsum.is_contiguous() or wsum.device != win.device:
            raise ValueError(f"stitch_windows: wsum must be a contiguous fp32 tensor of shape {(D, H, W)} on {win.device}")
    d0, dn = slab if slab is not None else (0, 0)
    _call("miseg_stitch_windows", L.Stitch(C.sizeof(L.Stitch), _ptr(win), _ptr(out), _ptr(count), Cc, D, H, W, roi[0], roi[1], roi[2], nd, nh, nw,
                                           C.cast(arr[0], C.c_void_p), C.cast(arr[1], C.c_void_p), C.cast(arr[2], C.c_void_p), int(d0), int(dn),
                                           _ptr(weight), _ptr(wsum)))
    return out


# ------------------------------------------------------------------------------------------ flip TTA / model ensembling
def _ensemble_vector(name, what, value, Cc):
    """a scalar or per-class weight / scale as a list of Cc python floats rounded to fp32, finite and non-negative"""
    v = torch.as_tensor(value, dtype=torch.float64).reshape(-1).cpu()
    if v.numel() == 1:
        v = v.repeat(Cc)
    if v.numel() != Cc:
        raise ValueError(f"{name}: {what} of {v.numel()} values for {Cc} classes (a scalar, or one value per class)")
    if not bool(torch.isfinite(v).all()) or bool((v < 0).any()):
        raise ValueError(f"{name}: {what} {v.tolist()} must be finite and non-negative")
    return v.to(torch.float32).tolist()


def _ensemble_args(name, src, acc, flip, kind, weight, out_scale):
    if kind not in L.ENSEMBLE_KINDS:
        raise ValueError(f"{name}: kind {kind!r} is not one of {tuple(L.ENSEMBLE_KINDS)}")
    if not (torch.is_tensor(src) and torch.is_tensor(acc)) or src.dtype != torch.float32 or acc.dtype != torch.float32 or src.dim() != 5:
        raise ValueError(f"{name}: src and acc must be float32 [B, C, D, H, W] tensors")
    if src.shape != acc.shape or src.device != acc.device:
        raise ValueError(f"{name}: src {tuple(src.shape)} on {src.device} and acc {tuple(acc.shape)} on {acc.device} differ")
    if not (src.is_contiguous() and acc.is_contiguous()):
        raise ValueError(f"{name}: src and acc must be contiguous")
    Cc = src.shape[1]
    if not 1 <= Cc <= 64 or min(src.shape) < 1:
        raise ValueError(f"{name}: shape {tuple(src.shape)} (1..64 channels, no empty dimension)")
    flip = tuple(flip)
    if len(flip) != 3:
        raise ValueError(f"{name}: flip {flip} is not one flag per spatial axis (D, H, W)")
    bits = sum(1 << a for a in range(3) if flip[a])
    w = _ensemble_vector(name, "weight", weight, Cc)
    s = None if out_scale is None else _ensemble_vector(name, "out_scale", out_scale, Cc)
    return bits, L.ENSEMBLE_KINDS[kind], w, s


def ensemble_accumulate_torch(src, acc, *, flip=(False, False, False), kind="mean_logits", weight=1.0, first=False, out_scale=None):
    """The arithmetic of miseg_ensemble_accumulate in torch, one rounded fp32 (the tensors' dtype: float64 tensors give the float64
    restatement) op per step, in the kernel's order: un-flip, the term t (the logits | softmax over dim 1: maximum subtracted, exp, summed in
    channel order, times 1 / sum | the one-hot of first_max_argmax), w_c * t, acc + that unless first, times out_scale[c] when given.  Writes
    and returns acc.  Kinds mean_logits and vote give the kernel's bits; mean_prob differs by the two exp implementations."""
    dims = [2 + a for a in range(3) if flip[a]]
    x = torch.flip(src, dims) if dims else src
    Cc = x.shape[1]
    shape = (1, Cc, 1, 1, 1)
    if kind == "mean_logits":
        t = x
    elif kind == "mean_prob":
        e = torch.exp(x - x.amax(dim=1, keepdim=True))
        total = e[:, 0:1]
        for c in range(1, Cc):
            total = total + e[:, c:c + 1]
        t = e * (1.0 / total)
    elif kind == "vote":
        arg = torch.stack([first_max_argmax(v) for v in x])
        t = torch.stack([(arg == c) for c in range(Cc)], 1).to(x.dtype)
        weight = 1.0
    else:
        raise ValueError(f"ensemble_accumulate: kind {kind!r} is not one of {tuple(L.ENSEMBLE_KINDS)}")
    w = torch.as_tensor(weight, dtype=torch.float64).reshape(-1).to(torch.float32).to(device=x.device, dtype=x.dtype)
    term = t * (w.reshape(shape) if w.numel() == Cc else w)
    total = term if first else acc + term
    if out_scale is not None:
        s = torch.as_tensor(out_scale, dtype=torch.float64).reshape(-1).to(torch.float32).to(device=x.device, dtype=x.dtype)
        total = total * (s.reshape(shape) if s.numel() == Cc else s)
    acc.copy_(total)
    return acc


def ensemble_accumulate(src, acc, *, flip=(False, False, False), kind="mean_logits", weight=1.0, first=False, out_scale=None):
    """Fold one ensemble member into the accumulator (miseg_ensemble_accumulate, csrc/ensemble.hip):
    acc' = fl(fl(acc + fl(w_c * t_c)) * s_c) with t the member's term at the voxel that `flip` (one flag per spatial axis D, H, W: the member
    was predicted on the volume mirrored along it) maps onto acc's voxel.  src, acc: contiguous fp32 [B, C, D, H, W] on one device, not
    overlapping.  kind "mean_logits" | "mean_prob" | "vote"; weight: a scalar or one value per class (ignored by "vote"); first: acc is
    written and not read (it may be torch.empty); out_scale: None, a scalar or one value per class, multiplied in after the add (the last
    member's 1 / sum of weights).  Writes and returns acc; only enqueues: graph-capturable.  CPU tensors take ensemble_accumulate_torch."""
    bits, k, w, s = _ensemble_args("ensemble_accumulate", src, acc, flip, kind, weight, out_scale)
    if not src.is_cuda:
        return ensemble_accumulate_torch(src, acc, flip=flip, kind=kind, weight=w, first=first, out_scale=s)
    B, Cc, D, H, W = src.shape
    p = L.Ensemble(C.sizeof(L.Ensemble), _ptr(src), _ptr(acc), B, Cc, D, H, W, bits, k, int(bool(first)), int(s is not None),
                   (C.c_float * 64)(*w), (C.c_float * 64)(*(s or ())))      # (a ctypes array is zero beyond the values given)
    _call("miseg_ensemble_accumulate", p, prof=("ensemble_accumulate", 0.0, _nb(src, acc) + (0.0 if first else _nb(acc))))
    return acc


# ------------------------------------------------------------------------------------------ dropout / stochastic depth
class _DropState:
    """keys of the counter-based dropout masks: `seed` (host, torch.initial_seed() unless set), a call counter that tells the call sites
    of one step apart (reset by begin_step / begin_forward) and a DEVICE step counter advanced once per step - under hipGraph replay the
    first two are baked into the graph, the third is what makes every replay draw new masks."""

    def __init__(self):
        self.seed, self.calls, self.step_dev = None, 0, None

    def next_key(self, device):
        if self.seed is None:
            self.seed = torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
        if self.step_dev is None or self.step_dev.device != device:
            self.step_dev = torch.zeros(1, dtype=torch.int64, device=device)
        self.calls += 1
        # the step counter is SNAPSHOT per call: the backward pass of this forward may run after a later forward advanced the counter
        snap = torch.empty(1, dtype=torch.int64, device=device)
        L.check(L.load().miseg_counter_copy(_ptr(snap), _ptr(self.step_dev), _stream()), "counter_copy")
        return self.seed, self.calls, snap

    def advance(self):
        """once per training step (arena.begin_step / GraphedStep._run / the nets' forward when nobody manages the step)"""
        self.calls = 0
        if self.step_dev is not None:
            L.check(L.load().miseg_counter_add(_ptr(self.step_dev), 1, _stream()), "counter_add")


DROP = _DropState()


def dropout_apply(x, p, key, rows_per_sample=0):
    """y = x * mask(key) / (1 - p); key = (seed, stream_id, step_dev) from DROP.next_key: the same key reproduces the same mask (backward)"""
    ld, n, Cc = rows(x)
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    seed, sid, step = key
    _call("miseg_dropout", L.Dropout(C.sizeof(L.Dropout), _ptr(x), ld, _ptr(y), rows(y)[0], n, Cc, _dt(x), rows_per_sample, float(p), seed, sid, _ptr(step)))
    return y
