"""Optimiser step of the whole model as ONE kernel launch over the gradient arena.

The reference builds torch.optim.AdamW / Adam / SGD(nesterov) over `self.parameters()` (networks/lightning_monai.py:255-278); torch
skips a parameter whose `grad is None` completely -- no update, no weight decay, no step count -- which is what happens every step to the
conditional-norm rows of the modality that is absent from the batch.  `ArenaOptimizer` keeps that rule: the "used" flags of
runtime/arena.py::ParamArena (set by the weight-gradient kernels' autograd nodes, max-reduced over ranks under DDP) travel to the
device and the kernel leaves unused tensors alone, with a per-parameter step count for Adam's bias correction.  The moments live in two
flat fp32 buffers laid out like the arena."""
import ctypes as C

import torch

from ..hip import lib as L
from ..hip import ops

KINDS = {"adamw": L.OPT_ADAMW, "adam": L.OPT_ADAM, "sgd": L.OPT_SGD_NESTEROV}


def clip_options(gradient_clip_val=None, gradient_clip_algorithm="norm", skip_nonfinite=False, track_grad_norm=False):
    """(MISEG_CLIP_* mode, clip value, guard on, tracking on) of ArenaOptimizer's clipping arguments; ValueError for what they do not allow.
    track_grad_norm also takes the command line's spelling: -1 = off, 2 = the L2 norm (the only norm the kernel forms)."""
    if gradient_clip_algorithm not in L.CLIP_MODES:
        raise ValueError("gradient_clip_algorithm {!r}: 'norm' or 'value'".format(gradient_clip_algorithm))
    val = None if gradient_clip_val is None else float(gradient_clip_val)
    if val is not None and not (0.0 < val < float("inf")):
        raise ValueError("gradient_clip_val {!r} must be finite and > 0 (None: no clipping)".format(gradient_clip_val))
    if isinstance(track_grad_norm, bool) or track_grad_norm is None:
        track = bool(track_grad_norm)
    elif track_grad_norm in (-1, 2):
        track = track_grad_norm == 2
    else:
        raise ValueError("track_grad_norm {!r}: only the L2 norm (2 / True) is computed; -1 / False turns it off".format(track_grad_norm))
    return (L.CLIP_NONE if val is None else L.CLIP_MODES[gradient_clip_algorithm]), (0.0 if val is None else val), bool(skip_nonfinite), track


class ArenaOptimizer:
    """The optimiser of the module docstring.  Its step controls beyond the hyper-parameters are gradient clipping and the non-finite guard
    (Lightning's Trainer(gradient_clip_val, gradient_clip_algorithm, track_grad_norm)), all off by default - the step then issues exactly the
    launches it always did:

      gradient_clip_val, gradient_clip_algorithm="norm"   every gradient is scaled by min(1, clip / (global L2 norm + 1e-6)): torch's clip_grad_norm_
      gradient_clip_val, gradient_clip_algorithm="value"  every gradient element is clamped to [-clip, clip]: torch's clip_grad_value_
      skip_nonfinite                                      a step whose gradient norm is inf or NaN changes nothing (weights, moments, packs, step counts)
      track_grad_norm                                     the norm (and `grad_norms`, one per parameter) is computed even when nothing else needs it

    The norm is two launches over the arena in front of the update (miseg_grad_norm), its result stays on the device (`clip_record`, `grad_norm`)
    and the update kernels read it there: no host read, so the step is capturable.  Unlike torch, which clips in place, the arena is NOT modified:
    `p.grad` shows the unclipped gradient after the step.  Under data parallelism step() runs behind the all-reduce, so every rank computes the
    same norm from the same bytes."""

    def __init__(self, arena, kind="adamw", lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, momentum=0.99, gradient_clip_val=None,
                 gradient_clip_algorithm="norm", skip_nonfinite=False, track_grad_norm=False):
        if kind not in KINDS:
            raise ValueError("Optimization {} not implemented, please chose another optimizer.".format(kind))
        self.clip_mode, self.clip_val, self.skip_nonfinite, self.track_grad_norm = clip_options(gradient_clip_val, gradient_clip_algorithm, skip_nonfinite,
                                                                                               track_grad_norm)
        # which launches the options add: the norm in front (norm clipping, the guard, tracking) and the clipped forms of the update (all but tracking)
        self._need_norm = self.clip_mode == L.CLIP_NORM or self.skip_nonfinite or self.track_grad_norm
        self._clipped = self.clip_mode != L.CLIP_NONE or self.skip_nonfinite
        self._rec = self._norm_ws = self.grad_norms = None
        self.arena, self.kind = arena, kind
        self.lr, self.betas, self.eps, self.weight_decay, self.momentum = float(lr), betas, float(eps), float(weight_decay), float(momentum)
        dev = arena.flat.device
        self.state1 = torch.zeros_like(arena.flat)
        self.state2 = torch.zeros_like(arena.flat) if kind != "sgd" else None
        n = len(arena.params)
        self.steps = torch.zeros(n, dtype=torch.int32, device=dev)
        self.used = torch.ones(n, dtype=torch.int32, device=dev)
        self._used_cache = {}      # bytes of a step's "used" flags -> the same flags on the device (one entry per present-modality set)
        descs = (L.OptDesc * n)()
        block0 = 0
        for i, (p, off) in enumerate(zip(arena.params, arena._offs)):
            if not p.is_contiguous():
                raise ValueError("parameters must be contiguous float32")
            descs[i] = L.OptDesc(p.data_ptr(), off, p.numel(), block0)
            block0 += (p.numel() + L.OPT_BLOCK - 1) // L.OPT_BLOCK
        self._ptrs = [p.data_ptr() for p in arena.params]
        self._table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
        self._blocks = block0
        self.lr_dev = None
        self._early = None          # (table, index, blocks, n) of the parameters updated by step_early(), and of the rest
        self._late = None
        self._early_done = False

    @property
    def clipping(self):
        """True when any of clipping / the guard / norm tracking is on (the step then starts with the norm launches or ends in the clipped kernels)"""
        return self._need_norm or self._clipped

    def _clip_buffers(self):
        """the 32-byte record (miseg_grad_clip_record, zeroed once: its counters run on), the norm workspace and the per-parameter norms.  Allocated
        ONCE: a captured hipGraph holds their addresses."""
        if self._rec is None and self.clipping:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ArenaOptimizer.prepare() must run before a step with clipping is captured (it allocates the clip record)")
            dev = self.state1.device
            self._rec = torch.zeros(C.sizeof(L.GradClipRecord) // 4, dtype=torch.int32, device=dev)
            if self._need_norm:
                n = len(self.arena.params)
                self._norm_ws = torch.empty(L.load().miseg_grad_norm_workspace_bytes(self._blocks, n) // 8, dtype=torch.float64, device=dev)
                if self.track_grad_norm:
                    self.grad_norms = torch.zeros(n, dtype=torch.float32, device=dev)
        return self._rec

    @property
    def clip_record(self):
        """the device record of the last step (int32 [8] over miseg_grad_clip_record: norm, coef as float bits, finite, skip, seen, clipped, skipped)"""
        return self._clip_buffers()

    @property
    def grad_norm(self):
        """global L2 norm of the last step's gradient BEFORE clipping: a 0-dim fp32 device view of the record (no sync; static under graph replay)"""
        if not self._need_norm:
            raise ValueError("no gradient norm is computed: turn on norm clipping, skip_nonfinite or track_grad_norm")
        return self._clip_buffers()[:1].view(torch.float32)[0]

    def clip_stats(self):
        """the record read back once (one device-to-host copy): norm, coef, finite, seen, clipped, skipped"""
        if not self.clipping:
            raise ValueError("clipping, the non-finite guard and norm tracking are all off")
        r = self._clip_buffers().cpu()
        f = r[:2].view(torch.float32)
        return {"norm": float(f[0]), "coef": float(f[1]), "finite": int(r[2]), "seen": int(r[4]), "clipped": int(r[5]), "skipped": int(r[6])}

    def _launch_norm(self):
        n = len(self.arena.params)
        p = L.GradNorm(C.sizeof(L.GradNorm), self.clip_mode, self._table.data_ptr(), n, self._blocks, self.arena.flat.data_ptr(), self.used.data_ptr(),
                       self.clip_val if self.clip_mode == L.CLIP_NORM else 0.0, int(self.skip_nonfinite), self._norm_ws.data_ptr(), self._rec.data_ptr(),
                       self.grad_norms.data_ptr() if self.grad_norms is not None else None)
        ops._call("miseg_grad_norm", p)

    def _clip_extra(self):
        """(record, mode, value): the trailing arguments of the clipped entry points; value mode without the guard reads no record"""
        rec = self._rec.data_ptr() if (self.clip_mode != L.CLIP_VALUE or self.skip_nonfinite) else None
        return (C.c_void_p(rec), self.clip_mode, C.c_float(self.clip_val if self.clip_mode != L.CLIP_NONE else 0.0))

    def _subset_table(self, sel):
        """(descriptor table, index, blocks, count) of the arena parameters `sel` (a list of indices) on the device"""
        dev = self.state1.device
        descs, index, block0 = (L.OptDesc * len(sel))(), [], 0
        for j, i in enumerate(sel):
            p = self.arena.params[i]
            descs[j] = L.OptDesc(p.data_ptr(), self.arena._offs[i], p.numel(), block0)
            block0 += (p.numel() + L.OPT_BLOCK - 1) // L.OPT_BLOCK
            index.append(i)
        return (torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev), torch.tensor(index, dtype=torch.int32, device=dev), block0, len(sel))

    def _fused_tables(self):
        """Round 5: the 3x3x3 conv weights (55 of C-Swin-UNETR's 62 M parameters) are updated by the launch that also writes their packs
        (miseg_opt_step_pack_conv3), everything else by the element-wise launch in front of it.  Returns (rest table | None, map, pack table) once
        the arena holds a current conv-pack table whose weights are all trainable arena parameters, else None (the plain one-launch step)."""
        a = self.arena
        if self._early is not None or not a.flat.is_cuda or a._ptable is None or a._pdirty or a.dtype not in (torch.float32, torch.bfloat16):
            return None
        key = a._ptable[0].data_ptr()
        cur = self.__dict__.get("_fused")
        if cur is not None and cur[0] == key:
            return cur[1]
        if torch.cuda.is_current_stream_capturing():
            return None                                  # (tables are uploaded eagerly: the warm-up steps in front of a capture build them)
        idx_of = {id(p): i for i, p in enumerate(a.params)}
        maps, conv = (L.OptPackMap * len(a._packs))(), set()
        for j, ent in enumerate(a._packs.values()):
            i = idx_of.get(id(ent[0]))
            if i is None or not ent[4]:                  # a frozen weight has packs but no arena slot: the plain step handles such models
                self._fused = (key, None)
                return None
            maps[j] = L.OptPackMap(a._offs[i], i, 0)
            conv.add(i)
        rest = [i for i in range(len(a.params)) if i not in conv]
        tabs = (self._subset_table(rest) if rest else None, torch.frombuffer(bytearray(bytes(maps)), dtype=torch.uint8).to(self.state1.device), a._ptable)
        self.__dict__.setdefault("_retired", []).append(cur)      # a captured hipGraph may still point at the old tables
        self._fused = (key, tabs)
        return tabs

    def prepare(self):
        """build (and upload) the launch tables now - call before capturing a step that contains `step()` into a hipGraph"""
        self._fused_tables()
        self._clip_buffers()

    def _launch_pack(self, tabs, lr, count_n):
        _, maps, (ptab, n, tiles) = tabs
        a = self.arena
        p = L.OptStep(C.sizeof(L.OptStep), KINDS[self.kind], None, 0, 0, a.flat.data_ptr(),
                      self.state1.data_ptr(), self.state2.data_ptr() if self.state2 is not None else None, self.used.data_ptr(), self.steps.data_ptr(),
                      self.lr if lr is None else float(lr), self.betas[0], self.betas[1], self.eps, self.weight_decay, self.momentum,
                      self.lr_dev.data_ptr() if self.lr_dev is not None else None, a.params_version_ptr(), None, count_n)
        state = a._ver(3)[1]
        if self._clipped:
            L.check(L.load().miseg_opt_step_pack_conv3_clipped(C.byref(p), C.c_void_p(ptab.data_ptr()), C.c_void_p(maps.data_ptr()), n, tiles,
                                                               L.F32 if a.dtype == torch.float32 else L.BF16, state, *self._clip_extra(), ops._stream()),
                    "opt_step_pack_conv3_clipped")
            return
        L.check(L.load().miseg_opt_step_pack_conv3(C.byref(p), C.c_void_p(ptab.data_ptr()), C.c_void_p(maps.data_ptr()), n, tiles,
                                                   L.F32 if a.dtype == torch.float32 else L.BF16, state, ops._stream()), "opt_step_pack_conv3")

    def split_early(self, early_params):
        """Two launches per step: `early_params` (parameters whose gradients are final before the end of the backward pass: what
        ParamArena.inline_final_params reports after a step) are updated by step_early() - which the caller may issue on a side stream beside the
        rest of the pass - and all the others by step().  Same arithmetic, same result as the one-launch step (each parameter is touched once).
        Refused with clipping or the guard on: the early launch runs before the gradient norm of the step exists."""
        if self.clipping:
            raise ValueError("split_early: gradient clipping / skip_nonfinite / track_grad_norm need the whole gradient before the first update")
        ids = {id(p) for p in early_params}
        # (tables a captured hipGraph points at by raw address must never be freed: an unchanged set keeps its tables - a second capture, of
        # another modality set, asks again - and replaced ones are retired, not dropped)
        if getattr(self, "_early_ids", None) == ids:
            return
        dev = self.state1.device

        def table(sel):
            descs, index, block0 = (L.OptDesc * len(sel))(), [], 0
            for j, i in enumerate(sel):
                p = self.arena.params[i]
                descs[j] = L.OptDesc(p.data_ptr(), self.arena._offs[i], p.numel(), block0)
                block0 += (p.numel() + L.OPT_BLOCK - 1) // L.OPT_BLOCK
                index.append(i)
            return (torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev), torch.tensor(index, dtype=torch.int32, device=dev), block0, len(sel))
        n = len(self.arena.params)
        early = [i for i in range(n) if id(self.arena.params[i]) in ids]
        late = [i for i in range(n) if id(self.arena.params[i]) not in ids]
        if len(early) != len(ids) or (ids and not late):
            raise ValueError("split_early: parameters that are not in the arena (or nothing left for the second launch)")
        new = (table(early), table(late)) if ids else (None, None)
        self.__dict__.setdefault("_retired", []).append((self._early, self._late))
        self._early, self._late = new
        self._early_ids = ids

    def _launch(self, tab, lr, count_n):
        table, index, blocks, n = tab
        p = L.OptStep(C.sizeof(L.OptStep), KINDS[self.kind], table.data_ptr(), n, blocks, self.arena.flat.data_ptr(),
                      self.state1.data_ptr(), self.state2.data_ptr() if self.state2 is not None else None, self.used.data_ptr(), self.steps.data_ptr(),
                      self.lr if lr is None else float(lr), self.betas[0], self.betas[1], self.eps, self.weight_decay, self.momentum,
                      self.lr_dev.data_ptr() if self.lr_dev is not None else None, self.arena.params_version_ptr(),
                      index.data_ptr() if index is not None else None, count_n)
        if self._clipped:
            ops._call("miseg_opt_step_clipped", p, extra=self._clip_extra())
        else:
            ops._call("miseg_opt_step", p)

    def step_early(self, lr=None):
        """the first launch of a split step (split_early): the `used` flags must be on the device already (set_used_from_arena / a captured
        step's static flags); step() then updates the rest and closes the step"""
        if self._early is None or self._early_done:
            return
        self._launch(self._early, lr, 0)
        self._early_done = True

    def set_used_from_arena(self):
        """copy the host "used" flags of this step (arena.publish / allreduce have settled them) to the device; under hipGraph replay call
        this BEFORE the replay that contains the step"""
        # The flags of a step are one of a handful of patterns (which modalities were in the batch).  Each pattern is uploaded ONCE from a
        # host buffer of its own and then copied device-to-device on the stream: a single pinned staging buffer rewritten every step raced
        # with its own asynchronous upload once the host ran ahead of the device (sync-free loops), and a step then saw the next step's flags.
        key = bytes(1 if p._miseg_used else 0 for p in self.arena.params)
        dev = self._used_cache.get(key)
        if dev is None:      # (grow-only: a captured train step reads the pattern tensor by its raw address - see ParamArena._flags_to_device)
            dev = self._used_cache[key] = torch.tensor(list(key), dtype=torch.int32, device=self.used.device)
        self.used.copy_(dev, non_blocking=True)

    def step(self, lr=None, update_flags=True):
        if [p.data_ptr() for p in self.arena.params] != self._ptrs:
            raise RuntimeError("a parameter was re-allocated after the optimiser was built (e.g. model.to(...)): rebuild the ArenaOptimizer")
        if update_flags:
            if getattr(self.arena, "used_on_device", False):      # a data-parallel exchange left the GLOBAL flags on the device (no host read)
                self.used.copy_(self.arena.used_dev, non_blocking=True)
            else:
                self.set_used_from_arena()
        fused = self._fused_tables()
        if self.clipping:             # the norm of the whole gradient first (two launches); the update kernels read its record on the device
            self._clip_buffers()
            if self._need_norm:
                self._launch_norm()
        if self._early_done:          # the early launch of this step is out: the rest, then the step counts of ALL parameters and the version bump
            self._launch(self._late, lr, len(self.arena.params))
            self._early_done = False
        elif fused is not None:       # everything but the 3x3x3 conv weights, then those together with their packs (which closes the step)
            if fused[0] is not None:
                self._launch(fused[0], lr, 0)
            self._launch_pack(fused, lr, len(self.arena.params))
        else:
            self._launch((self._table, None, self._blocks, len(self.arena.params)), lr, -1)
        # the compute-dtype copies of the parameters are stale now: the kernel bumped the arena's device-side parameter version (the refresh
        # launches of the next step re-lay-out everything); the host-side epoch moves on too, so that eager forwards cast per call until then
        self.arena.epoch += 1

    def state_dict(self):
        return {"kind": self.kind, "state1": self.state1.clone(), "state2": None if self.state2 is None else self.state2.clone(), "steps": self.steps.clone(),
                "lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay, "momentum": self.momentum}

    def load_state_dict(self, sd):
        if sd["kind"] != self.kind or sd["state1"].numel() != self.state1.numel():
            raise ValueError("optimizer state does not match this model / optimiser kind")
        self.state1.copy_(sd["state1"])
        if self.state2 is not None:
            self.state2.copy_(sd["state2"])
        self.steps.copy_(sd["steps"])


def accumulation_scale(k):
    """fl(1 / k) in float32: what miseg_grad_fold multiplies a window's sum by"""
    return float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(k), dtype=torch.float32))


class GradAccumulator:
    """Gradient accumulation over `accumulate_grad_batches` micro-batches on the device (the reference's --iters_to_accumulate,
    utils/trainer.py:33-78; Lightning's --accumulate_grad_batches).  Every micro-batch is a step of its own for the arena
    (zero fill, storing weight-gradient kernels); after its backward pass ONE launch (miseg_grad_fold) adds the arena into `acc`, a second flat
    fp32 buffer laid out like it, and on the micro-batch that closes the window writes the window's mean back into the ARENA, where the
    norm, the update kernels and `p.grad` find it.  Which parameters have a gradient in a micro-batch is the host's `_miseg_used`; the launch
    gets one op code per parameter.  A parameter absent from the whole window keeps `grad is None`: no update, no step count.

        arena.begin_step(); loss.backward(); arena.publish()
        closes = acc.plan(); acc.fold()
        if closes: opt.step()

    The mean is sum-then-scale: fl(fl(g1 + g2 + ..) * fl(1/k)); the scale stays 1/k for a window closed early (`plan(last=True)`), like the
    reference and Lightning.  accumulate_grad_batches == 1: inert - no buffer, no launch, plan() returns True."""

    def __init__(self, optimizer, accumulate_grad_batches):
        k = int(accumulate_grad_batches)
        if k < 1 or k != accumulate_grad_batches:
            raise ValueError("accumulate_grad_batches {!r} must be an integer >= 1".format(accumulate_grad_batches))
        self.opt, self.k = optimizer, k
        self.scale = accumulation_scale(k)
        self.acc = self.ops = None
        self._patterns = {}          # bytes of a micro-batch's op codes -> the same codes on the device (grow-only: see plan())
        self._seen = None            # per parameter: it had a gradient in an earlier micro-batch of the open window
        self._count = 0              # micro-batches of the open window planned so far

    @property
    def active(self):
        return self.k > 1

    def prepare(self):
        """allocate `acc` and the static op-code tensor - ONCE: a captured hipGraph holds their addresses; call before capturing fold()"""
        if self.active and self.acc is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("GradAccumulator.prepare() must run before fold() is captured (it allocates the accumulator)")
            flat = self.opt.arena.flat
            self.acc = torch.empty_like(flat)          # never read before its first write of a window (op 1)
            self.ops = torch.zeros(len(self.opt.arena.params), dtype=torch.int32, device=flat.device)
            self._seen = [False] * len(self.opt.arena.params)

    def closes(self, last=None):
        """whether the coming micro-batch closes the window: the k-th one, or any one with last=True (a short window at the end of an epoch)"""
        return (not self.active) or bool(last) or self._count + 1 >= self.k

    def plan(self, last=None):
        """the host bookkeeping of the coming micro-batch, outside capture and before the launch (or replay) that folds it: reads the
        parameters' `_miseg_used`, uploads the op codes and returns whether this micro-batch closes the window.  On close the window's union
        becomes the parameters' `_miseg_used` / `grad` and the optimiser's device flags, so opt.step(update_flags=False) may follow."""
        if not self.active:
            return True
        self.prepare()
        params = self.opt.arena.params
        closes = self.closes(last)
        used = [bool(p._miseg_used) for p in params]
        key = bytes((L.FOLD_USED if u else 0) | (L.FOLD_EARLIER if a else 0) | (L.FOLD_CLOSE if closes else 0) for u, a in zip(used, self._seen))
        # each distinct pattern is uploaded ONCE from a host buffer of its own and then copied device-to-device on the stream, and no entry is
        # ever dropped: the reasons written in ArenaOptimizer.set_used_from_arena
        dev = self._patterns.get(key)
        if dev is None:
            dev = self._patterns[key] = torch.tensor(list(key), dtype=torch.int32, device=self.ops.device)
        self.ops.copy_(dev, non_blocking=True)
        self._seen = [a or u for u, a in zip(used, self._seen)]
        self._count += 1
        if closes:
            for p, v, u in zip(params, self.opt.arena.views, self._seen):
                p._miseg_used = u
                p.grad = v if u else None
            self.opt.set_used_from_arena()
            self.reset()
        return closes

    def fold(self):
        """enqueue miseg_grad_fold for the micro-batch plan() prepared: one launch and nothing else, so it can be captured"""
        if not self.active:
            return
        if self.acc is None:
            self.prepare()          # (raises under capture)
        opt = self.opt
        p = L.GradFold(C.sizeof(L.GradFold), opt._table.data_ptr(), len(opt.arena.params), opt._blocks, opt.arena.flat.data_ptr(), self.acc.data_ptr(),
                       self.ops.data_ptr(), opt.arena.flat.numel(), self.scale)
        ops._call("miseg_grad_fold", p)

    def reset(self):
        """drop an open window: the next micro-batch starts a new one (`acc` needs no clearing: a window's first use of a slot overwrites it)"""
        if self._seen is not None:
            self._seen = [False] * len(self._seen)
        self._count = 0


def averaging_options(mode="ema", decay=0.999, warmup=False, start_step=0, every=1):
    """(MISEG_AVG_* mode, decay, warm-up on, start, every) of WeightAverager's arguments; ValueError for what miseg_weight_average would refuse"""
    if mode not in L.AVG_MODES:
        raise ValueError("weight averaging mode {!r}: 'ema' or 'swa'".format(mode))
    try:
        d = float(decay)
    except (TypeError, ValueError):
        raise ValueError("decay {!r} must be a number in [0, 1)".format(decay))
    if not (0.0 <= d < 1.0) or not (0.0 <= float(torch.tensor(d, dtype=torch.float32)) < 1.0):          # (what the kernel sees is the float32 of it)
        raise ValueError("decay {!r} must be finite and in [0, 1)".format(decay))
    for name, v, low in (("start_step", start_step, 0), ("every", every, 1)):
        if isinstance(v, bool) or int(v) != v or int(v) < low or int(v) >= 2 ** 31:
            raise ValueError("{} {!r} must be an integer >= {}".format(name, v, low))
    return L.AVG_MODES[mode], d, bool(warmup), int(start_step), int(every)


class WeightAverager:
    """An average of the weights over the optimisation steps, kept on the device beside the arena:

      mode="ema"   avg += (1 - decay) (w - avg) after every `every`-th step from step `start_step` on - the exponential moving average that
                   nnU-Net-style and MONAI bundles evaluate and ship; warmup=True uses min(decay, (1 + n) / (10 + n)) for the n-th update (the
                   timm / TF warm-up), without which the average stays biased towards the initial weights for about 1 / (1 - decay) steps
      mode="swa"   the running mean of the weights seen: torch.optim.swa_utils.AveragedModel / Lightning's StochasticWeightAveraging

    `avg` is a flat fp32 buffer laid out like the gradient arena; the first update copies the weights into it.  update() is two launches
    (miseg_weight_average) and nothing else, so it sits inside a captured step (GraphedTrainStep(weight_averager=)); with gradient clipping or the
    non-finite guard on it reads the optimiser's clip record on the device, and a skipped step is not averaged.  ALL trainable parameters are
    averaged whatever their "used" flags, like AveragedModel: a parameter without a gradient simply did not move.

        avg = WeightAverager(opt, "ema", decay=0.999); avg.prepare()
        ... opt.step(); avg.update() ...
        with avg.applied():            # the model computes on the averaged weights (conv packs and bf16 copies follow)
            validate(model)
        torch.save(avg.averaged_state_dict(model), path)

    Under data parallelism nothing is exchanged: the optimiser leaves the same weights on every rank, so every rank forms the same average
    from the same bytes."""

    def __init__(self, optimizer, mode="ema", decay=0.999, warmup=False, start_step=0, every=1):
        self._mode, self.decay, self.warmup, self.start_step, self.every = averaging_options(mode, decay, warmup, start_step, every)
        self.mode = mode
        self.opt = optimizer
        self.avg = self._rec = None
        self._swapped = False

    @property
    def arena(self):
        return self.opt.arena

    def prepare(self):
        """allocate `avg` and the zeroed record (miseg_weight_average_record: its counters run on) - ONCE: a captured hipGraph holds their
        addresses; call before capturing update()"""
        if self.avg is None:
            flat = self.arena.flat
            if flat.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("WeightAverager.prepare() must run before update() is captured (it allocates the average and its record)")
            self.avg = torch.empty_like(flat)          # never read before the first applying update writes it
            self._rec = torch.zeros(C.sizeof(L.WeightAverageRecord) // 4, dtype=torch.int32, device=flat.device)

    def update(self):
        """enqueue miseg_weight_average behind the optimiser step just issued: the tick and the streaming launch, nothing else (capturable)"""
        if self.avg is None:
            self.prepare()          # (raises under capture)
        if self._swapped:
            raise RuntimeError("WeightAverager.update() inside applied(): the parameters hold the average")
        opt = self.opt
        clip = opt._clip_buffers().data_ptr() if opt.clipping else None          # the guard's `skip` lives there: a skipped step is not averaged
        p = L.WeightAverage(C.sizeof(L.WeightAverage), self._mode, opt._table.data_ptr(), len(opt.arena.params), opt._blocks, self.avg.data_ptr(),
                            self._rec.data_ptr(), clip, self.decay, int(self.warmup), self.start_step, self.every)
        ops._call("miseg_weight_average", p)

    def stats(self):
        """the record read back once (one device-to-host copy): calls, n_averaged, and apply / first / coef of the last call"""
        if self._rec is None:
            return {"calls": 0, "n_averaged": 0, "apply": 0, "first": 0, "coef": 0.0}
        r = self._rec.cpu()
        return {"calls": int(r[3]) & 0xFFFFFFFF, "n_averaged": int(r[4]) & 0xFFFFFFFF, "apply": int(r[0]), "first": int(r[1]),
                "coef": float(r[2:3].view(torch.float32)[0])}

    @property
    def n_averaged(self):
        """how many updates the average holds (one device-to-host read)"""
        return self.stats()["n_averaged"]

    def swap(self):
        """exchange the parameters and the average in ONE launch (miseg_weight_swap); the launch bumps the arena's device-side parameter
        version, so the next refresh re-casts and re-packs every weight.  A second call restores every bit."""
        if self.avg is None:
            raise RuntimeError("WeightAverager.swap() before prepare(): there is no average")
        opt, a = self.opt, self.arena
        if [p.data_ptr() for p in a.params] != opt._ptrs:
            raise RuntimeError("a parameter was re-allocated after the optimiser was built (e.g. model.to(...)): rebuild the ArenaOptimizer")
        p = L.WeightSwap(C.sizeof(L.WeightSwap), opt._table.data_ptr(), len(a.params), opt._blocks, self.avg.data_ptr(), a.params_version_ptr())
        ops._call("miseg_weight_swap", p)
        a.epoch += 1
        self._swapped = not self._swapped

    def applied(self):
        """context manager: inside it the model's parameters ARE the averaged weights (swap(), then arena.refresh_weights(): bf16 copies and
        conv packs follow); on exit the training weights are back with their exact bits.  Raises while nothing has been averaged."""
        avg = self

        class _Applied:
            def __enter__(self_):
                if avg.n_averaged == 0:
                    raise RuntimeError("WeightAverager.applied(): nothing has been averaged yet (n_averaged == 0)")
                avg.swap()
                avg.arena.refresh_weights()
                return avg

            def __exit__(self_, *exc):
                avg.swap()
                avg.arena.refresh_weights()
                return False
        return _Applied()

    def _averaged_views(self):
        if self._swapped:          # inside applied() the average sits in the parameters (and the training weights in `avg`)
            return {id(p): p.detach() for p in self.arena.params}
        return {id(p): self.avg[o:o + p.numel()].view(p.shape) for p, o in zip(self.arena.params, self.arena._offs)}

    def averaged_state_dict(self, model):
        """model.state_dict() - its keys, shapes and order - with every trainable arena parameter replaced by (a copy of) its averaged value;
        frozen parameters and buffers pass through as they are.  A published-layout checkpoint loader takes it strictly."""
        if self.n_averaged == 0:
            raise RuntimeError("WeightAverager.averaged_state_dict(): nothing has been averaged yet (n_averaged == 0)")
        views = self._averaged_views()
        out = type(model.state_dict())()
        for k, v in model.state_dict(keep_vars=True).items():
            a = views.get(id(v))
            out[k] = a.clone() if a is not None else v.detach()
        return out

    def state_dict(self):
        st = self.stats()
        return {"mode": self.mode, "decay": self.decay, "warmup": self.warmup, "start_step": self.start_step, "every": self.every,
                "avg": None if self.avg is None else self.avg.clone(), "calls": st["calls"], "n_averaged": st["n_averaged"], "coef": st["coef"],
                "numel": self.arena.flat.numel()}

    def load_state_dict(self, sd):
        """continue the average of a checkpoint: `avg`, the counters and the options (which replace this object's); a mode or a size that does
        not match raises"""
        if sd["mode"] != self.mode:
            raise ValueError("weight averager state is {!r}, this one is {!r}".format(sd["mode"], self.mode))
        if sd["numel"] != self.arena.flat.numel() or (sd["avg"] is not None and sd["avg"].numel() != self.arena.flat.numel()):
            raise ValueError("weight averager state does not match this model (arena of {} elements, state of {})".format(self.arena.flat.numel(), sd["numel"]))
        self._mode, self.decay, self.warmup, self.start_step, self.every = averaging_options(sd["mode"], sd["decay"], sd["warmup"], sd["start_step"], sd["every"])
        self.prepare()
        if sd["avg"] is not None:
            self.avg.copy_(sd["avg"])
        rec = torch.zeros(self._rec.numel(), dtype=torch.int32)
        rec[2:3].view(torch.float32)[0] = float(sd.get("coef", 0.0))
        for i, key in ((3, "calls"), (4, "n_averaged")):
            v = int(sd[key])
            rec[i] = v - (1 << 32) if v >= (1 << 31) else v
        self._rec.copy_(rec)
