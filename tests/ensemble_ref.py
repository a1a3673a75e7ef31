"""TEST INFRASTRUCTURE ONLY: independent statements of the ensemble fold that the CPU and the GPU tests share - a
hand-written float64 computation in numpy (no torch op of the product's restatement), the explicit flip -> sliding_window_inference ->
flip back -> sequential sum loop the EnsembleInferer is held to, and the gap rule under which a mean_prob class map is compared."""
import numpy as np
import torch

KINDS = ("mean_logits", "mean_prob", "vote")
FLIPS = [tuple(bool((m >> a) & 1) for a in range(3)) for m in range(8)]


def term64(src, flip, kind):
    """float64 numpy [B, C, D, H, W]: what a member contributes, un-flipped, written out with plain loops over the channels"""
    x = np.asarray(src, dtype=np.float64)
    for a in range(3):
        if flip[a]:
            x = x[(slice(None),) * (2 + a) + (slice(None, None, -1),)]
    B, C = x.shape[:2]
    if kind == "mean_logits":
        return x.copy()
    if kind == "mean_prob":
        mx = np.full(x[:, 0].shape, -np.inf)
        for c in range(C):
            mx = np.maximum(mx, x[:, c])
        e = np.stack([np.exp(x[:, c] - mx) for c in range(C)], 1)
        return e / e.sum(1, keepdims=True)
    arg = np.zeros(x[:, 0].shape, dtype=np.int64)                 # vote: the strict `>` scan from channel 0
    mx = x[:, 0].copy()
    for c in range(1, C):
        with np.errstate(invalid="ignore"):
            up = x[:, c] > mx
        mx = np.where(up, x[:, c], mx)
        arg = np.where(up, c, arg)
    return np.stack([(arg == c).astype(np.float64) for c in range(C)], 1)


def fold64(members, kind, scale=None):
    """members: list of (src, flip, weight per class or scalar); returns (float64 result, float64 sum of |w t| s): acc = sum w t, times scale"""
    acc = mag = None
    for src, flip, weight in members:
        t = term64(src, flip, kind)
        w = np.ones(t.shape[1]) if kind == "vote" else np.broadcast_to(np.asarray(weight, dtype=np.float32).astype(np.float64), (t.shape[1],))
        term = t * w.reshape(1, -1, 1, 1, 1)
        acc = term if acc is None else acc + term
        mag = np.abs(term) if mag is None else mag + np.abs(term)
    if scale is not None:
        s = np.broadcast_to(np.asarray(scale, dtype=np.float32).astype(np.float64), (acc.shape[1],)).reshape(1, -1, 1, 1, 1)
        acc, mag = acc * s, mag * s
    return acc, mag


def loop_reference(inputs, predictors, flips, run, mode="mean_logits", weights=None):
    """the explicit loop an EnsembleInferer is held to bit for bit (mean_logits / vote): predictor-major, flip-minor; flip the input, run
    the inferer (`run(x, predictor)`), flip the logits back, add fl(w * t) in order, multiply by fl(1 / sum w) at the end (not for vote)"""
    from mi_seg_amd.hip import ops
    acc, total = None, 0.0
    for i, p in enumerate(predictors):
        w = 1.0 if weights is None else float(torch.tensor(weights[i], dtype=torch.float32))
        for f in flips:
            dims = [2 + a for a in range(3) if f[a]]
            logits = run(torch.flip(inputs, dims) if dims else inputs, p)
            logits = torch.flip(logits, dims) if dims else logits
            if mode == "vote":
                arg = torch.stack([ops.first_max_argmax(v) for v in logits])
                term = torch.stack([(arg == c) for c in range(logits.shape[1])], 1).float()
            else:
                term = logits * torch.tensor(w, dtype=torch.float32)
            acc = term.clone() if acc is None else acc + term
            total += w
    if mode != "vote":
        acc = acc * torch.tensor(1.0 / total, dtype=torch.float32).to(acc.device)
    return acc


def class_map_agrees(got, truth64, gap=1e-5, cap=0.01):
    """got [B, C, ...] (any float tensor), truth64 float64 of the same shape: the first-maximum argmax of `got` must equal the one of
    `truth64` at every voxel whose float64 top-two gap is >= gap; at most `cap` of the voxels may be left out.  Returns the share left out."""
    from mi_seg_amd.hip import ops
    t = torch.as_tensor(truth64)
    top = t.topk(2, dim=1).values
    decided = (top[:, 0] - top[:, 1]) >= gap
    left_out = 1.0 - float(decided.double().mean())
    a = torch.stack([ops.first_max_argmax(v) for v in got.cpu()])
    b = torch.stack([ops.first_max_argmax(v) for v in t])
    assert bool((a == b)[decided].all()), int(((a != b) & decided).sum())
    assert left_out <= cap, left_out
    return left_out
