"""numpy restatement of gradient accumulation over micro-batches (include/miseg_hip.h: miseg_grad_fold; training/optim.py::GradAccumulator).

    op_codes(used, seen, closes)     one code per parameter: u | a << 1 | F << 2
    fold(acc, g, ops, scale)         what one miseg_grad_fold launch does to the two buffers, parameter by parameter
    window(grads, used, k)           a whole window: the mean gradients the arena holds after the closing fold and the window's union

    op      effect                                   reads            writes
    0 2 4   nothing                                  -                -
    1       acc = g                                  g                acc
    3       acc = fl(acc + g)                        g, acc           acc
    5       g = fl(g * scale)                        g                g
    6       g = fl(acc * scale)                      acc              g
    7       g = fl(fl(acc + g) * scale)              g, acc           g

`g` is the gradient arena.  Every operation is rounded on its own in `dtype`: float32 is what the kernel computes, float64 (the CPU tests)
holds the rule itself against torch autograd."""
import numpy as np

U, A, F = 1, 2, 4


def scale_of(k, dtype=np.float32):
    """fl(1 / k)"""
    return dtype(1.0) / dtype(k)


def op_codes(used, seen, closes):
    return [(U if u else 0) | (A if a else 0) | (F if closes else 0) for u, a in zip(used, seen)]


def reads(op):
    """(the arena slot is read, the accumulator slot is read)"""
    u, a, f = bool(op & U), bool(op & A), bool(op & F)
    return u, a and (u or f)


def writes(op):
    """(the arena slot is written, the accumulator slot is written)"""
    u, a, f = bool(op & U), bool(op & A), bool(op & F)
    return f and (u or a), u and not f


def fold(acc, g, ops, scale, dtype=np.float32):
    """acc, g: one array (or None: a slot nobody may read) per parameter.  Returns the new (acc, g) lists; an entry the table leaves alone
    is the very object that came in."""
    s = dtype(scale)
    acc, g = list(acc), list(g)
    with np.errstate(over="ignore", invalid="ignore"):
        for i, op in enumerate(ops):
            rg, ra = reads(op)
            if not (rg or ra):
                continue
            if rg and ra:
                v = (np.asarray(acc[i], dtype=dtype) + np.asarray(g[i], dtype=dtype)).astype(dtype)
            else:
                v = np.array(g[i] if rg else acc[i], dtype=dtype)
            if op & F:
                g[i] = (v * s).astype(dtype)
            else:
                acc[i] = v
    return acc, g


def window(grads, used, k, dtype=np.float32):
    """grads[j][i] / used[j][i]: gradient and "has one" of parameter i in micro-batch j of ONE window (len(grads) <= k: a short window still
    divides by k).  Returns (mean, union): mean[i] is None for a parameter absent from the whole window."""
    n = len(used[0])
    acc, seen = [None] * n, [False] * n
    g = None
    for j in range(len(grads)):
        ops = op_codes(used[j], seen, j == len(grads) - 1)
        g = [grads[j][i] if used[j][i] else None for i in range(n)]
        acc, g = fold(acc, g, ops, scale_of(k, dtype), dtype)
        seen = [a or bool(u) for u, a in zip(used[j], seen)]
    return [g[i] if seen[i] else None for i in range(n)], seen
