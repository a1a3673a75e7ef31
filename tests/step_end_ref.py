"""float64 references of the step-end reductions (tests/test_hip_step_end_forms.py), plain torch, on the very operands the kernels get, and
naive Python loops of the same operations that tests/test_step_end_cases_cpu.py holds them to."""
import torch


def tn_product(a, b):
    """C[m][n] = sum_k A[k][m] B[k][n] in float64"""
    return a.double().t() @ b.double()


def regroup_index(N, regroup):
    """dst[n]: column n = j * regroup + c of a product is stored at column c * (N / regroup) + j"""
    assert regroup > 0 and N % regroup == 0
    per = N // regroup
    dst = [0] * N
    for j in range(per):
        for c in range(regroup):
            dst[j * regroup + c] = c * per + j
    return torch.tensor(dst, dtype=torch.long)


def regrouped(prod, regroup):
    """the product with its columns where the regrouped store puts them (regroup 0: as it is)"""
    if not regroup:
        return prod
    out = torch.empty_like(prod)
    out[:, regroup_index(prod.shape[1], regroup).to(prod.device)] = prod
    return out


def partial_sum(partial):
    """sum over the splits of partial[s][m][n] in float64"""
    return partial.double().sum(0)


def colsum(x):
    """out[c] = sum_r x[r][c] in float64"""
    return x.double().sum(0)


def accumulate(before, term, keep=True):
    """what the slot holds afterwards: before + term (accumulate modes) or term alone, in float64"""
    return before.double() + term if keep else term


# ------------------------------------------------------------------------------------------------ the same, one element at a time
def naive_tn(a, b, regroup=0):
    K, M = len(a), len(a[0])
    N = len(b[0])
    out = [[0.0] * N for _ in range(M)]
    per = N // regroup if regroup else 0
    for m in range(M):
        for n in range(N):
            s = 0.0
            for k in range(K):
                s += float(a[k][m]) * float(b[k][n])
            out[m][(n % regroup) * per + n // regroup if regroup else n] = s
    return out


def naive_partial_sum(p):
    S, M, N = len(p), len(p[0]), len(p[0][0])
    out = [[0.0] * N for _ in range(M)]
    for m in range(M):
        for n in range(N):
            for s in range(S):
                out[m][n] += float(p[s][m][n])
    return out


def naive_colsum(x):
    out = [0.0] * len(x[0])
    for r in range(len(x)):
        for c in range(len(x[0])):
            out[c] += float(x[r][c])
    return out
