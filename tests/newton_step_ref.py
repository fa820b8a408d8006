"""One undamped Newton step of the chain kernels, on the host, in a chosen precision (TEST INFRASTRUCTURE).

In the whitened singular basis (oracle/sform.py): u = V v, H and w as sform.evaluate computes them, rho = c V^T H - ghat,
W = V^T diag(w) V, and the step is

    (c W c + alpha I) z = rho + alpha v / c ,   delta = c o z ,   v_next = v - delta .

A damped Newton iteration corrects its own solver -- an elimination that mishandles a row or a Gram tile summed from the wrong
place reaches the same fixed point in more iterations -- so a scan that converges says little about the solve.  ONE step says
all of it: tests/test_gpu_one_chain_builds.py compares the step every build of the one-chain kernel takes with this one."""
import numpy as np

LD = np.longdouble


def _cholesky_solve(B, rhs):
    """B z = rhs for a positive definite B, in the precision of its entries (numpy's solve is binary64)"""
    n = len(rhs)
    L = np.zeros_like(B)
    for j in range(n):
        d = B[j, j] - np.dot(L[j, :j], L[j, :j])
        assert d > 0, 'the Newton matrix is not positive definite'
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (B[j + 1:, j] - np.dot(L[j + 1:, :j], L[j, :j])) / L[j, j]
    y = np.zeros_like(rhs)
    for i in range(n):
        y[i] = (rhs[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
    z = np.zeros_like(rhs)
    for i in range(n - 1, -1, -1):
        z[i] = (y[i] - np.dot(L[i + 1:, i], z[i + 1:])) / L[i, i]
    return z


def newton_step(V, c, ghat, D, kind, alpha, v, dtype, drop=None):
    """(delta, delta^T W delta) of the undamped step from ``v``; ``kind``: 'normal' | 'plusminus'.

    ``dtype``: np.longdouble (Cholesky by hand), np.float64, or 'f32 stream': u, w, H, h = V^T H and W in binary32 from the
    binary32 roundings of V, v and D, the system and its solve in binary64 -- the arithmetic of Stream<float> in
    maxent_amd/csrc/mxe_kernel.hip.h.  ``drop`` = k: direction k treated as decoupled (row and column k of the matrix zero,
    alpha on its diagonal)."""
    stream = np.float32 if isinstance(dtype, str) else dtype
    solve = np.float64 if isinstance(dtype, str) else dtype
    if isinstance(dtype, str):
        assert dtype == 'f32 stream', dtype
    Vs, Ds, vs = V.astype(stream), D.astype(stream), v.astype(stream)
    u = np.dot(Vs, vs)
    if kind == 'normal':
        H = Ds * np.exp(u)
        w = H
    else:
        Hp, Hm = Ds * np.exp(u), Ds * np.exp(-u)
        H, w = Hp - Hm, Hp + Hm
    h = np.dot(Vs.T, H)
    W = np.dot(Vs.T * w[np.newaxis, :], Vs)
    assert u.dtype == stream and h.dtype == stream and W.dtype == stream
    c, ghat, v, W, alpha = c.astype(solve), ghat.astype(solve), v.astype(solve), W.astype(solve), solve(alpha)
    rho = c * h.astype(solve) - ghat
    rhs = rho + alpha * v / c
    B = c[:, np.newaxis] * W * c[np.newaxis, :] + alpha * np.eye(len(c), dtype=solve)
    if drop is not None:
        B[drop, :] = 0
        B[:, drop] = 0
        B[drop, drop] = alpha
    z = _cholesky_solve(B, rhs) if solve is LD else np.linalg.solve(B, rhs)
    delta = c * z
    assert delta.dtype == solve
    return delta, float(np.dot(delta, np.dot(W, delta)))


def rel_err(a, b):
    """|a - b| / |b|, in the wider of the two types"""
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
