"""Plain helpers of the cross-validation tests: the score of ``mxe_cv_score`` in extended precision with the magnitude
sums its gates are made of, and the fold tables written from their definition."""

import numpy as np

EPS = float(np.finfo(float).eps)
#: the project's gate on a sum taken in another order: 64 eps times the sum of the magnitudes of its terms
SUM_GATE = 64.0 * EPS


def score(H, K, Gval, w, T=None, rank=None, dtype=np.longdouble):
    """one group: ``H`` (rows, n_omega), ``K`` (n_data, n_omega), ``Gval``, ``w`` (n_data,), ``T`` (n_data, n_data) or
    None (the identity), ``rank`` or None (n_data).  Returns (z (rows, n_data), score (rows,), terms (rows, n_data)):
    z_k = sqrt(w_k) (sum_j T_kj sum_i K_ji H_i - Gval_k) for k < rank and 0 behind it, score = sum_k z_k^2,
    terms_k = sqrt(w_k) (sum_j |T_kj| sum_i |K_ji H_i| + |Gval_k|); a row of H that is not finite is NaN in all three."""
    H = np.atleast_2d(np.asarray(H, dtype=float)).astype(dtype)
    K = np.asarray(K, dtype=float).astype(dtype)
    n = K.shape[0]
    Gv = np.asarray(Gval, dtype=float).astype(dtype)
    sw = np.sqrt(np.asarray(w, dtype=float).astype(dtype))
    Tm = np.eye(n, dtype=dtype) if T is None else np.asarray(T, dtype=float).astype(dtype)
    r = n if rank is None else int(rank)
    rows = H.shape[0]
    z, terms = np.zeros((rows, n), dtype=dtype), np.zeros((rows, n), dtype=dtype)
    sc = np.zeros(rows, dtype=dtype)
    for a in range(rows):
        if not np.all(np.isfinite(H[a])):
            z[a], terms[a], sc[a] = np.nan, np.nan, np.nan
            continue
        m = np.array([np.sum(K[j] * H[a]) for j in range(n)], dtype=dtype)
        ma = np.array([np.sum(np.abs(K[j] * H[a])) for j in range(n)], dtype=dtype)
        for k in range(r):
            z[a, k] = sw[k] * (np.sum(Tm[k] * m) - Gv[k])
            terms[a, k] = sw[k] * (np.sum(np.abs(Tm[k]) * ma) + np.abs(Gv[k]))
        sc[a] = np.sum(z[a] * z[a])
    return z, sc, terms


def gates(z, sc, terms):
    """the derived bounds on the device's binary64 numbers: |dz_k| <= 64 eps terms_k (another summation order, with room
    for the rounding of sqrt, difference and product), |dscore| <= 2 sum_k |z_k| 64 eps terms_k + 64 eps score (the first
    order of the z errors, and the sum of squares in another order)"""
    gz = SUM_GATE * np.asarray(terms, dtype=float)
    gs = 2.0 * np.sum(np.abs(np.asarray(z, dtype=float)) * gz, axis=-1) + SUM_GATE * np.asarray(sc, dtype=float)
    return gz, gs


def fold_ranges(n_bins, n_folds):
    """contiguous folds whose sizes differ by at most one, the longer ones first: [(start, stop), ...]"""
    base, extra = divmod(n_bins, n_folds)
    out, pos = [], 0
    for f in range(n_folds):
        size = base + (1 if f < extra else 0)
        out.append((pos, pos + size))
        pos += size
    return out


def fold_table(n_bins, n_folds):
    """the table of 1 + 2 K rows from its definition: ones; per fold 0 inside / 1 outside; per fold 1 inside / 0 outside"""
    rows = [[1] * n_bins]
    rng = fold_ranges(n_bins, n_folds)
    for a, b in rng:
        rows.append([0 if a <= i < b else 1 for i in range(n_bins)])
    for a, b in rng:
        rows.append([1 if a <= i < b else 0 for i in range(n_bins)])
    return np.array(rows, dtype=np.int32)


def cov_longdouble(bins):
    """the covariance of the mean of ``bins`` (n_bins, n_data), formed in extended precision"""
    b = np.asarray(bins, dtype=np.longdouble)
    nb = b.shape[0]
    X = (b - b.mean(axis=0)) / np.sqrt(np.longdouble(nb) * (nb - 1))
    return np.asarray(X.T @ X, dtype=float)


def pick_rules(alpha, score, score_err):
    """the argmin rules, written out: (index of the minimum over the finite scores, of equal ones the larger alpha; the
    largest alpha whose score is <= the minimum + score_err there); (-1, -1) without a finite score"""
    best = one = -1
    for i in range(len(score)):
        if np.isfinite(score[i]) and (best < 0 or score[i] < score[best] or (score[i] == score[best] and alpha[i] > alpha[best])):
            best = i
    if best < 0:
        return -1, -1
    for i in range(len(score)):
        if np.isfinite(score[i]) and score[i] <= score[best] + score_err[best] and (one < 0 or alpha[i] > alpha[one]):
            one = i
    return best, one
