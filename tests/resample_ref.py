"""numpy / longdouble restatements of ``bins_resample_kernel`` and ``resample_reduce_kernel`` (mxe_resample.hip.h), with
the componentwise bounds their sums are held to.  A helper of tests/test_gpu_resample.py: it needs no GPU."""
import numpy as np

EPS = np.finfo(float).eps
LD = np.longdouble


def bins_resample_ref(bins, counts, T, rank, mean=None):
    """one set: bins (n_bins, n_data), counts (n_res, n_bins), T (n_data, n_data), rank.  ``mean``: the binary64 mean the
    bins are centred with (default: the longdouble mean, rounded).  Returns mean, dev, Tmean (longdouble, rows >= rank
    zero) and the componentwise bounds of dev and of T mean:
        (n_bins + n_data + 8) eps (|counts| / N_r |X_c| |T|^T),     4 n_data eps |T| |mean|"""
    b = np.asarray(bins, dtype=LD)
    n_bins, n_data = b.shape
    if mean is None:
        mean = np.asarray(b.sum(axis=0) / LD(n_bins), dtype=float)
    m = np.asarray(mean, dtype=LD)
    Xc = b - m[None, :]
    c = np.asarray(counts, dtype=LD)
    W = c / c.sum(axis=1)[:, None]
    Tk = np.array(T, dtype=LD)
    Tk[rank:] = 0
    D = W @ Xc
    dev = D @ Tk.T
    Tmean = Tk @ m
    bound_dev = (n_bins + n_data + 8) * EPS * np.asarray((np.abs(W) @ np.abs(Xc)) @ np.abs(Tk).T, dtype=float)
    bound_Tm = 4 * n_data * EPS * np.asarray(np.abs(Tk) @ np.abs(m), dtype=float)
    return dict(mean=np.asarray(mean, dtype=float), dev=dev, Tmean=Tmean, bound_dev=bound_dev, bound_Tm=bound_Tm)


def reduce_ref(H, group_offset, scale, F=None):
    """groups of rows of H (rows, n_omega): per group, over its finite rows, mean, scale * sum (H_r - mean)^2, the same
    of the functional values F H_row; fewer than two finite rows: NaN variances.  Everything in longdouble.  Also the
    bounds  n eps mean|H|  of the mean and  4 n eps (var + scale sum |H_r - mean| eps |mean|)  of the variance
    (the two-pass bound).  The functional values: each is a sum of n_omega products, error e = (n_omega + 2) eps |F| |H_row|;
    their mean inherits n eps mean|f| + mean(e); their covariance the two-pass bound 4 n eps scale sum |d1| |d2| plus what
    the errors of the values do to the centred products, 2 scale sum (e1 |d2| + |d1| e2) (the factor 2: each value also
    moves its mean)."""
    H = np.asarray(H, dtype=float)
    rows, nw = H.shape
    ng = len(group_offset) - 1
    F = np.zeros((0, nw)) if F is None else np.atleast_2d(np.asarray(F, dtype=float))
    nf = F.shape[0]
    Hl, Fl = H.astype(LD), F.astype(LD)
    fval = Hl @ Fl.T
    fval_bound = (nw + 2) * EPS * np.asarray(np.abs(Hl) @ np.abs(Fl).T, dtype=float)
    out = dict(fval=fval, fval_bound=fval_bound, used=np.zeros(ng, dtype=int),
               mean=np.full((ng, nw), np.nan, dtype=LD), var=np.full((ng, nw), np.nan, dtype=LD),
               fmean=np.full((ng, nf), np.nan, dtype=LD), fcov=np.full((ng, nf, nf), np.nan, dtype=LD),
               mean_bound=np.full((ng, nw), np.nan), var_bound=np.full((ng, nw), np.nan),
               fmean_bound=np.full((ng, nf), np.nan), fcov_bound=np.full((ng, nf, nf), np.nan))
    for g in range(ng):
        r = np.arange(group_offset[g], group_offset[g + 1])
        r = r[np.all(np.isfinite(H[r]), axis=1)] if len(r) else r
        n = len(r)
        out['used'][g] = n
        if n == 0:
            continue
        mean = Hl[r].sum(axis=0) / LD(n)
        out['mean'][g] = mean
        out['mean_bound'][g] = n * EPS * np.asarray(np.abs(Hl[r]).sum(axis=0) / n, dtype=float)
        fm = fval[r].sum(axis=0) / LD(n)
        out['fmean'][g] = fm
        fb = fval_bound[r]
        out['fmean_bound'][g] = n * EPS * np.asarray(np.abs(fval[r]).sum(axis=0) / n, dtype=float) + fb.sum(axis=0) / n
        if n >= 2:
            d = Hl[r] - mean[None, :]
            var = LD(scale[g]) * (d * d).sum(axis=0)
            out['var'][g] = var
            out['var_bound'][g] = 4 * n * EPS * np.asarray(
                var + abs(LD(scale[g])) * np.abs(d).sum(axis=0) * EPS * np.abs(mean), dtype=float)
            df = fval[r] - fm[None, :]
            out['fcov'][g] = LD(scale[g]) * (df.T @ df)
            ad = np.asarray(np.abs(df), dtype=float)
            out['fcov_bound'][g] = abs(float(scale[g])) * (4 * n * EPS * (ad.T @ ad) + 2 * (fb.T @ ad + ad.T @ fb))
    return out
