"""numpy / longdouble restatement of ``evidence_scan_kernel`` and ``evidence_group_kernel`` (mxe_evidence.hip.h), with the
bounds their results are held to.  A helper of tests/test_gpu_model_scan.py and tests/test_model_scan_host.py: it needs no
GPU.

The bounds, derived like those of tests/resample_ref.py:

* an exponent is x_k = fl(logp_k + log_measure_k), the binary64 sum the kernel forms: at |logp| ~ 4000 the rounding of that
  sum (2^-41) is the conditioning of exp at the INPUT, not an error of the reduction, so the reference starts from the same
  rounded sums and does everything behind them in longdouble;
* a weight e_k / sum_j e_j, e_k = exp(x_k - m): the subtraction (eps |x_k - m|), exp and the division (a few eps), the
  sum of n terms in order (n eps): relative (|x_k - m| + n_alpha + 8) eps, plus the smallest normal number (an e_k below
  it may be flushed to zero);
* log Z = m + log S: what the terms' errors do to S, (sum_k e_k (|x_k - m| + 8) / S + n) eps, plus the roundings of log
  and of the last sum, 2 eps (|m| + |log S| + |log Z|);
* a weighted sum of n terms  sum w_k h_k:  (n + 8) eps sum |w_k| |h_k|  plus the weights' share  sum dw_k |h_k|  (and
  sum |w_k| dh_k where the h carry errors of their own);
* a functional value: (n_omega + 2) eps |F| |row| plus |F| d row;
* a weighted centred second moment (two passes): 4 (n + 8) eps sum u |d1| |d2| plus sum du |d1| |d2| plus what the errors e
  of the values and of their mean do to the centred products, sum u (e1 |d2| + |d1| e2).
"""
import numpy as np

EPS = np.finfo(float).eps
TINY = np.finfo(float).tiny
LD = np.longdouble


def _softmax(x, n_extra):
    """x: binary64 exponents (finite or -inf, not all -inf).  Returns m, weights (longdouble), their bounds, log sum, its
    bound -- the restatement of the kernel's maximum / exp / ordered sum / division"""
    x = np.asarray(x, dtype=float)
    m = float(np.max(x))
    d = x.astype(LD) - LD(m)
    e = np.exp(d)
    S = e.sum()
    w = e / S
    ad = np.where(np.isfinite(np.asarray(d, dtype=float)), np.abs(np.asarray(d, dtype=float)), 0.0)
    w_bound = (ad + n_extra + 8) * EPS * np.asarray(w, dtype=float) + TINY
    dS = (float((e * (ad + 8)).sum() / S) + len(x)) * EPS
    return m, w, w_bound, np.log(S), dS


def evidence_reduce_ref(H, group_offset, logp, log_quad, log_mix=None, log_prior=None, row_mode=0, pick=None, F=None):
    """H (n_scan, n_alpha, n_omega), logp (n_scan, n_alpha): section 1 of the issue, the good / usable rules included.
    Returns a dict of the values (longdouble where they are sums) and ``<name>_bound`` beside every one."""
    H = np.asarray(H, dtype=float)
    ns, na, nw = H.shape
    logp = np.asarray(logp, dtype=float).reshape(ns, na)
    log_quad = np.asarray(log_quad, dtype=float)
    log_mix = np.zeros(na) if log_mix is None else np.asarray(log_mix, dtype=float)
    log_prior = np.zeros(ns) if log_prior is None else np.asarray(log_prior, dtype=float)
    off = np.asarray(group_offset, dtype=int)
    ng = len(off) - 1
    F = np.zeros((0, nw)) if F is None else np.atleast_2d(np.asarray(F, dtype=float))
    nf = F.shape[0]
    Fl = F.astype(LD)
    out = dict(logZ=np.full(ns, -np.inf, dtype=LD), logZ_bound=np.zeros(ns), kmax=np.full(ns, -1), ngood=np.zeros(ns, dtype=int),
               usable=np.zeros(ns, dtype=bool), walpha=np.zeros((ns, na), dtype=LD), walpha_bound=np.zeros((ns, na)),
               row=np.full((ns, nw), np.nan, dtype=LD), row_bound=np.zeros((ns, nw)),
               fval=np.full((ns, nf), np.nan, dtype=LD), fval_bound=np.zeros((ns, nf)),
               wmodel=np.zeros(ns, dtype=LD), wmodel_bound=np.zeros(ns), used=np.zeros(ng, dtype=int),
               mean=np.full((ng, nw), np.nan, dtype=LD), mean_bound=np.zeros((ng, nw)),
               between=np.full((ng, nw), np.nan, dtype=LD), between_bound=np.zeros((ng, nw)),
               fmean=np.full((ng, nf), np.nan, dtype=LD), fmean_bound=np.zeros((ng, nf)),
               fcov=np.full((ng, nf, nf), np.nan, dtype=LD), fcov_bound=np.zeros((ng, nf, nf)))
    for s in range(ns):
        good = np.isfinite(logp[s])
        if row_mode == 0:
            good &= np.all(np.isfinite(H[s]), axis=1)
        k = np.nonzero(good)[0]
        out['ngood'][s] = len(k)
        if len(k) == 0:
            continue
        out['kmax'][s] = k[np.argmax(logp[s][k])]               # (argmax: the first index of the largest)
        m, _, _, logS, dS = _softmax(logp[s][k] + log_quad[k], na)
        logZ = LD(m) + logS
        dZ = dS + 2 * EPS * (abs(m) + abs(float(logS)) + abs(float(logZ)))
        _, w, wb, _, _ = _softmax(logp[s][k] + log_mix[k], na)
        out['walpha'][s][k], out['walpha_bound'][s][k] = w, wb
        if row_mode == 0:
            Hk = H[s][k].astype(LD)
            row = w @ Hk
            rb = (len(k) + 8) * EPS * np.asarray(np.abs(w) @ np.abs(Hk), dtype=float) + wb @ np.abs(H[s][k])
        else:
            ksel = out['kmax'][s] if row_mode == 1 else int(pick[s])
            if ksel < 0:
                continue
            row, rb = H[s][ksel].astype(LD), np.zeros(nw)
        if not np.all(np.isfinite(np.asarray(row, dtype=float))):
            continue
        out['usable'][s] = True
        out['logZ'][s], out['logZ_bound'][s] = logZ, dZ
        out['row'][s], out['row_bound'][s] = row, rb
        out['fval'][s] = Fl @ row
        out['fval_bound'][s] = (nw + 2) * EPS * np.asarray(np.abs(Fl) @ np.abs(row), dtype=float) + np.abs(F) @ rb
    for g in range(ng):
        r = np.arange(off[g], off[g + 1])
        r = r[out['usable'][r]] if len(r) else r
        n = len(r)
        out['used'][g] = n
        if n == 0:
            continue
        t = np.asarray(out['logZ'][r], dtype=float) + log_prior[r]           # (the kernel's binary64 sum)
        if not np.any(np.isfinite(t)):
            out['wmodel'][r] = np.nan                                            # (every usable scan is switched off)
            continue
        _, u, ub, _, _ = _softmax(t, n)
        # what the errors of log Z (and the rounding of log Z + log prior) do to the exponents: to a weight directly, and
        # through the sum
        dt = np.where(np.isfinite(t), out['logZ_bound'][r] + EPS * np.abs(np.where(np.isfinite(t), t, 0.0)), 0.0)
        uf = np.asarray(u, dtype=float)
        ub = ub + uf * (dt + float(np.sum(uf * dt)))
        out['wmodel'][r], out['wmodel_bound'][r] = u, ub
        rows, rbs = out['row'][r], out['row_bound'][r]
        mean = u @ rows
        mb = (n + 8) * EPS * np.asarray(np.abs(u) @ np.abs(rows), dtype=float) + ub @ np.asarray(np.abs(rows), dtype=float) + uf @ rbs
        d = rows - mean[None, :]
        ad = np.asarray(np.abs(d), dtype=float)
        e = rbs + mb[None, :]
        out['mean'][g], out['mean_bound'][g] = mean, mb
        out['between'][g] = u @ (d * d)
        out['between_bound'][g] = 4 * (n + 8) * EPS * (uf @ ad ** 2) + ub @ ad ** 2 + 2 * (uf @ (e * ad)) + uf @ e ** 2
        fv, fb = out['fval'][r], out['fval_bound'][r]
        fm = u @ fv
        fmb = (n + 8) * EPS * np.asarray(np.abs(u) @ np.abs(fv), dtype=float) + ub @ np.asarray(np.abs(fv), dtype=float) + uf @ fb
        df = fv - fm[None, :]
        adf = np.asarray(np.abs(df), dtype=float)
        ef = fb + fmb[None, :]
        out['fmean'][g], out['fmean_bound'][g] = fm, fmb
        out['fcov'][g] = (df * u[:, None]).T @ df
        wa = adf * uf[:, None]
        out['fcov_bound'][g] = 4 * (n + 8) * EPS * (wa.T @ adf) + (adf * ub[:, None]).T @ adf + \
            (ef * uf[:, None]).T @ adf + wa.T @ ef + (ef * uf[:, None]).T @ ef
    return out


def scan_problem(widths=(0.5, 1.0, 2.0, 4.0, 8.0)):
    """The problem of the end-to-end test and of the oracle check: beta = 10, 40 tau points, a hyperbolic mesh of 60 points
    on [-8, 8], A = 0.6 N(1, 0.5^2) + 0.4 N(-1.5, 0.8^2) (trapezoid-normalised), G = K_delta A + 1e-3 noise (seed 7).
    Returns tau, omega, A, G and the models as D arrays (density x delta, sum 1): flat, Gaussians at 0 of the ``widths``,
    the true spectrum."""
    from oracle import ref_numpy as R
    tau = np.linspace(0.0, 10.0, 40)
    omega = R.hyperbolic_omega_mesh(-8.0, 8.0, 60)
    delta = R.omega_delta(omega)

    def shape(mu, sig):
        # (the Gaussian SHAPES with the heights 0.6 and 0.4, normalised together below: this is the spectrum the oracle
        #  figures of DESIGN.md 4v were made with)
        return np.exp(-0.5 * ((omega - mu) / sig) ** 2)
    A = 0.6 * shape(1.0, 0.5) + 0.4 * shape(-1.5, 0.8)
    A = A / np.trapezoid(A, omega)
    _, K_delta = R.tau_kernel(tau, omega, 10.0)
    G = np.dot(K_delta, A) + 1e-3 * np.random.RandomState(7).randn(len(tau))
    models = [R.flat_default_model(omega)]
    for w in widths:
        D = np.exp(-0.5 * (omega / w) ** 2) * delta
        models.append(D / D.sum())
    models.append(A * delta / np.sum(A * delta))
    return tau, omega, A, G, models


def brute_force(H, logp, log_quad, log_mix, log_prior):
    """one group, row_mode 0, every alpha good, plain binary64 without any shift: for tiny inputs of moderate size"""
    H, logp = np.asarray(H, dtype=float), np.asarray(logp, dtype=float)
    ns = len(logp)
    Z, rows, wal = np.empty(ns), [], []
    for s in range(ns):
        Z[s] = sum(np.exp(logp[s][k]) * np.exp(log_quad[k]) for k in range(len(log_quad)))
        p = np.array([np.exp(logp[s][k]) * np.exp(log_mix[k]) for k in range(len(log_mix))])
        wal.append(p / p.sum())
        rows.append(sum(wal[-1][k] * H[s][k] for k in range(len(p))))
    rows = np.array(rows)
    pw = Z * np.exp(log_prior)
    u = pw / pw.sum()
    mean = sum(u[s] * rows[s] for s in range(ns))
    between = sum(u[s] * (rows[s] - mean) ** 2 for s in range(ns))
    return dict(logZ=np.log(Z), walpha=np.array(wal), row=rows, wmodel=u, mean=mean, between=between)
