"""``TauMaxEnt``: MaxEnt with the imaginary-time kernel (user facade).

Keeps the reference's surface (reference python/tau_maxent.py:37-356): owns a
:class:`MaxEntLoop` and shadows its attributes (``tm.omega = ...``,
``tm.alpha_mesh = ...``), default 100-point hyperbolic omega mesh on
[-10, 10] with a flat default model, setters for G(tau) from arrays or text
files, scalar / per-tau errors and full covariance matrices (the problem is
rotated into the covariance eigenbasis).  ``set_G_iw_data`` takes G(i omega_n)
as arrays instead: the kernel becomes an :class:`IOmegaKernel` and the data
its stacked real form ``[Re G ; Im G]``.  ``set_chi_tau_data`` / ``set_chi_iw_data``
take bosonic data (susceptibilities) the same way, with a
:class:`BosonicTauKernel` / :class:`BosonicIOmegaKernel`, ``set_G_l_data``
takes Legendre coefficients with a :class:`LegendreKernel`.  ``set_G_tau`` /
``set_G_iw`` need TRIQS Green-function objects and are not provided.
"""

from copy import deepcopy

import numpy as np

from . import default_models, kernels, maxent_loop as loop_module, omega_meshes


class TauMaxEnt(object):
    maxent_loop = None      # needed by the attribute shadowing below

    def __init__(self, cov_threshold=1.e-14, svd_backend='host', **kwargs):
        self.maxent_loop = loop_module.MaxEntLoop(**kwargs)
        omega = omega_meshes.HyperbolicOmegaMesh()
        self.D = default_models.FlatDefaultModel(omega)
        # svd_backend='device': kernel fill + SVD on the GPU (mxe_kernel_svd)
        self.K = kernels.TauKernel([0, 1], omega, svd_backend=svd_backend)      # placeholder tau grid
        self.omega = omega
        self.cov_threshold = cov_threshold

    # attributes of the loop can be used as if they were ours
    def __getattr__(self, name):
        return getattr(object.__getattribute__(self, 'maxent_loop'), name)

    def __setattr__(self, name, value):
        if hasattr(self.maxent_loop, name):
            setattr(self.maxent_loop, name, value)
        else:
            object.__setattr__(self, name, value)

    def set_G_tau(self, *args, **kwargs):
        raise NotImplementedError('set_G_tau needs TRIQS Green functions; '
                                  'use set_G_tau_data or set_G_tau_file')

    set_G_iw = set_G_tau

    # ---- data, errors and the rotation of the data space -------------------
    # State: ``G`` (the data as the solver sees them, possibly rotated), ``cost_function._G_orig``
    # (as supplied) and the absolute rotation ``K._T`` of the kernel (None: unrotated).  Two moves:
    # ``_adopt_data`` -- new data arrive in the original basis and are brought into the current
    # rotation; ``_rotate_to`` -- data and kernel go from the current rotation to another one.
    # (reference tau_maxent.py:181-325)

    def _move_data(self, T_to, T_from):
        """data from rotation ``T_from`` to rotation ``T_to`` (None = unrotated): back, then forth"""
        G = self.G
        if T_from is not None:
            G = np.dot(T_from.conjugate().transpose(), G)
        if T_to is not None:
            G = np.dot(T_to, G)
        if G is not self.G:
            self.G = G

    def _announce_kernel(self, T):
        self.K.transform(T)          # sets K._T
        self.K = self.K              # chi2 and H_of_v hear about the changed kernel

    def _adopt_data(self, keep_rotation=True):
        T = self._T if keep_rotation else None
        self.cost_function._G_orig = deepcopy(self.G)
        self._move_data(T, None)
        self._announce_kernel(T)

    def _rotate_to(self, T):
        self._move_data(T, self._T)
        self._announce_kernel(T)

    def _transform(self, T_, G_original_basis=False):
        """the reference's name for the two moves (tau_maxent.py:303-325)"""
        if G_original_basis:
            self.cost_function._G_orig = deepcopy(self.G)
            self._move_data(T_, None)
            self._announce_kernel(T_)
        else:
            self._rotate_to(T_)

    def _inner_kernel(self):
        """the kernel of the problem, looked up inside a PreblurKernel"""
        K = self.K
        return getattr(K, 'kernel', K)

    def _stacked_kernel(self):
        """the kernel whose rows are ``[Re K ; Im K]`` (also inside a PreblurKernel), else None"""
        K = self._inner_kernel()
        return K if getattr(K, 'stacked', False) else None

    def _use_kernel(self, cls, grid, assign_grid=True, **params):
        """A kernel of class ``cls`` on ``grid`` with the constructor arguments ``params`` (same omega mesh and SVD
        backend).  The kernel that is there -- also inside a PreblurKernel -- stays if its ``setter_kind`` is the wanted
        ``kind`` and it is equal in ``cls.kind_params``: it is refilled, once, only when the grid changes or a ``beta``
        that enters its matrix (``beta_in_matrix``; other kernels just remember theirs).  ``assign_grid=False`` leaves the grid of a
        kernel that stays to the caller.  Arguments are validated before anything is changed."""
        grid = cls._checked_args(grid, **params)
        K = self._inner_kernel()
        keep = getattr(K, 'setter_kind', 'tau') == cls.kind
        for p in cls.kind_params:
            keep = keep and getattr(K, p) == params[p]
        if not keep:
            self.K = cls(np.array(grid, dtype=float), self.omega, svd_backend=self.K.svd_backend, **params)
            return
        refill = False
        if 'beta' in params and (not cls.beta_in_matrix or K.beta != params['beta']):
            K.beta = params['beta']
            refill = cls.beta_in_matrix
        if assign_grid and self.set_tau(grid):    # (a new grid refills)
            return
        if refill:
            self.K.parameter_change()
            self.K = self.K

    def set_G_tau_data(self, tau, G_tau):
        """G(tau) from arrays (reference tau_maxent.py:181-196)"""
        if len(tau) != len(G_tau):
            raise AssertionError("tau and G_tau don't have the same dimension")
        self._use_kernel(kernels.TauKernel, tau)
        self.G = G_tau
        self._adopt_data()

    def set_G_iw_data(self, iomega, G_iw, beta=None):
        """G(i omega_n) from arrays: ``iomega`` the real Matsubara frequencies omega_n, ``G_iw`` the complex data
        there; ``beta`` defaults to 2 pi / (omega_1 - omega_0).  The kernel becomes an :class:`IOmegaKernel` (the
        reference's kernel, kernels.py:283-346, in its stacked real form) and ``G`` the stacked real vector
        ``[Re G ; Im G]`` of 2 n_iw values, which ``scale_alpha='Ndata'`` counts; results give G, G_orig and G_rec
        back as complex arrays of n_iw values.  (The reference's ``set_G_iw`` takes a TRIQS Green function and
        Fourier-transforms it to tau first, tau_maxent.py:148-179.)"""
        iomega = np.asarray(iomega, dtype=float)
        G_iw = np.asarray(G_iw)
        if iomega.ndim != 1 or G_iw.shape != iomega.shape:
            raise AssertionError("iomega and G_iw don't have the same dimension")
        self._use_kernel(kernels.IOmegaKernel, iomega, beta=beta)
        self.G = self.K.unfold(G_iw)
        self._adopt_data()

    def set_chi_tau_data(self, tau, chi, beta=None, symmetric=False):
        """Bosonic chi(tau) from arrays, continued to A(omega) = Im chi(omega) / (pi omega): the kernel becomes a
        :class:`BosonicTauKernel` (``beta`` defaults to ``tau[-1]``).  ``symmetric``: A(omega) = A(-omega), the omega
        mesh holds omega >= 0 only.  Not in the reference."""
        tau = np.asarray(tau, dtype=float)
        chi = np.asarray(chi)
        if tau.ndim != 1 or chi.shape != tau.shape:
            raise AssertionError("tau and chi don't have the same dimension")
        if np.iscomplexobj(chi):
            raise AssertionError('chi(tau) must be real')
        self._use_kernel(kernels.BosonicTauKernel, tau, beta=beta, symmetric=bool(symmetric))
        self.G = np.asarray(chi, dtype=float)
        self._adopt_data()

    def set_chi_iw_data(self, inu, chi_iw, beta=None, symmetric=False):
        """Bosonic chi(i nu_n) from arrays: ``inu`` the real Matsubara frequencies nu_n = 2 pi n / beta (nu_0 = 0
        included if it is there), ``chi_iw`` the data; ``beta`` defaults to 2 pi / (nu_1 - nu_0).  The kernel becomes
        a :class:`BosonicIOmegaKernel` and ``G`` the stacked real vector ``[Re chi ; Im chi]`` of 2 n values, which
        ``scale_alpha='Ndata'`` counts; results give G, G_orig and G_rec back complex.  ``symmetric``:
        A(omega) = A(-omega) on a mesh omega >= 0, chi(i nu_n) is real: ``G`` holds the n values Re chi(i nu_n) (an
        imaginary part of the data is dropped), and the results are real."""
        inu = np.asarray(inu, dtype=float)
        chi_iw = np.asarray(chi_iw)
        if inu.ndim != 1 or chi_iw.shape != inu.shape:
            raise AssertionError("inu and chi_iw don't have the same dimension")
        self._use_kernel(kernels.BosonicIOmegaKernel, inu, beta=beta, symmetric=bool(symmetric))
        self.G = np.asarray(self._inner_kernel().unfold(chi_iw), dtype=float)
        self._adopt_data()

    @staticmethod
    def _legendre_orders(l, n):
        """the orders of ``n`` Legendre coefficients: ``l``, or 0..n-1"""
        l = np.arange(n) if l is None else np.asarray(l)
        if l.ndim != 1 or len(l) != n:
            raise AssertionError("l and G_l don't have the same dimension")
        return l

    def set_G_l_data(self, G_l, beta, l=None):
        """G as Legendre coefficients G_l in TRIQS's ``GfLegendre`` normalisation, G(tau) = sum_l sqrt(2l+1)/beta
        P_l(2 tau/beta - 1) G_l (what continuous-time Monte Carlo solvers measure): the kernel becomes a
        :class:`LegendreKernel` on the orders ``l`` (default 0..n-1; any distinct non-negative integers, such as the
        even orders only).  ``beta`` is required; the coefficients are real.  Not in the reference."""
        G_l = np.asarray(G_l)
        if G_l.ndim != 1:
            raise AssertionError('G_l must be one-dimensional')
        if np.iscomplexobj(G_l):
            raise AssertionError('G_l must be real')
        self._use_kernel(kernels.LegendreKernel, self._legendre_orders(l, len(G_l)), beta=beta)
        self.G = np.asarray(G_l, dtype=float)
        self._adopt_data()

    def set_G_tau_file(self, filename, tau_col=0, G_col=1, err_col=None):
        """G(tau), optionally with its error bar, from the columns of a text file
        (reference tau_maxent.py:198-225); a file that brings errors ends any rotation"""
        table = np.loadtxt(filename)
        self._use_kernel(kernels.TauKernel, table[:, tau_col])
        self.G = table[:, G_col]
        if err_col is not None:
            self.err = table[:, err_col]
        self._adopt_data(keep_rotation=err_col is None)

    def set_error(self, error):
        """one standard deviation for all tau or one per tau; ends a covariance rotation
        (reference tau_maxent.py:227-251).  Matsubara data: a scalar, one value per frequency (for the real and the
        imaginary part alike) or one per stacked real value (2 n_iw: the real parts', then the imaginary parts')"""
        if not np.all(np.isreal(error)):
            raise Exception('complex error supplied, only real accepted')
        sigma = np.real(error) * np.ones(np.shape(self.G)) if np.ndim(error) == 0 \
            else np.asarray(np.real(error), dtype=float)
        K = self._stacked_kernel()
        if K is not None and sigma.shape == (K.n_iw,) and np.shape(self.G) == (2 * K.n_iw,):
            sigma = np.concatenate([sigma, sigma])
        if sigma.shape != np.shape(self.G):
            raise Exception('Supply scalar error or with length of G_tau.')
        self.err = sigma
        self._rotate_to(None)

    def set_cov(self, cov):
        """Full covariance matrix of the data (reference tau_maxent.py:253-288): the problem is rotated
        into the eigenbasis of ``cov`` (eigenvalues below ``cov_threshold`` dropped), where the errors are
        the square roots of the eigenvalues.  As in the reference, the data are first reset to the supplied
        ones and then moved by the hop from the PREVIOUS rotation to the new one -- after an earlier
        ``set_cov`` that is not the new rotation alone; the element-wise drivers rely on reproducing it."""
        given = cov
        known = self.__dict__.get('_cov_eig')
        if known is not None and known[0] is given and known[1] == self.cov_threshold and \
                np.array_equal(known[2], np.asarray(given)):        # (the same object with the same CONTENT: an in-place edit recomputes)
            # the same matrix again (one covariance for all matrix elements of an element-wise job): its
            # eigenbasis, and the SAME rotation object -- the kernel then has nothing to do, and the batch
            # solver sees one data set instead of one per element
            cov, sigma, T = known[2:]
        else:
            cov = np.array(cov)                   # (a private copy: the cache compares against it)
            if np.max(np.abs(cov - cov.transpose())) >= 1.e-10:
                raise AssertionError('Supplied covariance matrix is not symmetric.')
            var, vec = np.linalg.eigh(cov)
            if var.min() < 0:
                self.logtaker.error_message(
                    'Eigenvalues of the covariance matrix are not all positive; they will be ignored. '
                    'Smallest negative value: {}', var.min())
            keep = var >= self.cov_threshold
            sigma, T = np.sqrt(var[keep]), vec[:, keep].conjugate().transpose()
            object.__setattr__(self, '_cov_eig', (given, self.cov_threshold, cov, sigma, T))
        self.cov = cov
        self.err = None              # no chi2 with stale errors while the kernel changes
        if hasattr(self.cost_function, '_G_orig'):
            self.G = self.cost_function._G_orig
        self._rotate_to(T)
        self.err = sigma

    def set_cov_file(self, filename):
        self.set_cov(np.loadtxt(filename))

    # ---- bins: mean, covariance of the mean and its eigenbasis from the device ------------------------------
    @staticmethod
    def _check_bins(grid, bins, what, per_point=1):
        """``bins`` as an array whose first axis are the bins and whose last the grid; raises like the other setters"""
        bins = np.asarray(bins)
        n = len(grid)
        if bins.ndim < 2 or bins.shape[-1] != n:
            raise AssertionError("{0} must have the bins on its first and the {1} values of the grid on its last axis; "
                                 "its shape is {2}".format(what, n, bins.shape))
        if bins.shape[0] < 2:
            raise AssertionError('{0}: {1} bin(s); a covariance needs at least two'.format(what, bins.shape[0]))
        if not np.all(np.isfinite(bins)):
            raise AssertionError('{0} hold {1} values that are not finite'.format(what, int((~np.isfinite(bins)).sum())))
        from . import device
        if per_point * n > device.BINS_MAX_DATA:
            raise AssertionError('{0}: {1} data values per set; the device decomposition takes at most {2} '
                                 '(set_cov takes a covariance matrix of any size)'.format(what, per_point * n,
                                                                                       device.BINS_MAX_DATA))
        return bins

    def _warn_few_bins(self, n_bins, n_data):
        if n_bins <= n_data:
            self.logtaker.error_message(
                '{} bins for {} data values: the covariance of the mean is rank-deficient, at most {} directions of the '
                'data are kept.', n_bins, n_data, n_bins - 1)

    def _device_for_bins(self):
        loop = self.maxent_loop
        return loop.device_ids[0] if getattr(loop, 'device_ids', None) else getattr(loop, 'device_id', 0)

    def _set_eigenbasis(self, sigma, T, mean=None):
        """the job a fresh object holds after ``set_G_*_data`` of ``mean`` (default: the data as supplied last) and
        ``set_cov`` of a covariance with the eigenvalues ``sigma**2`` and the eigenvectors ``T`` (rows): data and kernel
        are rotated by ``T`` alone, whatever rotation there was (no hop from the previous one as in :meth:`set_cov`)"""
        self.err = None              # no chi2 with stale errors while data and kernel change
        self.G = self.cost_function._G_orig if mean is None else mean
        self._leave_truncated_rotation()
        self._transform(T, G_original_basis=True)
        self.err = sigma

    def _leave_truncated_rotation(self):
        """A rotation that dropped directions (fewer bins than data values, or eigenvalues below ``cov_threshold``) has
        fewer rows than columns, and the hop of ``Kernel.transform`` cannot leave it: T_new T_old^H T_old K is T_new
        applied to a projection of K, not to K.  The kernel is filled again unrotated (from the cache of recent fills)
        so that the next rotation is applied to K itself -- the second matrix element of an element-wise job on such
        bins got the projected kernel.  A square rotation is left by the hop as before."""
        inner = self._inner_kernel()
        T = inner.rotation
        if inner._projected or (T is not None and T.shape[0] != T.shape[1]):
            self.K.refill_unrotated()

    def _note_shrinkage(self, n_bins, n_data, lambdas):
        """in place of the few-bins warning: with shrinkage no direction of the data is lost"""
        from .logtaker import VerbosityFlags
        lambdas = np.atleast_1d(np.asarray(lambdas, dtype=float))
        self.logtaker.message(
            VerbosityFlags.Header,
            '{} bins for {} data values: shrinkage covariance of the mean, lambda = {}',
            n_bins, n_data, '{:.4g}'.format(lambdas[0]) if lambdas.size == 1 else
            '{:.4g} .. {:.4g} over {} sets'.format(lambdas.min(), lambdas.max(), lambdas.size))

    def _bins_eig(self, stacked_bins, shrinkage=None):
        """mean and covariance eigenbasis of real ``stacked_bins`` (n_bins, n_data) from the device; changes nothing.
        ``shrinkage``: see :meth:`set_G_tau_bins` (refused with a ValueError before the device is asked for anything)"""
        from . import device
        n_bins, n_data = stacked_bins.shape
        lambda_in = device.shrinkage_argument(shrinkage, n_bins)
        if lambda_in is None:
            self._warn_few_bins(n_bins, n_data)
            st = device.bins_eig(stacked_bins, self.cov_threshold, device=self._device_for_bins())
        else:
            st = device.bins_eig_shrunk(stacked_bins, self.cov_threshold, shrinkage, device=self._device_for_bins())
            self._note_shrinkage(n_bins, n_data, st['shrinkage'])
        if st['rank'] == 0:
            raise AssertionError('no eigenvalue of the covariance of the mean is above cov_threshold = {}'.format(
                self.cov_threshold))
        return dict(st, n_bins=n_bins)

    def _adopt_bins(self, st):
        object.__setattr__(self, 'bin_statistics', st)
        self._set_eigenbasis(st['sigma'], st['T'], mean=st['mean'])

    def set_G_tau_bins(self, tau, bins, shrinkage=None):
        """G(tau) as ``bins`` of shape (n_bins, n_tau): independent estimates (Monte Carlo bins).  The data become their
        mean, the errors those of the covariance of the mean C = X^T X, X = (bins - mean) / sqrt(n_bins (n_bins - 1)):
        the job is the one of ``set_G_tau_data(tau, mean)`` and ``set_cov(C)`` on a fresh object, with ``cov_threshold``
        as the cut.  Mean and eigenbasis come from the device (``mxe_bins_eig``: the singular value decomposition of X;
        C is never formed, and small eigenvalues keep their relative accuracy); ``bin_statistics`` holds ``mean``,
        ``sigma``, ``T``, ``rank`` and ``n_bins``.  Bins that are refused leave the object as it was.  Not in the
        reference.

        ``shrinkage``: with fewer than about twice as many bins as data values the small eigenvalues of C are biased low
        (and with ``n_bins <= n_data`` directions of the data are lost).  ``'auto'`` replaces C by the shrinkage estimator
        C* = (1 - lambda) C + lambda diag(C) of Schaefer and Strimmer with the intensity lambda* estimated from the bins
        (at least 4), a number in (0, 1] fixes lambda; both on the device (``mxe_bins_eig_shrunk``, DESIGN.md section
        4y; :func:`maxent_amd.shrink_bins` is the plain function).  ``bin_statistics`` then also holds ``shrinkage``,
        ``shrinkage_raw`` and ``variance``.  ``None`` or ``0.0``: the sample covariance as before.  Anything else is a
        ValueError that leaves the object as it was."""
        tau = np.asarray(tau, dtype=float)
        bins = self._check_bins(tau, bins, 'G(tau) bins')
        if bins.ndim != 2:
            raise AssertionError('G(tau) bins must be (n_bins, n_tau); their shape is {}'.format(bins.shape))
        if np.iscomplexobj(bins):
            raise AssertionError('G(tau) bins must be real')
        st = self._bins_eig(np.asarray(bins, dtype=float), shrinkage)
        self._use_kernel(kernels.TauKernel, tau)
        self._adopt_bins(st)

    def set_G_iw_bins(self, iomega, bins, beta=None, shrinkage=None):
        """G(i omega_n) as complex ``bins`` of shape (n_bins, n_iw), see :meth:`set_G_tau_bins` (also for ``shrinkage``)
        and :meth:`set_G_iw_data`: every bin is unfolded to the stacked real vector ``[Re G ; Im G]``, mean and covariance
        are those of the 2 n_iw stacked values."""
        iomega = np.asarray(iomega, dtype=float)
        bins = self._check_bins(iomega, bins, 'G(i omega_n) bins', per_point=2)
        if bins.ndim != 2:
            raise AssertionError('G(i omega_n) bins must be (n_bins, n_iw); their shape is {}'.format(bins.shape))
        st = self._bins_eig(kernels.stack_complex(bins), shrinkage)        # (every bin as [Re ; Im])
        self._use_kernel(kernels.IOmegaKernel, iomega, beta=beta)
        self._adopt_bins(st)

    def set_G_l_bins(self, bins, beta, l=None, shrinkage=None):
        """Legendre coefficients as ``bins`` of shape (n_bins, n_l), see :meth:`set_G_tau_bins` (also for ``shrinkage``) and
        :meth:`set_G_l_data`: the job is the one of ``set_G_l_data(mean, beta, l)`` and ``set_cov(C)`` on a fresh
        object."""
        bins = np.asarray(bins)
        if bins.ndim != 2:
            raise AssertionError('G_l bins must be (n_bins, n_l); their shape is {}'.format(bins.shape))
        l = self._legendre_orders(l, bins.shape[-1])
        bins = self._check_bins(l, bins, 'G_l bins')
        if np.iscomplexobj(bins):
            raise AssertionError('G_l bins must be real')
        st = self._bins_eig(np.asarray(bins, dtype=float), shrinkage)
        self._use_kernel(kernels.LegendreKernel, l, beta=beta)
        self._adopt_bins(st)

    # ---- error bars ------------------------------------------------------------
    def posterior_errors(self, result, alpha=None, windows=None, functionals=None, pointwise=False, timing=None):
        """Posterior error bars of ``result`` (made by this object: its kernel, errors, default model and alpha mesh
        are used) in the Gaussian approximation around the minimiser, computed on the device (``mxe_posterior_var``).
        Not in the reference.

        ``alpha``: an analyzer name (default: the result's default analyzer), an index, a sequence of indices,
        ``'all'``, or ``'bryan'`` (the mixture over alpha with the weights of ``BryanAnalyzer``: mean
        ``sum p_a x_a``, variance ``sum p_a [var_a + (x_a - mean)^2]``; needs the probability).
        ``windows=[(lo, hi), ...]`` -> ``window_weight`` (the sum of H over the mesh points inside: the integral of
        A) and ``window_err``; ``functionals=F`` (n_f, n_omega: weights on ``A delta_omega``) -> ``functional_value``,
        ``functional_err``; ``pointwise=True`` -> ``A_err``, the standard deviation of A(omega_i) -- large and strongly
        correlated between neighbouring points: only integrated quantities have meaningful errors.  Always there:
        ``prior_err`` (windows, then functionals; also ``window_prior_err``, ``functional_prior_err``,
        ``A_prior_err``), the error the default model alone would leave, ``alpha``, ``alpha_index`` and ``info``
        (``nan_rows``: alphas whose H is not finite).  A sequence of alphas or ``'all'`` keeps an alpha axis in front.
        With a ``PreblurKernel`` everything refers to A = B H."""
        from . import posterior
        loop = self.maxent_loop
        spec = loop.make_spec()
        posterior.check_alpha(spec, result.alpha)
        H = np.asarray(result.element_array('H'))
        logp = np.asarray(result.element_array('probability'), dtype=float)
        item = dict(spec=spec, H=H, alpha=np.asarray(result.alpha, dtype=float), analysis=result.analyzer_results,
                    probability=None if np.all(np.isnan(logp)) else logp, B=loop.A_of_H.matrix())
        ids = loop.device_ids if loop.device_ids else (loop.device_id,)
        return posterior.element_errors(self.K, self.omega, [item], alpha=alpha, windows=windows, functionals=functionals,
                                        pointwise=pointwise, default_name=result.default_analyzer_name,
                                        chi2_factor=loop.cost_function.chi2_factor, device_ids=ids[:1],
                                        bryan=posterior.find_bryan(loop.analyzers), timing=timing)[0]

    def posterior_samples(self, result=None, n_samples=100, seed=0, alpha=None, transform='linear', z=None, timing=None):
        """Spectra drawn from the Gaussian posterior around the minimiser that :meth:`posterior_errors` integrates
        (``mxe_posterior_sample``), for error bars of what is not linear in A: a peak position or width, a gap edge, a
        quasi-particle weight, Sigma(omega) after ``set_Gaux_w_from_Aaux_w``.  Evaluate the quantity on every row of
        ``A_samples`` and take the spread.  Not in the reference.

        ``result``: a result of this object (required: a ``TauMaxEnt`` keeps none).  ``alpha`` as in
        :meth:`posterior_errors`; with ``'bryan'`` every sample's alpha is allotted with the ``BryanAnalyzer`` weights from
        ``np.random.Generator(np.random.Philox(seed))`` and returned as ``alpha_index_samples``.  ``seed``: the draw is a
        function of (seed, element, alpha, sample index) alone (a counter-based generator,
        :func:`maxent_amd.posterior.sample_normals` mirrors it), so more samples extend a draw and never change it.
        ``z``: standard normals (n_samples, n_omega + n_s) -- or one such block per chosen alpha -- used instead of the
        generator's.  ``transform='linear'``: H + delta, the Gaussian itself, consistent with :meth:`posterior_errors` (tail
        points can go negative); ``'log'``: H exp(delta / H), positive and equal to first order (normal entropy only).

        Returns a dict: ``H`` (the minimiser), ``H_samples`` (n_samples, n_omega), ``A_samples`` (H / delta_omega, or B H
        with a ``PreblurKernel``), ``alpha_index``, ``alpha``, ``seed``, ``info`` (``nan_rows``: alphas whose H is not
        finite or whose curvature is not positive definite: their samples are NaN).  A sequence of alphas or ``'all'``
        keeps an alpha axis in front."""
        from . import posterior
        if result is None:
            raise ValueError('no result: hand in the result of run()')
        loop = self.maxent_loop
        spec = loop.make_spec()
        posterior.check_alpha(spec, result.alpha)
        H = np.asarray(result.element_array('H'))
        logp = np.asarray(result.element_array('probability'), dtype=float)
        item = dict(spec=spec, H=H, alpha=np.asarray(result.alpha, dtype=float), analysis=result.analyzer_results,
                    probability=None if np.all(np.isnan(logp)) else logp, B=loop.A_of_H.matrix(), stream=0)
        ids = loop.device_ids if loop.device_ids else (loop.device_id,)
        return posterior.element_samples(self.K, self.omega, [item], n_samples=n_samples, seed=seed, alpha=alpha,
                                         transform=transform, z=z, default_name=result.default_analyzer_name,
                                         chi2_factor=loop.cost_function.chi2_factor, device_ids=ids[:1],
                                         bryan=posterior.find_bryan(loop.analyzers), timing=timing)[0]

    def fit_diagnostics(self, result, alpha='all', timing=None):
        """Diagnostics of the fits of ``result`` (made by this object: its kernel, data, errors, default model and alpha
        mesh are used) from the hat matrix of the fit -- the derivative of the fitted whitened data with respect to the
        whitened data, exact at the minimiser --, computed on the device (``mxe_fit_diagnostics``).  Not in the reference.

        ``alpha``: ``'all'`` (default), an analyzer name, an index or a sequence of indices.  Returns a dict: ``alpha``,
        ``alpha_index``; ``n_good``, the number of good data N_g = tr Hat; ``chi2``; ``residual`` =
        Sigma^-1/2 (K H - G) and ``leverage`` = diag Hat per data row (tau points; the 2 n_iw stacked real values of
        Matsubara data; the kept eigen-directions after ``set_cov`` or ``set_G_*_bins``); ``studentized`` =
        r / sqrt(1 - h) (NaN where 1 - h < 1e-12); ``autocorr`` = sum r_i r_i+1 / sum r_i^2 (NaN in a covariance
        eigenbasis, where the data index has no order); ``gcv`` = n chi2 / (n - N_g)^2; ``good_data_ratio`` =
        -2 a S / N_g with a = alpha~ / chi2_factor; ``info`` (``nan_rows``: alphas whose H is not finite or whose curvature
        is not positive definite).  With ``'all'`` also ``alpha_index_gcv`` (the smallest GCV score),
        ``alpha_index_classic`` (the ratio closest to 1 on the logarithmic scale) and the rows ``A_gcv``, ``A_classic`` of
        ``result.A``.  A single alpha drops the alpha axis in front."""
        from . import diagnostics, posterior
        loop = self.maxent_loop
        spec = loop.make_spec()
        posterior.check_alpha(spec, result.alpha)
        item = dict(spec=spec, H=np.asarray(result.element_array('H')), alpha=np.asarray(result.alpha, dtype=float),
                    S=np.asarray(result.element_array('S'), dtype=float), A=np.asarray(result.element_array('A')),
                    analysis=result.analyzer_results)
        ids = loop.device_ids if loop.device_ids else (loop.device_id,)
        return diagnostics.element_diagnostics(self.K, [item], alpha=alpha, default_name=result.default_analyzer_name,
                                               chi2_factor=loop.cost_function.chi2_factor, device_ids=ids[:1],
                                               timing=timing)[0]

    def _response_item(self, result):
        from . import posterior
        loop = self.maxent_loop
        spec = loop.make_spec()
        posterior.check_alpha(spec, result.alpha)
        item = dict(spec=spec, H=np.asarray(result.element_array('H')), alpha=np.asarray(result.alpha, dtype=float),
                    analysis=result.analyzer_results, B=loop.A_of_H.matrix())
        ids = loop.device_ids if loop.device_ids else (loop.device_id,)
        return item, dict(default_name=result.default_analyzer_name, chi2_factor=loop.cost_function.chi2_factor,
                          device_ids=ids[:1])

    def resolution(self, result, omega0=None, alpha=None, test=None, timing=None):
        """What this continuation does to a feature that is really there: the linear response of the minimiser of
        ``result`` (made by this object) to a change of the true spectrum, exact at the minimiser, computed on the device
        (``mxe_response``, :mod:`maxent_amd.response`).  Not in the reference.

        ``omega0``: a point or a sequence of points, snapped to the mesh (None: every mesh point, in chunks).  ``alpha``: an
        analyzer name (default: the result's default analyzer), an index, a sequence of indices or ``'all'``;
        ``'bryan'`` raises ``ValueError`` (the mixture weights depend on the data).  Returns a dict: ``index``, ``omega0``
        (the mesh points taken); ``psf`` (n_pts, n_omega), the change of the returned A for a unit of weight at omega0 --
        column j of the resolution operator R over delta_omega --; ``averaging_kernel`` (n_pts, n_omega), r_j with
        ``dA_returned(omega0_j) = sum_i r_j(omega_i) dA_true(omega_i) delta_omega_i``; of each psf ``weight`` (what comes back
        of the unit), ``centroid``, ``shift`` (centroid - omega0), ``spread`` (Backus-Gilbert's), ``peak``, ``height``,
        ``fwhm`` (NaN when a side does not fall to half the maximum on the mesh) and ``data_share`` = R_jj in [0, 1], the
        share of point j that the data decide (the default model decides the rest); ``alpha``, ``alpha_index``, ``info``
        (``nan_rows``).  ``test``: (n_test, n_omega) changes of the true A -> ``image``, the linearised change of the
        returned A.  A sequence of alphas or ``'all'`` keeps an alpha axis in front.  With a ``PreblurKernel`` everything
        refers to A = B H and goes through the data (dG = K_delta dA_true); ``averaging_kernel`` is None."""
        from . import response
        item, common = self._response_item(result)
        return response.element_resolution(self.K, self.omega, [item], omega0=omega0, alpha=alpha, test=test, timing=timing,
                                           note=self.logtaker.error_message, **common)[0]

    def default_model_response(self, result, dlogD, alpha=None, timing=None):
        """How much of ``result`` is the default model: the linear response ``dA`` (n_dir, n_omega) of the returned A to
        the changes ``dlogD`` (n_dir, n_omega) of ln D, ``dH = (I - R)(H o dlnD)`` with the resolution operator R of
        :meth:`resolution`, exact at the minimiser, for both entropies (``mxe_response``).  Not in the reference.
        ``alpha`` as in :meth:`resolution`.  Returns a dict: ``dA``, ``dH``, ``alpha``, ``alpha_index``, ``info``."""
        from . import response
        item, common = self._response_item(result)
        return response.element_default_model_response(self.K, self.omega, [item], dlogD, alpha=alpha, timing=timing,
                                                       **common)[0]

    def resample_errors(self, bins, method='jackknife', block=1, n_resamples=None, seed=None, alpha=None,
                        alpha_mode='per_resample', windows=None, functionals=None, pointwise=True, keep_samples=False,
                        timing=None, quantiles=None):
        """Jackknife or bootstrap error bars from the Monte Carlo ``bins`` the last ``set_G_tau_bins`` / ``set_G_iw_bins``
        call of this object received: every resample of the bins is continued with the covariance of the full sample (one
        launch for all of them, :mod:`maxent_amd.resampling`) and the spread of the results is taken on the device.  The
        object is not changed.  Not in the reference.

        ``method='jackknife'``: ``n_bins // block`` leave-one-block-out resamples; ``'bootstrap'``: ``n_resamples`` draws
        with ``numpy.random.default_rng(seed)`` (``seed`` is required).  ``alpha``: the analyzer whose alpha is taken
        (``'LineFitAnalyzer'``, ``'Chi2CurvatureAnalyzer'``, ``'EntropyAnalyzer'``; default: the first analyzer of this
        object, if it is one of them), or one index.  ``alpha_mode='per_resample'``: every resample at the alpha the
        analyzer picks for its own scan -- the uncertainty of the alpha selection is inside the error --;
        ``'full_sample'``: all at the alpha of the full sample.  ``windows``, ``functionals``, ``pointwise`` as in
        :meth:`posterior_errors` (with a ``PreblurKernel`` they refer to A = B H).

        Returns a dict: ``A``, ``alpha``, ``alpha_index`` (the full sample at its alpha); ``A_mean``, ``A_err`` (and
        ``A_bias`` = (n_used - 1) (A_mean - A), jackknife only) with ``pointwise``; ``window_weight`` (the mean over the
        resamples), ``window_err``, ``window_full`` (the full sample's); ``functional_value``, ``functional_err``,
        ``functional_cov``, ``functional_full``; ``alpha_index_samples`` (n_res); ``n_used`` (a resample whose chosen
        alpha failed is left out), ``n_resamples``, ``method``; ``info`` (kernel times, launches, ``n_datasets``,
        ``left_out``); with ``keep_samples`` ``samples['H']`` (n_res, n_omega) and ``samples['functional']``
        (n_res, windows then functionals) for anything nonlinear downstream.  ``quantiles`` (bootstrap only; with the
        jackknife a ``ValueError``: pseudo-values are not a sample of the distribution): probabilities in [0, 1] ->
        ``quantiles``, ``A_quantiles`` (n_q, n_omega), ``window_quantiles``, ``functional_quantiles``, the percentile
        intervals over the resamples (type 7, numpy's default; ``mxe_resample_quantiles``)."""
        from . import resampling
        return resampling.tau_resample_errors(self, bins, method=method, block=block, n_resamples=n_resamples, seed=seed,
                                              alpha=alpha, alpha_mode=alpha_mode, windows=windows, functionals=functionals,
                                              pointwise=pointwise, keep_samples=keep_samples, timing=timing,
                                              quantiles=quantiles)

    def parametric_bootstrap(self, result=None, n_mock=200, seed=None, alpha=None, alpha_mode='per_mock',
                             quantiles=(0.16, 0.5, 0.84), windows=None, functionals=None, pointwise=True, keep_samples=False,
                             keep_data=False, timing=None):
        """Parametric bootstrap (closure test) of this continuation, for data without bins: ``n_mock`` mock data sets are
        drawn from the continued spectrum with the noise of the job -- N(K H0, diag(err^2)) in the data space of the job:
        the eigenbasis after ``set_cov``, the stacked real form of Matsubara data --, every one is continued exactly like
        the data (one launch for all of them, :mod:`maxent_amd.mock`), and the distribution of what comes back is reduced
        on the device.  This is the distribution of the procedure's answers to data from ONE spectrum, not a posterior.
        The object is not changed.  Not in the reference.

        ``result``: a result of this object's present job (None: ``run()``); another job's is refused before anything is
        launched.  ``alpha`` as in :meth:`resample_errors`; H0 is the row of ``result.H`` at that pick.  ``seed`` is
        required; the mocks are rows of the counter-based generator of :meth:`posterior_samples`
        (:func:`maxent_amd.mock.mock_rows` mirrors them), so more mocks extend a draw.  ``alpha_mode='per_mock'``: every
        mock at the alpha the analyzer picks for its own scan; ``'fixed'``: all at the pick of the data.  ``quantiles``:
        probabilities in [0, 1] or None.  ``windows``, ``functionals``, ``pointwise`` as in :meth:`resample_errors`
        (with a ``PreblurKernel`` they refer to A = B H; at most 1024 mocks with ``quantiles``).

        Returns the keys of :meth:`resample_errors` (``A``, ``A_mean``, ``A_err``, ``alpha_index``,
        ``alpha_index_samples``, ``n_used``, ``window_*``, ``functional_*``, ``info``, ``samples`` with
        ``keep_samples``) and: ``A_bias`` = A_mean - A -- the mocks were drawn from A, so this is what the procedure does
        to A on average (it says nothing about the distance of A from the truth) --; ``A_quantiles`` (n_q, n_omega),
        ``quantiles``, ``window_quantiles``, ``functional_quantiles``; ``chi2`` (the data's at its pick),
        ``chi2_samples`` (every mock's at its own pick), ``chi2_p_value`` (:func:`maxent_amd.mock.chi2_p_value`);
        ``G_mock`` (n_mock, n_data) with ``keep_data``; ``method='parametric'``, ``n_mock``, ``seed``."""
        from . import mock
        return mock.tau_parametric_bootstrap(self, result=result, n_mock=n_mock, seed=seed, alpha=alpha, alpha_mode=alpha_mode,
                                             quantiles=quantiles, windows=windows, functionals=functionals,
                                             pointwise=pointwise, keep_samples=keep_samples, keep_data=keep_data,
                                             timing=timing)

    def cross_validate(self, bins, n_folds=5, rule='min', result=None, keep_rows=False, timing=None):
        """k-fold cross-validation of alpha over the Monte Carlo ``bins`` the last ``set_G_tau_bins`` / ``set_G_iw_bins`` /
        ``set_G_l_bins`` call of this object received: does the spectrum continued from one part of the bins predict the
        other part?  The bins are cut into ``n_folds`` contiguous folds (the bin index is Monte Carlo time); the mean of the
        bins outside fold f is continued over the whole alpha mesh -- the full sample and the folds are one launch, with
        the covariance of the full sample as ``set_G_*_bins`` staged it --, and every H row of that scan is scored on the
        device against the mean of fold f (``mxe_cv_score``, :mod:`maxent_amd.cross_validation`):
        ``chi2_val = sum_k w_k ((T K H)_k - (T mean_f)_k)^2`` with ``w_k = N_f / (N sigma_k^2)``, sigma_k the error of the
        full-sample mean along eigen-direction k.  The object is not changed.  Not in the reference.

        The training solve at mesh alpha uses the full-sample sigma; a training mean of N - N_f bins is noisier by
        N / (N - N_f), so the solve equals one with the training mean's own error at alpha (N - N_f) / N
        (``info['alpha_train_factor']``).  The pick is applied to the full sample at the same mesh index (the plug-in
        rule); sigma is estimated from all bins, the validation fold included; with few bins per fold the score is noisy,
        ``score_err`` says how noisy.

        Returns a dict: ``alpha`` (the mesh); ``fold_scores`` (K, n_alpha) = chi2_val / rank; ``score`` (their mean over
        the folds) and ``score_err`` (their standard deviation / sqrt(K)); ``train_chi2`` (K, n_alpha); ``alpha_index_cv``
        (the argmin of ``score`` over the alphas at which every fold is finite, -1 if there is none; of equal scores the
        larger alpha); ``alpha_index_one_se`` (the largest alpha whose score is <= the minimum + ``score_err`` at the
        minimum); ``alpha_at_edge`` (the minimum sits on an end of the mesh: widen it); ``A_cv``, ``A_one_se`` (the rows of
        the full-sample scan at those indices; with a ``PreblurKernel`` A = B H); ``z`` (K, rank), the out-of-sample
        whitened residuals at ``alpha_index_cv``, and ``calibration``, the mean of z^2 (about 1 when the error bars are
        right); ``left_out`` (the (fold, alpha) pairs that were not finite); ``folds`` (the bin ranges); ``info``
        (``kernel_ms``, ``score_ms``, ``launches``, ``devices``, ``alpha_train_factor``).  ``keep_rows``: also ``rows_H``
        (K, n_alpha, n_omega), the H rows that were scored.

        ``result``: a result of ``run()`` on the same alpha mesh (another mesh raises ``ValueError``) gets the entry
        ``analyzer_results['CrossValidationAnalyzer']`` whose ``alpha_index`` and ``A_out`` follow ``rule`` (``'min'`` or
        ``'one_se'``): ``result.get_A_out('CrossValidationAnalyzer')`` and ``posterior_errors(result,
        alpha='CrossValidationAnalyzer')`` then work; the default analyzer stays what it was."""
        from . import cross_validation
        return cross_validation.tau_cross_validate(self, bins, n_folds=n_folds, rule=rule, result=result, keep_rows=keep_rows,
                                                   timing=timing)

    def default_model_scan(self, models, prior=None, alpha='bryan', windows=None, functionals=None, pointwise=True,
                           keep_models=True, timing=None):
        """Continue the data of this object under a family of default models in one launch and let the data say which
        they prefer (:mod:`maxent_amd.model_scan`, ``mxe_evidence_reduce``).  The object is not changed.  Not in the
        reference.

        ``models``: a list, or a dict name -> model, of ``BaseDefaultModel`` objects on this object's omega mesh or
        arrays of length n_omega holding ``D`` (density times delta_omega).  ``prior``: P(model), one value per model
        (default: equal; 0 switches a model off).  ``alpha``: ``'bryan'`` (default; the mixture over alpha with the weights
        of ``BryanAnalyzer``, ``average_by_integration`` as the one among this object's analyzers has it), ``'classic'``
        (the alpha of the largest probability), ``'LineFitAnalyzer'``, ``'Chi2CurvatureAnalyzer'``, ``'EntropyAnalyzer'``
        or one index.  ``windows``, ``functionals``, ``pointwise`` as in :meth:`posterior_errors` (with a
        ``PreblurKernel`` they refer to A = B H).  The probability is the object's, or ``NormalLogProbability()`` when it
        has none.

        Returns a dict: ``log_evidence`` (n_models), log of the integral of p(alpha, D | G) over the alpha mesh --
        comparable between models on the same data, errors, omega mesh and alpha mesh only --; ``log_bayes_factor``
        (``log_evidence`` minus the largest); ``weight`` (prior times evidence, normalised), ``best``, ``n_eff`` =
        1 / sum weight^2; ``alpha_index`` per model (the alpha of the largest probability, or the pick);
        ``alpha_at_edge`` per model: True where the probability peaks at the first or last alpha -- the mesh then
        truncates that model's evidence integral and its ``log_evidence`` is a lower bound: widen the alpha mesh --;
        ``n_good`` (alphas that have a probability and a finite H); ``A`` (the evidence-weighted average) and
        ``A_model_err`` (the spread between the models, the square root of the weighted centred second moment) with
        ``pointwise``; ``A_models`` (n_models, n_omega) with ``keep_models``; ``window_weight``, ``window_err``,
        ``window_models``; ``functional_value``, ``functional_err``, ``functional_cov``, ``functional_models``;
        ``names``; ``info`` (``kernel_ms``, ``reduce_ms``, ``launches``, ``devices``; ``audit_max`` with
        ``MAXENT_AMD_AUDIT=1``)."""
        from . import model_scan
        return model_scan.tau_default_model_scan(self, models, prior=prior, alpha=alpha, windows=windows,
                                                 functionals=functionals, pointwise=pointwise, keep_models=keep_models,
                                                 timing=timing)

    def check_bins(self, bins, basis='eigen'):
        """May the Monte Carlo ``bins`` the last ``set_G_*_bins`` call received be used as they are?  The covariance of
        the mean is right for bins that are uncorrelated, chi^2 is a log-likelihood for bins that are normally
        distributed; the device (``mxe_bins_check``, :mod:`maxent_amd.bin_checks`) tests both on blocks of 1, 2, 4, ...
        successive bins -- the bin index must be Monte Carlo time.  The object is not changed.  Not in the reference.

        ``basis='eigen'``: per kept eigen-direction of the covariance (``bin_statistics``), the directions chi^2 sums;
        ``'data'``: per data value (the stacked ``[Re ; Im]`` values of Matsubara bins), which needs no earlier
        ``set_G_*_bins`` call.  Returns the dict of :func:`maxent_amd.bin_checks.summarize`: per level ``block``,
        ``n_blocks``, ``err2``, ``inefficiency`` (the estimate of 2 tau_int), its column mean ``R``, ``skew``, ``kurt``,
        their z-scores, ``frac_non_normal``; ``plateau_level`` and ``recommended_block`` (None: the bins are correlated
        beyond what their number resolves).  A ``recommended_block`` other than 1 is reported through the logtaker's
        error messages: pass ``rebin_bins(bins, block)`` to the setter."""
        from . import bin_checks
        return bin_checks.tau_check_bins(self, bins, basis=basis)

    # ---- tau ----------------------------------------------------------------
    def get_tau(self):
        return self.maxent_loop.get_data_variable()

    def set_tau(self, tau, update_K=True, update_chi2=True, update_Q=True,
                update_H_of_v=True):
        """a new tau grid refills the kernel (and drops its SVD); setting the
        grid it already has is free -- this is what lets the element-wise
        driver reuse one SVD for all matrix elements, where the reference
        recomputes it per element.  Returns whether the grid was new."""
        old = self.maxent_loop.get_data_variable()
        same = old is not None and np.shape(old) == np.shape(tau) and \
            np.array_equal(np.asarray(old), np.asarray(tau))
        if same:
            return False
        self.maxent_loop.set_data_variable(tau, update_K=update_K,
                                           update_chi2=update_chi2,
                                           update_Q=update_Q,
                                           update_H_of_v=update_H_of_v)
        return True

    tau = property(get_tau, set_tau)

    @property
    def _T(self):
        return self.K._T
