"""Helpers around a continuation (the reference's python/maxent_util.py): G(w) from A(w) by Kramers-Kronig and
G(tau) from A(w); chi(w) from the A(w) = Im chi(w) / (pi w) of a bosonic continuation, Legendre coefficients G_l from
A(w) and G(tau) from G_l (not in the reference).

The reference returns TRIQS Green functions (``GfReFreq``, ``GfImTime``); here :class:`ArrayGf` takes their place: a
mesh array and a data array in TRIQS's layout ``(n_points, n, n)``, so ``g.data[:, 0, 0]`` and
``[w.real for w in g.mesh]`` read as they do on a TRIQS Gf.  The Kramers-Kronig sum runs on the device
(``mxe_kramers_kronig``); there is no CPU fallback.
"""

import numpy as np

from . import device
from .kernels import LegendreKernel, TauKernel
from .omega_meshes import DataOmegaMesh

__all__ = ['ArrayGf', 'get_G_w_from_A_w', 'get_chi_w_from_A_w', 'get_G_tau_from_A_w', 'get_G_l_from_A_w',
           'get_G_tau_from_G_l', 'kramers_kronig']


class ArrayGf(object):
    """A Green function on a mesh as plain arrays: ``mesh`` (1-D float: real frequencies, Matsubara frequencies
    omega_n or tau) and ``data`` (complex ``(n_points, n, n)``, TRIQS's layout).  Takes the place of the TRIQS Gf
    objects the reference passes around; picklable."""

    def __init__(self, mesh, data):
        self.mesh = np.array(mesh, dtype=float).ravel()
        data = np.array(data, dtype=complex)
        if data.ndim == 1:
            data = data[:, None, None]
        if data.ndim != 3 or data.shape[0] != len(self.mesh) or data.shape[1] != data.shape[2]:
            raise ValueError('ArrayGf: data must be (n_points, n, n) or (n_points,) on a mesh of n_points; got %s on %d'
                             % (data.shape, len(self.mesh)))
        self.data = data

    @property
    def target_shape(self):
        return self.data.shape[1:]

    def copy(self):
        return ArrayGf(self.mesh, self.data)

    def __reduce_to_dict__(self):
        return {'mesh': self.mesh, 'data': self.data}

    @classmethod
    def __factory_from_dict__(cls, name, D):
        return cls(D['mesh'], D['data'])

    def __repr__(self):
        return 'ArrayGf(%d points, target_shape=%s)' % (len(self.mesh), self.target_shape)


def _kk_weights(w_points, broadening_factor):
    """the reference's Delta_j = (w[min(j+1, n-1)] - w[max(j-1, 0)]) / 2 (maxent_util.py:115-116) and its broadening"""
    w = np.asarray(w_points, dtype=float).ravel()
    n = len(w)
    j = np.arange(n)
    delta = (w[np.minimum(j + 1, n - 1)] - w[np.maximum(j - 1, 0)]) * 0.5
    return w, delta, broadening_factor * delta


def _kk_rows(rows_list, w_points, w_out, broadening_factor, bosonic=False):
    """one device launch for a list of spectra arrays ``(..., n_w)`` on the same grid; returns their G, complex
    ``(..., n_out)`` each.  A complex spectrum goes as its real and imaginary rows, recombined as G(Re A) + i G(Im A).
    ``bosonic``: weight_j -> -w_j weight_j, the sum of :func:`get_chi_w_from_A_w` (the broadening stays)."""
    w, weight, eta = _kk_weights(w_points, broadening_factor)
    if bosonic:
        weight = -w * weight
    n_w = len(w)
    real_rows, plan = [], []
    for A in rows_list:
        A = np.asarray(A)
        if A.ndim < 1 or A.shape[-1] != n_w:
            raise ValueError('kramers_kronig: A of shape %s does not end in the %d points of w_points' % (A.shape, n_w))
        r = A.reshape(-1, n_w)
        cplx = np.iscomplexobj(A)
        real_rows.append(r.real.astype(float))
        if cplx:
            real_rows.append(r.imag.astype(float))
        plan.append((A.shape[:-1], r.shape[0], cplx))
    G_all = device.kramers_kronig(w, weight, eta, w_out, np.concatenate(real_rows, axis=0))
    out, at = [], 0
    for lead, n, cplx in plan:
        G = G_all[at:at + n]
        at += n
        if cplx:
            G = G + 1j * G_all[at:at + n]
            at += n
        out.append(G.reshape(lead + (len(w_out),)))
    return out


def kramers_kronig(A, w_points, w_out, broadening_factor=1.0):
    r"""Batched Kramers-Kronig transform, the primitive behind :func:`get_G_w_from_A_w`:

    .. math:: G(\omega_o) = \sum_j A(\omega_j) \Delta_j / (\omega_o - \omega_j + i\, bf \Delta_j),
              \quad \Delta_j = (\omega_{j+1} - \omega_{j-1}) / 2

    (one-sided at the ends).  ``A``: real or complex, any leading shape ``(..., n_w)`` -- every alpha of every
    element of a result, say -- on ``w_points``; returns complex ``(..., len(w_out))``, all in one device launch."""
    w_out = np.asarray(w_out, dtype=float).ravel()
    return _kk_rows([A], w_points, w_out, broadening_factor)[0]


def _check_A_w(A_w, w_min, w_max):
    shape_A = np.shape(A_w)
    if len(shape_A) == 1:
        matrix_valued = False
    elif len(shape_A) == 3 and shape_A[0] == shape_A[1]:
        matrix_valued = True
    else:
        raise Exception('A_w has wrong shape, must be n x n x n_w')
    if w_min > w_max:
        raise Exception('w_min must be smaller than w_max')
    return matrix_valued


def _interp_A_w(A_w, w_points, np_interp_A):
    """the reference's optional interpolation onto linspace(min w, max w, np_interp_A) (maxent_util.py:96-109)"""
    w_points = np.asarray(w_points, dtype=float)
    if not np_interp_A:
        return np.asarray(A_w), w_points
    w_interp = np.linspace(np.min(w_points), np.max(w_points), np_interp_A)
    A_w = np.asarray(A_w)
    if A_w.ndim == 3:
        A_temp = np.zeros((A_w.shape[0], A_w.shape[1], np_interp_A), dtype=complex)
        for i in range(A_w.shape[0]):
            for j in range(A_w.shape[1]):
                A_temp[i, j, :] = np.interp(w_interp, w_points, A_w[i, j, :])
        A_w = A_temp
    else:
        A_w = np.interp(w_interp, w_points, A_w)
    return A_w, w_interp


def _to_array_gf(G, w_out):
    """(n_out,) or (n, n, n_out) -> ArrayGf of (n_out, n, n)"""
    if G.ndim == 1:
        return ArrayGf(w_out, G[:, None, None])
    return ArrayGf(w_out, np.transpose(G, (2, 0, 1)))


def _get_G_w_from_A_w_many(A_ws, w_points, np_interp_A=None, np_omega=2000, w_min=-10, w_max=10,
                           broadening_factor=1.0):
    """:func:`get_G_w_from_A_w` for a list of spectra on one grid, in one device launch"""
    for A_w in A_ws:
        _check_A_w(A_w, w_min, w_max)
    prepared = [_interp_A_w(A_w, w_points, np_interp_A) for A_w in A_ws]
    w = prepared[0][1] if prepared else np.asarray(w_points, dtype=float)
    w_out = np.linspace(w_min, w_max, np_omega)
    Gs = _kk_rows([A for A, _ in prepared], w, w_out, broadening_factor)
    return [_to_array_gf(G, w_out) for G in Gs]


def get_G_w_from_A_w(A_w, w_points, np_interp_A=None, np_omega=2000, w_min=-10, w_max=10, broadening_factor=1.0):
    r"""Use Kramers-Kronig to determine the retarded Green function :math:`G(\omega)` from the spectral function
    :math:`A(\omega)` (reference maxent_util.py:43-132):

    .. math:: G(\omega) = \sum_j A(\omega_j) \Delta\omega_j / (\omega - \omega_j + i\, bf \Delta\omega_j)

    with the numerical broadening :math:`bf \cdot i\Delta\omega_j` (bf = ``broadening_factor``).  Unlike what the
    reference's docstring says, A is *not* normalised (neither does the reference's code).  The sum runs on the device.

    Parameters
    ----------
    A_w : array
        Real-frequency spectral function, 1-D or ``(n, n, n_w)``, real or complex.
    w_points : array
        Real-frequency grid points.
    np_interp_A : int
        If given, A_w is first interpolated (``np.interp``) onto ``np_interp_A`` equidistant points from
        min(w_points) to max(w_points).
    np_omega : int
        Number of equidistant grid points of the output Green function.
    w_min, w_max : float
        First and last point of the output Green function's mesh.
    broadening_factor : float
        Factor multiplying the broadening :math:`i\Delta\omega`.

    Returns
    -------
    G_w : ArrayGf
        ``mesh`` = linspace(w_min, w_max, np_omega) (the mesh of TRIQS's ``GfReFreq(window, n_points)``), ``data``
        complex ``(np_omega, n, n)`` (n = 1 for a 1-D A_w).
    """
    return _get_G_w_from_A_w_many([A_w], w_points, np_interp_A, np_omega, w_min, w_max, broadening_factor)[0]


def _mirror_half_axis(A_w, w_points):
    """a spectrum given on w >= 0 with A(w) = A(-w) on the whole axis: (A, w) with the mirrored points in front (a
    point w = 0 is not doubled)"""
    w = np.asarray(w_points, dtype=float).ravel()
    A_w = np.asarray(A_w)
    if len(w) < 1 or np.any(w < 0.0) or np.any(np.diff(w) <= 0.0):
        raise Exception('symmetric: w_points must be increasing and >= 0')
    if A_w.shape[-1] != len(w):
        raise Exception('A_w does not end in the %d points of w_points' % len(w))
    k = 1 if w[0] == 0.0 else 0
    return (np.concatenate([A_w[..., :k - 1 if k else None:-1], A_w], axis=-1),
            np.concatenate([-w[:k - 1 if k else None:-1], w]))


def get_chi_w_from_A_w(A_w, w_points, np_interp_A=None, np_omega=2000, w_min=-10, w_max=10, broadening_factor=1.0,
                       symmetric=False):
    r"""The retarded bosonic correlator :math:`\chi(\omega + i0)` from the spectral function
    :math:`A(\omega) = \mathrm{Im}\,\chi(\omega)/(\pi\omega)` of a bosonic continuation
    (:meth:`TauMaxEnt.set_chi_tau_data`, :meth:`TauMaxEnt.set_chi_iw_data`):

    .. math:: \chi(\omega) = \sum_j \omega_j A(\omega_j) \Delta\omega_j / (\omega_j - \omega - i\, bf \Delta\omega_j)

    so that :math:`\mathrm{Im}\,\chi(\omega) = \pi\omega A(\omega)` and :math:`\mathrm{Re}\,\chi(0) = \int A`.  It is
    the sum of :func:`get_G_w_from_A_w` with the weight :math:`-\omega_j\Delta\omega_j`, on the device
    (``mxe_kramers_kronig``).  Parameters and return value as :func:`get_G_w_from_A_w`; ``symmetric``: ``A_w`` is given
    on ``w_points`` >= 0 only and mirrored, A(-w) = A(w), before anything else."""
    _check_A_w(A_w, w_min, w_max)
    if symmetric:
        A_w, w_points = _mirror_half_axis(A_w, w_points)
    A_w, w = _interp_A_w(A_w, w_points, np_interp_A)
    w_out = np.linspace(w_min, w_max, np_omega)
    return _to_array_gf(_kk_rows([A_w], w, w_out, broadening_factor, bosonic=True)[0], w_out)


def get_G_tau_from_A_w(A_w, w_points, beta, np_tau):
    r"""Calculate :math:`G(\tau)` for a given :math:`A(\omega)` (reference maxent_util.py:135-167):
    ``TauKernel(linspace(0, beta, np_tau), w_points, beta).K_delta @ A_w``.  ``w_points``: an array or an omega
    mesh.  Returns an :class:`ArrayGf` of shape ``(np_tau, 1, 1)`` on the tau mesh."""
    if not hasattr(w_points, 'delta'):
        w_points = DataOmegaMesh(w_points)
    tau = np.linspace(0.0, beta, np_tau)
    K = TauKernel(tau=tau, omega=w_points, beta=beta)
    return ArrayGf(tau, np.dot(np.asarray(K.K_delta), A_w)[:, None, None])


def get_G_l_from_A_w(A_w, w_points, l, beta):
    r"""The Legendre coefficients :math:`G_l` (TRIQS's ``GfLegendre`` normalisation) of the G that belongs to
    :math:`A(\omega)`: ``LegendreKernel(l, w_points, beta).K_delta @ A_w``.  ``w_points``: an array or an omega mesh;
    ``l``: the orders.  Returns an array of ``len(l)`` values.  Not in the reference."""
    if not hasattr(w_points, 'delta'):
        w_points = DataOmegaMesh(w_points)
    K = LegendreKernel(l, w_points, beta=beta)
    return np.dot(np.asarray(K.K_delta), A_w)


def get_G_tau_from_G_l(G_l, l, tau, beta):
    r""":math:`G(\tau) = \sum_l \sqrt{2l+1}/\beta\; P_l(2\tau/\beta - 1)\, G_l` at the points ``tau`` (an array) from the
    Legendre coefficients ``G_l`` (last axis) of the orders ``l``.  Returns an array ``(..., len(tau))``.  Not in the
    reference."""
    l = LegendreKernel._checked_l(l)
    G_l = np.asarray(G_l)
    if G_l.shape[-1] != len(l):
        raise ValueError('G_l does not end in the %d orders of l' % len(l))
    c = np.zeros(G_l.shape[:-1] + (int(l.max()) + 1,), dtype=G_l.dtype if np.iscomplexobj(G_l) else float)
    c[..., l] = np.sqrt(2.0 * l + 1.0) / beta * G_l
    x = 2.0 * np.asarray(tau, dtype=float) / beta - 1.0
    # legval takes the coefficients on the FIRST axis and returns (..., len(x))
    return np.polynomial.legendre.legval(x, np.moveaxis(c, -1, 0))
