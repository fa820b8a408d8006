"""Analytic continuation of self-energies (the reference's python/sigma_continuator.py), on arrays.

The workflow of the reference's guide (doc/guide/sigma_continuator.rst): build an auxiliary Green function
G_aux(i omega_n) from Sigma(i omega_n), continue it (``TauMaxEnt.set_G_iw_data``), turn A_aux(omega) into G_aux(omega)
by Kramers-Kronig (``set_Gaux_w_from_Aaux_w``, on the device) and invert that to Sigma(omega) (``S_w``).

Where the reference takes TRIQS Green functions, these classes take :class:`~maxent_amd.maxent_util.ArrayGf` (mesh =
the real Matsubara frequencies omega_n, data ``(n_iw, n, n)`` or ``(n_iw,)``) or a ``(mesh, data)`` tuple; a ``dict``
name -> such takes the place of a BlockGf, and ``Gaux_iw``, ``Gaux_w`` and ``S_w`` then are dicts of the same keys.
"""

import numpy as np

from .maxent_util import ArrayGf, _get_G_w_from_A_w_many

__all__ = ['SigmaContinuator', 'InversionSigmaContinuator', 'DirectSigmaContinuator']


def _as_gf(g):
    if isinstance(g, ArrayGf):
        return g
    if isinstance(g, tuple) and len(g) == 2:
        return ArrayGf(*g)
    raise NotImplementedError('SigmaContinuator takes ArrayGf or (mesh, data) tuples (or a dict of them for blocks)')


def _blocks(g):
    """(name, gf) pairs: the blocks of a dict, or the one unnamed block '0' (the reference's name for it)"""
    return list(g.items()) if isinstance(g, dict) else [('0', g)]


def _unblocks(pairs, block):
    return dict(pairs) if block else pairs[0][1]


def _identity(n):
    return np.eye(n)[None, :, :]


class SigmaContinuator(object):
    """Base class for the analytic continuation of self-energies"""

    def __init__(self):
        self._BlockGf = False
        self._constant_shift = {}

    def set_S_iw(self, S_iw):
        """Set the Matsubara self-energy: an ArrayGf, a (mesh, data) tuple, or a dict of them (blocks)"""
        self.S_iw = self.check_S_iw(S_iw)

    def check_S_iw(self, S_iw):
        """the self-energy as ArrayGf (or a dict of them); raises for anything else"""
        if isinstance(S_iw, dict):
            self._BlockGf = True
            if not S_iw:
                raise ValueError('SigmaContinuator: no blocks')
            return {name: self.check_S_iw(s) for name, s in S_iw.items()}
        return _as_gf(S_iw)

    def check_Gaux_w(self, Gaux_w):
        """G_aux(omega) as ArrayGf (or a dict of them with the block names of S_iw); raises for anything else"""
        if self._BlockGf:
            if not isinstance(Gaux_w, dict) or set(Gaux_w.keys()) != set(self.S_iw.keys()):
                raise IOError('Block names of Gaux_w do not agree with S_iw')
            return {name: _as_gf(Gaux_w[name]) for name in self.S_iw}
        if isinstance(Gaux_w, dict):
            raise IOError('Gaux_w has blocks, S_iw has none')
        return _as_gf(Gaux_w)

    def set_Gaux_w_from_Aaux_w(self, Aaux_w, w_points, *args, **kwargs):
        r"""Calculate the auxiliary Green function :math:`G_{aux}(\omega)` from the auxiliary spectral function
        :math:`A_{aux}(\omega)` with :func:`~maxent_amd.maxent_util.get_G_w_from_A_w` and call :meth:`set_Gaux_w`.
        Further arguments go to ``get_G_w_from_A_w``; all blocks go through one device launch.

        Parameters
        ==========
        Aaux_w : dict or array
            Real-frequency spectral function as numpy array or, for blocks, a dict of arrays with the keys of S_iw.
        w_points : array
            Real-frequency grid points.
        """
        if self._BlockGf:
            if not isinstance(Aaux_w, dict) or set(self.S_iw.keys()) != set(Aaux_w.keys()):
                raise Exception('Indices of Aaux dictionary are not the same as in S_iw')
            names = list(self.S_iw.keys())
            for name in names:
                if not isinstance(Aaux_w[name], np.ndarray):
                    raise Exception('Please supply Aaux_w as a dict of numpy ndarrays.')
            gs = _get_G_w_from_A_w_many([Aaux_w[name] for name in names], w_points, *args, **kwargs)
            self.set_Gaux_w(dict(zip(names, gs)))
        else:
            if not isinstance(Aaux_w, np.ndarray):
                raise Exception('Please supply Aaux_w as a numpy ndarray.')
            self.set_Gaux_w(_get_G_w_from_A_w_many([Aaux_w], w_points, *args, **kwargs)[0])

    def set_Gaux_w(self, Gaux_w):
        r"""Set the auxiliary real-frequency Green function :math:`G_{aux}(\omega)` (ArrayGf, or a dict of them) and
        calculate the real-frequency self-energy :math:`\Sigma(\omega)`, stored as ``S_w``."""
        self.Gaux_w = self.check_Gaux_w(Gaux_w)
        self._calculate_S_w()

    def _calculate_Gaux_iw(self):
        raise NotImplementedError('Please use a subclass of SigmaContinuator.')

    def _calculate_S_w(self):
        raise NotImplementedError('Please use a subclass of SigmaContinuator.')

    def __reduce_to_dict__(self):
        return dict(self.__dict__)

    @classmethod
    def __factory_from_dict__(cls, name, D):
        self = cls(D['S_iw'])
        for key in D:
            setattr(self, key, D[key])
        return self


class InversionSigmaContinuator(SigmaContinuator):
    r"""Inversion method to construct the auxiliary Green function

    :math:`G_{aux}(i\omega_n) = [(i\omega_n + C) 1 - \Sigma(i\omega_n)]^{-1}` (a matrix inverse per frequency) and
    :math:`\Sigma(\omega) = (\omega + C) 1 - G_{aux}(\omega)^{-1}`.

    Parameters
    ==========
    S_iw : ArrayGf, (mesh, data) or dict of them
        Self-energy :math:`\Sigma(i\omega_n)` on the real Matsubara frequencies :math:`\omega_n`
    constant_shift : float or dict
        Constant C (usually the double counting); for blocks a scalar for all or a dict per block
    """

    def __init__(self, S_iw, constant_shift=0):
        super(InversionSigmaContinuator, self).__init__()
        self.set_S_iw(S_iw)
        if not self._BlockGf:
            self._constant_shift['0'] = constant_shift
        elif isinstance(constant_shift, dict) and set(constant_shift.keys()) == set(self.S_iw.keys()):
            self._constant_shift = dict(constant_shift)
        else:
            self._constant_shift = dict.fromkeys(self.S_iw.keys(), constant_shift)
        self._calculate_Gaux_iw()

    def _calculate_Gaux_iw(self):
        out = []
        for name, s in _blocks(self.S_iw):
            n = s.target_shape[0]
            z = 1j * s.mesh + self._constant_shift[name]
            out.append((name, ArrayGf(s.mesh, np.linalg.inv(z[:, None, None] * _identity(n) - s.data))))
        self.Gaux_iw = _unblocks(out, self._BlockGf)

    def _calculate_S_w(self):
        out = []
        for name, g in _blocks(self.Gaux_w):
            n = g.target_shape[0]
            z = g.mesh + self._constant_shift[name]
            out.append((name, ArrayGf(g.mesh, z[:, None, None] * _identity(n) - np.linalg.inv(g.data))))
        self.S_w = _unblocks(out, self._BlockGf)


def fit_tail(iomega, S, tail_fraction=0.2, expansion_order=4):
    r"""High-frequency expansion :math:`S(i\omega_n) \approx \sum_{k=0}^{K} c_k (i\omega_n)^{-k}` with real c_k,
    fitted by least squares to the ``tail_fraction`` of the frequencies of largest :math:`|\omega_n|` (at least
    K + 1 of them); columns are scaled by :math:`\omega_{max}^k` for conditioning.  Returns c_0 .. c_K.  (Takes the
    place of TRIQS's ``fit_tail()``.)"""
    iomega = np.asarray(iomega, dtype=float)
    S = np.asarray(S, dtype=complex)
    K = int(expansion_order)
    if K < 1:
        raise ValueError('expansion_order must be >= 1')
    n = len(iomega)
    n_fit = max(K + 1, int(np.ceil(tail_fraction * n)))
    if n_fit > n:
        raise ValueError('%d frequencies are too few for a tail fit of order %d' % (n, K))
    idx = np.argsort(np.abs(iomega))[n - n_fit:]
    wmax = np.max(np.abs(iomega[idx]))
    x = 1j * iomega[idx] / wmax                        # |x| <= 1
    cols = np.stack([x ** (-k) for k in range(K + 1)], axis=1)
    M = np.concatenate([cols.real, cols.imag])        # real unknowns: the equations' real and imaginary parts
    rhs = np.concatenate([S[idx].real, S[idx].imag])
    scale = np.linalg.norm(M, axis=0)
    c, *_ = np.linalg.lstsq(M / scale, rhs, rcond=None)
    return c / scale * wmax ** np.arange(K + 1)


class DirectSigmaContinuator(SigmaContinuator):
    r"""Direct method to construct the auxiliary Green function

    :math:`G_{aux}(z) = (\Sigma(z) - c_0) / c_1`, with :math:`c_0 = \Sigma(i\infty)` and :math:`c_1` the coefficient
    of :math:`1/z` of the high-frequency expansion; :math:`\Sigma(\omega) = G_{aux}(\omega) c_1 + c_0`.  Scalar
    self-energies only.

    The reference takes c_0 and c_1 from TRIQS's ``fit_tail()``; here :func:`fit_tail` fits them (``tail_fraction``,
    ``expansion_order``), unless ``constant_shift`` and ``norm`` are given (scalars, or dicts per block), which skip
    the fit.  The values are kept per block in ``_constant_shift`` and ``_norm``.

    Parameters
    ==========
    S_iw : ArrayGf, (mesh, data) or dict of them
        Self-energy :math:`\Sigma(i\omega_n)` on the real Matsubara frequencies :math:`\omega_n`
    """

    def __init__(self, S_iw, constant_shift=None, norm=None, tail_fraction=0.2, expansion_order=4):
        super(DirectSigmaContinuator, self).__init__()
        self.set_S_iw(S_iw)
        self._norm = {}
        self._tail_fraction = tail_fraction
        self._expansion_order = expansion_order
        self._given = (constant_shift, norm)
        self._calculate_Gaux_iw()

    @staticmethod
    def _per_block(v, name):
        return v[name] if isinstance(v, dict) else v

    def _calculate_Gaux_iw(self):
        out = []
        c_given, n_given = self._given
        for name, s in _blocks(self.S_iw):
            if tuple(s.target_shape) != (1, 1):
                raise NotImplementedError('DirectSigmaContinuator not implemented for matrix-valued Sigma')
            c0, c1 = self._per_block(c_given, name), self._per_block(n_given, name)
            if c0 is None or c1 is None:
                tail = fit_tail(s.mesh, s.data[:, 0, 0], self._tail_fraction, self._expansion_order)
                c0 = tail[0] if c0 is None else c0
                c1 = tail[1] if c1 is None else c1
            self._constant_shift[name] = c0
            self._norm[name] = c1
            out.append((name, ArrayGf(s.mesh, (s.data - c0) / c1)))
        self.Gaux_iw = _unblocks(out, self._BlockGf)

    def _calculate_S_w(self):
        out = []
        for name, g in _blocks(self.Gaux_w):
            if tuple(g.target_shape) != (1, 1):
                raise NotImplementedError('DirectSigmaContinuator not implemented for matrix-valued Sigma')
            out.append((name, ArrayGf(g.mesh, g.data * self._norm[name] + self._constant_shift[name])))
        self.S_w = _unblocks(out, self._BlockGf)
