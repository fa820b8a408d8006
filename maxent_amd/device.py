"""ctypes binding of libmaxent_hip.so (include/maxent_hip.h).

This is the only place where Python crosses into native code.  There is no
CPU fallback: if the shared library is missing or no gfx950 device is
visible, every entry point raises :class:`MaxEntDeviceError`.
"""

import ctypes
import weakref
import os

import numpy as np

_LIB = None
_LIB_PATH = os.environ.get(
    'MAXENT_AMD_LIB',
    os.path.join(os.path.dirname(os.path.abspath(__file__)), 'lib',
                 'libmaxent_hip.so'))

ENTROPY_NORMAL = 0
ENTROPY_PLUSMINUS = 1
PRECISION_F64 = 0
PRECISION_F32 = 1


class MaxEntDeviceError(RuntimeError):
    pass


_MXE_ERR_ARG = -1
_MXE_ERR_LIMIT = -5
_MXE_ERR_NUMERIC = -6
#: most rows of a kernel matrix the device SVD takes: the largest m_rows with svd_lds_bytes(m_rows) <= SVD_LDS_LIMIT
#: (maxent_hip.hip, the one place the formula is written: m_rows + 216 doubles in 60 KB)
SVD_MAX_ROWS = 60 * 1024 // 8 - 216
#: most significant directions (rows of R the pivoted QR keeps, SVD_RCAP of mxe_svd.hip.h) of a matrix the device SVD
#: decomposes; a matrix of higher numerical rank raises MaxEntDeviceError
SVD_MAX_RANK = 128
#: most rows of a group ``mxe_resample_quantiles`` sorts (MXE_QUANTILE_MAX_ROWS of include/maxent_hip.h: 16 columns of them
#: fill 128 KB of the 160 KB of LDS)
QUANTILE_MAX_ROWS = 1024


class MxeOpts(ctypes.Structure):
    """mirror of ``struct mxe_opts`` (include/maxent_hip.h)."""
    _fields_ = [('maxiter', ctypes.c_int32),
                ('miniter', ctypes.c_int32),
                ('tol_h', ctypes.c_double),
                ('tol_d', ctypes.c_double),
                ('tol_relq', ctypes.c_double),
                ('step_max', ctypes.c_double),
                ('mu_first', ctypes.c_double),
                ('mu_grow', ctypes.c_double),
                ('mu_max', ctypes.c_double),
                ('decouple_tol', ctypes.c_double),
                ('waves_per_chain', ctypes.c_int32),
                ('chains_per_wg', ctypes.c_int32),
                ('alpha_split', ctypes.c_int32),
                ('stop_estimate', ctypes.c_int32),
                ('precision', ctypes.c_int32),
                ('wg_per_cu', ctypes.c_int32),
                ('chi2_factor', ctypes.c_double),
                ('lds_basis', ctypes.c_int32),
                ('in_flight', ctypes.c_int32)]


_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_lp = ctypes.POINTER(ctypes.c_int64)
_vp = ctypes.c_void_p

# every symbol include/maxent_hip.h declares: (name, restype, argtypes)
SYMBOLS = [
    ('mxe_version', ctypes.c_char_p, []),
    ('mxe_source_hash', ctypes.c_char_p, []),
    ('mxe_host_alloc', ctypes.c_void_p, [ctypes.c_size_t]),
    ('mxe_host_free', None, [ctypes.c_void_p]),
    ('mxe_strerror', ctypes.c_char_p, [ctypes.c_int]),
    ('mxe_device_count', ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    ('mxe_opts_default', None, [ctypes.POINTER(MxeOpts)]),
    ('mxe_ctx_create', ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_int, _dp, _dp, _dp,
                                      ctypes.POINTER(_vp)]),
    ('mxe_ctx_destroy', None, [_vp]),
    ('mxe_last_hip_error', ctypes.c_char_p, [_vp]),
    ('mxe_dataset_add', ctypes.c_int, [_vp, ctypes.c_int, _dp, _dp,
                                       ctypes.POINTER(ctypes.c_int)]),
    ('mxe_dataset_clear', ctypes.c_int, [_vp]),
    ('mxe_elements_set', ctypes.c_int, [_vp, ctypes.c_int, _ip, _dp, _lp, _dp,
                                        _ip]),
    ('mxe_elements_update_data', ctypes.c_int, [_vp, ctypes.c_int, _dp, _lp]),
    ('mxe_solve_chains', ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _ip,
                                        _dp, _dp, ctypes.POINTER(MxeOpts),
                                        _dp, _dp, _dp, _dp, _dp, _ip, _ip,
                                        _ip]),
    ('mxe_chains_upload', ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _ip,
                                         _dp, _dp, ctypes.POINTER(MxeOpts)]),
    ('mxe_chains_launch', ctypes.c_int, [_vp]),
    ('mxe_sync', ctypes.c_int, [_vp]),
    ('mxe_logdet', ctypes.c_int, [_vp, _dp]),
    ('mxe_chains_fetch_nact', ctypes.c_int, [_vp, _ip]),
    ('mxe_chains_finish', ctypes.c_int, [_vp, _ip]),
    ('mxe_chains_fetch', ctypes.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, _ip, _ip,
                                        _ip]),
    ('mxe_result_device_ptrs', ctypes.c_int, [_vp] + [ctypes.POINTER(_vp)] * 7),
    ('mxe_ns_padded', ctypes.c_int, [_vp]),
    ('mxe_set_result_buffer', ctypes.c_int, [_vp, ctypes.c_int]),
    ('mxe_last_kernel_ms', ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_float)]),
    ('mxe_last_kernel_name', ctypes.c_char_p, [_vp]),
    ('mxe_timing_mark', ctypes.c_int, [_vp]),
    ('mxe_ms_since_mark', ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_float)]),
    ('mxe_stream', ctypes.c_void_p, [_vp]),
    ('mxe_last_launch_info', ctypes.c_int, [_vp] +
     [ctypes.POINTER(ctypes.c_int)] * 3),
    ('mxe_apply_output_map', ctypes.c_int, [_vp, _dp, _dp]),
    ('mxe_launch_depth', ctypes.c_int, [_vp, _ip, _dp]),
    ('mxe_schedule_info', ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    ('mxe_eval_batch', ctypes.c_int, [_vp, ctypes.c_int, _ip, _dp, _dp, ctypes.c_int, ctypes.c_double] + [_dp] * 11),
    ('mxe_posterior_var', ctypes.c_int, [_vp, ctypes.c_int, _ip, _dp, _dp, _ip, ctypes.c_double, ctypes.c_int, _dp, _dp, _dp, _dp,
                                         ctypes.POINTER(ctypes.c_float)]),
    ('mxe_posterior_sample', ctypes.c_int, [_vp, ctypes.c_int, _ip, _dp, _dp, _ip, ctypes.c_double, ctypes.c_int, ctypes.c_uint64,
                                            ctypes.POINTER(ctypes.c_uint64), _dp, _dp, ctypes.POINTER(ctypes.c_float)]),
    ('mxe_fit_diagnostics', ctypes.c_int, [_vp, ctypes.c_int, _ip, _dp, _dp, _ip, ctypes.c_double, ctypes.c_int, _dp, _dp, _dp, _dp,
                                           ctypes.POINTER(ctypes.c_float)]),
    ('mxe_response', ctypes.c_int, [_vp, ctypes.c_int, _ip, _dp, _dp, _ip, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_int, _dp, _dp, ctypes.POINTER(ctypes.c_float)]),
    ('mxe_normals', ctypes.c_int, [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, _dp]),
    ('mxe_entropy', ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _dp, _dp, _dp, _dp]),
    ('mxe_audit', ctypes.c_int, [_vp, _dp, _dp]),
    ('mxe_select_launch', ctypes.c_int, [_vp, ctypes.c_int]),
    ('mxe_select_fetch', ctypes.c_int, [_vp, _ip, _dp]),
    ('mxe_select3_launch', ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double]),
    ('mxe_select3_fetch', ctypes.c_int, [_vp, _ip, _dp]),
    ('mxe_select3_fetch_rows', ctypes.c_int, [_vp, _ip, ctypes.c_int, ctypes.c_int, _dp]),
    ('mxe_select3_prefetch_rows', ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _dp]),
    ('mxe_chains_prefetch', ctypes.c_int, [_vp, _dp, _ip]),
    ('mxe_fetch_rows', ctypes.c_int, [_vp, ctypes.c_int, _ip, _dp]),
    ('mxe_shard_plan', ctypes.c_int, [ctypes.c_int, ctypes.c_int, _ip, _ip, _ip]),
    ('mxe_comm_unique_id', ctypes.c_int, [ctypes.c_char_p]),
    ('mxe_comm_init', ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_char_p]),
    ('mxe_comm_init_local', ctypes.c_int, [ctypes.POINTER(_vp), ctypes.c_int]),
    ('mxe_comm_destroy', ctypes.c_int, [_vp]),
    ('mxe_comm_set_loopback', ctypes.c_int, [_vp, ctypes.c_int]),
    ('mxe_gather', ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _lp, _dp]),
    ('mxe_gather_local', ctypes.c_int, [ctypes.POINTER(_vp), ctypes.c_int, ctypes.c_int, ctypes.c_int, _lp, _dp]),
    ('mxe_comm_allreduce', ctypes.c_int, [_vp, _dp, ctypes.c_int, ctypes.c_int]),
    ('mxe_kernel_svd', ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _dp, _dp,
                                      ctypes.c_double, ctypes.c_int, _dp, ctypes.c_double,
                                      ctypes.c_int, _dp, _dp, _dp, _dp, _ip, _ip,
                                      ctypes.POINTER(ctypes.c_float)]),
    ('mxe_kernel_svd_iw', ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _dp, _dp,
                                         ctypes.c_int, _dp, ctypes.c_double,
                                         ctypes.c_int, _dp, _dp, _dp, _dp, _ip, _ip,
                                         ctypes.POINTER(ctypes.c_float)]),
    ('mxe_kernel_svd_boson', ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _dp, _dp,
                                            ctypes.c_double, ctypes.c_int, ctypes.c_int, _dp, ctypes.c_double,
                                            ctypes.c_int, _dp, _dp, _dp, _dp, _ip, _ip,
                                            ctypes.POINTER(ctypes.c_float)]),
    ('mxe_kernel_svd_boson_iw', ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _dp, _dp,
                                               ctypes.c_int, ctypes.c_int, _dp, ctypes.c_double,
                                               ctypes.c_int, _dp, _dp, _dp, _dp, _ip, _ip,
                                               ctypes.POINTER(ctypes.c_float)]),
    ('mxe_kernel_svd_legendre', ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _dp, _dp,
                                               ctypes.c_double, ctypes.c_int, _dp, ctypes.c_double,
                                               ctypes.c_int, _dp, _dp, _dp, _dp, _ip, _ip,
                                               ctypes.POINTER(ctypes.c_float)]),
    ('mxe_kernel_svd_data', ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _dp, _dp,
                                           ctypes.c_int, _dp, ctypes.c_double,
                                           ctypes.c_int, _dp, _dp, _dp, _dp, _ip, _ip,
                                           ctypes.POINTER(ctypes.c_float)]),
    ('mxe_kramers_kronig', ctypes.c_int, [ctypes.c_int, ctypes.c_int, _dp, _dp, _dp, ctypes.c_int, _dp,
                                          ctypes.c_int, _dp, _dp, ctypes.POINTER(ctypes.c_float)]),
    ('mxe_bins_eig', ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, ctypes.c_double,
                                    _dp, _dp, _dp, _ip, _ip]),
    ('mxe_bins_eig_shrunk', ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, ctypes.c_double,
                                           ctypes.c_double, _dp, _dp, _dp, _ip, _ip, _dp, _dp, _dp,
                                           ctypes.POINTER(ctypes.c_float)]),
    ('mxe_bins_resample', ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, ctypes.c_int, _ip, _dp, _ip,
                                         _dp, _dp, _dp, ctypes.POINTER(ctypes.c_float)]),
    ('mxe_resample_reduce', ctypes.c_int, [_vp, ctypes.c_int, _ip, _dp, _ip, _dp, ctypes.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _ip,
                                           ctypes.POINTER(ctypes.c_float)]),
    ('mxe_resample_quantiles', ctypes.c_int, [_vp, ctypes.c_int, _ip, _dp, _ip, ctypes.c_int, _dp, _dp, _ip,
                                              ctypes.POINTER(ctypes.c_float)]),
    ('mxe_mock_data', ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _dp, _dp, _dp, _ip,
                                     ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), _dp, _dp, ctypes.POINTER(ctypes.c_float)]),
    ('mxe_cv_score', ctypes.c_int, [_vp, ctypes.c_int, _ip, _dp, _ip, ctypes.c_int, ctypes.c_int, _dp, _dp, _ip, _dp, _dp,
                                    _dp, _dp, _ip, ctypes.POINTER(ctypes.c_float)]),
    ('mxe_evidence_reduce', ctypes.c_int, [_vp, ctypes.c_int, _ip, ctypes.c_int, _dp, _ip, _dp, _dp, _dp, _dp, ctypes.c_int, _ip,
                                           ctypes.c_int, _dp, _dp, _ip, _ip, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip,
                                           ctypes.POINTER(ctypes.c_float)]),
    ('mxe_bins_check', ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _dp, _ip,
                                      _dp, _dp, _dp, _dp, _ip, ctypes.POINTER(ctypes.c_float)]),
    ('mxe_hermitian_eig', ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, ctypes.c_double,
                                         _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip, ctypes.POINTER(ctypes.c_float)]),
    ('mxe_fullmatrix_solve', ctypes.c_int, [ctypes.c_int] * 7 + [_dp] * 7 + [ctypes.c_int, ctypes.c_double] + [_dp] * 5 +
                                           [_ip, _ip, ctypes.POINTER(ctypes.c_float)]),
    ('mxe_fullmatrix_solve_metric', ctypes.c_int, [ctypes.c_int] * 7 + [_dp] * 8 + [ctypes.c_int, ctypes.c_double] +
                                                  [_dp] * 5 + [_ip, _ip, ctypes.POINTER(ctypes.c_float)]),
    ('mxe_fullmatrix_posterior_var', ctypes.c_int, [ctypes.c_int] * 7 + [_dp] * 6 + [ctypes.c_int] + [_dp] * 6 +
                                                   [ctypes.POINTER(ctypes.c_float)]),
    ('mxe_fullmatrix_logdet', ctypes.c_int, [ctypes.c_int] * 6 + [_dp] * 5 + [ctypes.c_int, _dp, _dp,
                                                                                ctypes.POINTER(ctypes.c_float)]),
]


def library_path():
    return _LIB_PATH


def load_library():
    """Load libmaxent_hip.so and declare every prototype. Raises if missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_LIB_PATH):
        raise MaxEntDeviceError(
            'HIP library not built: {} is missing. Run '
            '`python -c "import __graft_entry__ as g; g.build()"` or '
            '`make -C maxent_amd/csrc`. There is no CPU fallback.'.format(
                _LIB_PATH))
    lib = ctypes.CDLL(_LIB_PATH)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)      # AttributeError if a symbol is missing
        fn.restype = restype
        fn.argtypes = argtypes
    _LIB = lib
    return lib


def comm_unique_id():
    """128 bytes that rank 0 hands to the other ranks before ``DeviceContext.comm_init`` (ncclGetUniqueId)"""
    lib = load_library()
    buf = ctypes.create_string_buffer(128)
    rc = lib.mxe_comm_unique_id(buf)
    if rc != 0:
        raise MaxEntDeviceError('mxe_comm_unique_id failed: ' + lib.mxe_strerror(rc).decode())
    return buf.raw


def shard_plan(n_elem, n_ranks):
    """``mxe_shard_plan``: (rank of every element, its index inside the rank's shard, shard sizes);
    host arithmetic only, works without a GPU"""
    lib = load_library()
    rk = np.zeros(max(n_elem, 1), dtype=np.int32)
    li = np.zeros(max(n_elem, 1), dtype=np.int32)
    nl = np.zeros(n_ranks, dtype=np.int32)
    rc = lib.mxe_shard_plan(int(n_elem), int(n_ranks), _p(rk), _p(li), _p(nl))
    if rc != 0:
        raise MaxEntDeviceError('mxe_shard_plan failed: ' + lib.mxe_strerror(rc).decode())
    return rk[:n_elem], li[:n_elem], nl


def comm_init_local(contexts):
    """ranks of one process: rank = position in ``contexts`` (``mxe_comm_init_local``)"""
    lib = load_library()
    arr = (_vp * len(contexts))(*[c._h for c in contexts])
    rc = lib.mxe_comm_init_local(arr, len(contexts))
    if rc != 0:
        raise MaxEntDeviceError('mxe_comm_init_local failed: ' + lib.mxe_strerror(rc).decode())


def gather_local(contexts, root, counts, full=False, recv=None):
    lib = load_library()
    arr = (_vp * len(contexts))(*[c._h for c in contexts])
    counts = _c(counts, np.int64)
    rc = lib.mxe_gather_local(arr, len(contexts), int(root), 1 if full else 0, _p(counts), _p(recv))
    if rc != 0:
        msg = lib.mxe_strerror(rc).decode()
        if rc == -2:
            msg += ': ' + lib.mxe_last_hip_error(contexts[root]._h).decode()
        raise MaxEntDeviceError('mxe_gather_local failed: ' + msg)
    return recv


def source_hash():
    """hash of the sources the loaded library was built from (mxe_source_hash)"""
    return load_library().mxe_source_hash().decode()


def device_count():
    lib = load_library()
    n = ctypes.c_int(0)
    lib.mxe_device_count(ctypes.byref(n))
    return n.value


def default_opts(**kw):
    lib = load_library()
    o = MxeOpts()
    lib.mxe_opts_default(ctypes.byref(o))
    for k, val in kw.items():
        if not hasattr(o, k):
            raise TypeError('unknown solver option {!r}'.format(k))
        setattr(o, k, val)
    return o


def pinned_empty(shape, dtype=np.float64, min_bytes=1 << 20):
    """an uninitialised array in page-locked host memory (``mxe_host_alloc``; the block goes back to the library's pool with
    the last view of it) -- the destination of the large device-to-host copies; plain ``np.empty`` for arrays below
    ``min_bytes`` or when the runtime cannot pin that much"""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    if n < min_bytes or n == 0:
        return np.empty(shape, dtype=dtype)
    if n < (1 << 20) + (1 << 21) and _small_pinned[0] + n > SMALL_PINNED_LIMIT:
        return np.empty(shape, dtype=dtype)              # (results a caller keeps hold their blocks: see SMALL_PINNED_LIMIT)
    lib = load_library()
    p = lib.mxe_host_alloc(n)
    if not p:
        return np.empty(shape, dtype=dtype)
    buf = (ctypes.c_char * n).from_address(p)
    weakref.finalize(buf, _host_free, lib, p, n)         # (every view keeps ``buf`` alive through its base)
    if n < (1 << 20) + (1 << 21):
        _small_pinned[0] += n
    return np.frombuffer(buf, dtype=dtype).reshape(shape)


# The scalars and rows of a launch (DeviceContext.result_arrays(pinned_rows=...): ~2 MB per 16 x 16 x 100 job) live in page-locked
# memory as long as the result that holds them; a caller who keeps hundreds of results would pin gigabytes.  Beyond this many
# bytes of such blocks alive, further ones are ordinary memory (and are then copied out when the result is waited for, as before).
SMALL_PINNED_LIMIT = 256 << 20
_small_pinned = [0]


def _host_free(lib, p, n):
    if n < (1 << 20) + (1 << 21):
        _small_pinned[0] -= n
    lib.mxe_host_free(p)


def is_pinned(a):
    """whether ``a`` lies in a block of :func:`pinned_empty`"""
    b = a
    while getattr(b, 'base', None) is not None:
        b = b.base
    return isinstance(b, ctypes.Array)


def _c(a, dtype=np.float64):
    return np.ascontiguousarray(a, dtype=dtype)


def _p(a):
    if a is None:
        return None
    if a.dtype == np.float64:
        return a.ctypes.data_as(_dp)
    if a.dtype == np.int32:
        return a.ctypes.data_as(_ip)
    if a.dtype == np.int64:
        return a.ctypes.data_as(_lp)
    raise TypeError(a.dtype)


def kernel_svd(tau, omega, delta, beta, preblur_b=(0.0,), threshold=1.e-14,
               ns_max=128, want_K=False, device=0):
    """``mxe_kernel_svd``: TauKernel (and PreblurKernel, one per entry of
    ``preblur_b`` > 0) filled and decomposed on the device.  Returns a list of
    dicts ``U, S, V`` (truncated at ``S >= threshold``), ``K`` (if wanted),
    ``qr_rank``, ``sweeps`` and the device time ``ms`` of the whole batch."""
    return _kernel_svd('mxe_kernel_svd', tau, (float(beta),), omega, delta, preblur_b, threshold, ns_max, want_K,
                            device)


def kernel_svd_iw(iomega, omega, delta, preblur_b=(0.0,), threshold=1.e-14, ns_max=128, want_K=False, device=0):
    """``mxe_kernel_svd_iw``: IOmegaKernel (stacked real, 2 n_iw rows) and its PreblurKernels filled and
    decomposed on the device; returns what :func:`kernel_svd` returns.  More rows than the decomposition's LDS
    holds (2 n_iw > ``SVD_MAX_ROWS``) raise :class:`MaxEntDeviceError` -- the host SVD (``svd_backend='host'``) takes them."""
    return _kernel_svd('mxe_kernel_svd_iw', iomega, (), omega, delta, preblur_b, threshold, ns_max, want_K, device,
                            n_rows=2 * len(iomega))


def kernel_svd_boson(tau, omega, delta, beta, symmetric=False, preblur_b=(0.0,), threshold=1.e-14, ns_max=128,
                     want_K=False, device=0):
    """``mxe_kernel_svd_boson``: BosonicTauKernel (``symmetric``: its half-axis form) and its PreblurKernels filled
    and decomposed on the device; returns what :func:`kernel_svd` returns."""
    return _kernel_svd('mxe_kernel_svd_boson', tau, (float(beta), 1 if symmetric else 0), omega, delta, preblur_b,
                            threshold, ns_max, want_K, device)


def kernel_svd_boson_iw(inu, omega, delta, symmetric=False, preblur_b=(0.0,), threshold=1.e-14, ns_max=128,
                        want_K=False, device=0):
    """``mxe_kernel_svd_boson_iw``: BosonicIOmegaKernel -- stacked real of 2 n rows, or with ``symmetric`` the real
    half-axis form of n rows -- and its PreblurKernels filled and decomposed on the device; returns what
    :func:`kernel_svd` returns.  Too many rows for the decomposition's LDS: as :func:`kernel_svd_iw`."""
    return _kernel_svd('mxe_kernel_svd_boson_iw', inu, (1 if symmetric else 0,), omega, delta, preblur_b,
                            threshold, ns_max, want_K, device, n_rows=len(inu) if symmetric else 2 * len(inu))


def kernel_svd_legendre(l, omega, delta, beta, preblur_b=(0.0,), threshold=1.e-14, ns_max=128, want_K=False, device=0):
    """``mxe_kernel_svd_legendre``: LegendreKernel (orders ``l``: non-negative integers in any order) and its
    PreblurKernels filled and decomposed on the device; returns what :func:`kernel_svd` returns.  An order that is
    negative, not an integer or too large, or ``beta`` <= 0, is refused by the library before anything is launched
    (:class:`MaxEntDeviceError`)."""
    return _kernel_svd('mxe_kernel_svd_legendre', l, (float(beta),), omega, delta, preblur_b, threshold, ns_max,
                            want_K, device)


def kernel_svd_data(K, omega, delta, preblur_b=(0.0,), threshold=1.e-14, ns_max=128, want_K=False, device=0):
    """``mxe_kernel_svd_data``: the decomposition (and the preblur products, one per entry of ``preblur_b`` > 0) of a
    matrix the caller filled, ``K`` of shape (n_rows, n_omega); returns what :func:`kernel_svd` returns.  More rows
    than the decomposition's LDS holds (``SVD_MAX_ROWS``) raise :class:`MaxEntDeviceError` -- the host SVD takes them."""
    return _kernel_svd('mxe_kernel_svd_data', K, (), omega, delta, preblur_b, threshold, ns_max, want_K, device)


def _kernel_svd(name, grid, scalar_args, omega, delta, preblur_b=(0.0,), threshold=1.e-14, ns_max=128, want_K=False,
                device=0, n_rows=None):
    """What the ``kernel_svd*`` functions and ``Kernel._device_svd`` share: the C entry ``name`` on the row grid
    ``grid`` (tau, i omega_n, the orders l, or the rows of a caller's matrix, which is checked here) with
    ``scalar_args`` between ``delta`` and ``n_b`` in the entry's order; ``n_rows``: the rows of K where they are not
    ``len(grid)``."""
    load_library()
    if device_count() < 1:
        raise MaxEntDeviceError('no HIP device visible; the device SVD has no CPU fallback')
    grid, omega, delta = _c(grid), _c(omega), _c(delta)
    if name == 'mxe_kernel_svd_data':
        if grid.ndim != 2 or grid.shape[1] != len(omega) or len(delta) != len(omega):
            raise ValueError('kernel_svd_data: K (n_rows, n_omega) = %s on an omega mesh of %d points' % (grid.shape, len(omega)))
        if not np.all(np.isfinite(grid)):
            raise ValueError('kernel_svd_data: K holds %d values that are not finite' % int((~np.isfinite(grid)).sum()))
    return _kernel_svd_call(name, len(grid), (_p(grid),), scalar_args, omega, delta, preblur_b, threshold, ns_max, want_K,
                            device, n_rows)


def _kernel_svd_call(name, n_grid, grid_args, scalar_args, omega, delta, preblur_b, threshold, ns_max, want_K, device,
                     n_rows=None):
    """the C entry itself, on converted arrays, and the mapping of its error codes"""
    lib = load_library()
    bs = _c(np.atleast_1d(np.asarray(preblur_b, dtype=float)))
    n_rows = n_grid if n_rows is None else n_rows      # (rows of K: n_tau, or 2 n_iw)
    n_w, n_b = len(omega), len(bs)
    K = np.empty((n_b, n_rows, n_w)) if want_K else None
    U = np.empty((n_b, n_rows, ns_max))
    S = np.empty((n_b, ns_max))
    V = np.empty((n_b, n_w, ns_max))
    ns = np.zeros(n_b, dtype=np.int32)
    info = np.zeros((n_b, 3), dtype=np.int32)
    ms = ctypes.c_float(0)
    rc = getattr(lib, name)(int(device), n_grid, n_w, *grid_args, _p(omega), _p(delta), *scalar_args,
                            n_b, _p(bs), float(threshold), int(ns_max), _p(K), _p(U), _p(S), _p(V),
                            _p(ns), _p(info), ctypes.byref(ms))
    if rc == _MXE_ERR_LIMIT and n_rows > SVD_MAX_ROWS:
        raise MaxEntDeviceError('%s: %d rows of the kernel exceed the %d the device decomposition holds in LDS; '
                                'svd_backend="host" takes them' % (name, n_rows, SVD_MAX_ROWS))
    if rc == _MXE_ERR_LIMIT and np.any(info[:, 2] == 3):
        raise MaxEntDeviceError('%s: the matrix (%d x %d) has more than %d significant directions (its pivoted QR still '
                                'had columns above eps x the largest after %d steps), and the device decomposition '
                                'keeps no more; svd_backend="host" takes it' % (name, n_rows, n_w, SVD_MAX_RANK, SVD_MAX_RANK))
    if rc != 0:
        raise MaxEntDeviceError(name + ' failed: ' + lib.mxe_strerror(rc).decode())
    out = []
    for ib in range(n_b):
        k = int(ns[ib])
        out.append(dict(U=U[ib, :, :k].copy(), S=S[ib, :k].copy(), V=V[ib, :, :k].copy(),
                        K=(K[ib] if want_K else None), qr_rank=int(info[ib, 0]),
                        sweeps=int(info[ib, 1]), ms=float(ms.value)))
    return out


#: most complex values of G one ``mxe_kramers_kronig`` launch writes (1 GiB of result on the device); more spectra are
#: split into launches of fewer
KK_MAX_VALUES = 1 << 26


def kramers_kronig(w, weight, eta, w_out, A, device=0, max_spectra=None, timing=None):
    """``mxe_kramers_kronig``: ``G[..., o] = sum_j A[..., j] weight[j] / (w_out[o] - w[j] + i eta[j])`` on the device.
    ``A``: real or complex, shape ``(..., n_w)``; returns complex ``(..., n_out)``.  A complex ``A`` goes as two real
    rows (its real and its imaginary part), recombined as ``G(Re A) + i G(Im A)``.  The spectra go in launches of at
    most ``max_spectra`` rows (default: as many as keep a launch's result within ``KK_MAX_VALUES``); the bits of a
    spectrum's G do not depend on the launch it is in.  ``timing``: a dict that receives the device time ``ms`` of the
    sums (all launches) and the number of ``launches``."""
    lib = load_library()
    if device_count() < 1:
        raise MaxEntDeviceError('no HIP device visible; the Kramers-Kronig transform has no CPU fallback')
    w, weight, eta, w_out = (_c(np.ravel(a)) for a in (w, weight, eta, w_out))
    A = np.asarray(A)
    n_w, n_out = len(w), len(w_out)
    if A.ndim < 1 or A.shape[-1] != n_w or len(weight) != n_w or len(eta) != n_w or n_out < 1 or n_w < 1:
        raise ValueError('kramers_kronig: A (..., n_w) = %s, weight and eta of n_w = %d values, w_out not empty'
                         % (A.shape, n_w))
    lead = A.shape[:-1]
    is_complex = np.iscomplexobj(A)
    rows = A.reshape(-1, n_w)
    rows = _c(np.stack([rows.real, rows.imag], axis=1).reshape(-1, n_w)) if is_complex else _c(rows)
    cap = max(1, min(KK_MAX_VALUES // n_out, (2 ** 31 - 1) // max(n_out, n_w)))
    if max_spectra is not None:
        cap = max(1, min(cap, int(max_spectra)))
    G = np.empty((rows.shape[0], n_out), dtype=complex)
    ms_total, launches = 0.0, 0
    for r0 in range(0, rows.shape[0], cap):
        part = rows[r0:r0 + cap]
        out = G[r0:r0 + len(part)]            # (a C-contiguous slice of rows: the library writes it in place)
        ms = ctypes.c_float(0)
        rc = lib.mxe_kramers_kronig(int(device), n_w, _p(w), _p(weight), _p(eta), n_out, _p(w_out), len(part),
                                    _p(part), out.ctypes.data_as(_dp), ctypes.byref(ms))
        if rc != 0:
            raise MaxEntDeviceError('mxe_kramers_kronig failed: ' + lib.mxe_strerror(rc).decode())
        ms_total += float(ms.value)
        launches += 1
    if timing is not None:
        timing['ms'] = ms_total
        timing['launches'] = launches
    if is_complex:
        G = G[0::2] + 1j * G[1::2]
    return G.reshape(lead + (n_out,))


#: most data points of a set ``mxe_bins_eig`` takes (``BINS_NMAX``)
BINS_MAX_DATA = 512


def bins_keep(var, threshold, n_bins, n_data):
    """The selection rule of ``mxe_bins_eig`` on a spectrum ``var`` of covariance eigenvalues: kept are those
    ``>= threshold`` and ``> (max(n_bins, n_data) eps)^2 max(var)`` -- the second bound is the noise floor of a
    singular value of the centred bins, which separates a null direction from a small eigenvalue.  Returns a mask."""
    var = np.asarray(var, dtype=float)
    if var.size == 0:
        return np.zeros(0, dtype=bool)
    floor = (max(int(n_bins), int(n_data)) * np.finfo(float).eps) ** 2
    return (var >= threshold) & (var > floor * var.max()) & (var > 0.0)


def bins_eig(bins, threshold, device=0):
    """``mxe_bins_eig``: ``bins`` of shape (n_sets, n_bins, n_data) or (n_bins, n_data) -- independent estimates of
    the data -- into the mean over the bins and the eigenbasis of the covariance of that mean, every set in one launch.
    Returns one dict per set (one dict for 2-d ``bins``): ``mean`` (n_data), ``sigma`` (the square roots of the kept
    eigenvalues, ascending), ``T`` (rank x n_data, row k the eigenvector of ``sigma[k]``), ``rank``, ``sweeps`` (Jacobi
    sweeps taken)."""
    lib = load_library()
    b = np.asarray(bins)
    single = b.ndim == 2
    if single:
        b = b[None]
    if b.ndim != 3 or np.iscomplexobj(b):
        raise ValueError('bins_eig: bins must be real, (n_sets, n_bins, n_data) or (n_bins, n_data); got %s' % (np.shape(bins),))
    b = _c(b)
    n_sets, n_bins, n_data = b.shape
    if n_sets < 1 or n_bins < 2:
        raise ValueError('bins_eig: at least one set and two bins are needed; got %d set(s) of %d bin(s)' % (n_sets, n_bins))
    if n_data < 1 or n_data > BINS_MAX_DATA:
        raise MaxEntDeviceError('mxe_bins_eig: %d data points per set; the device decomposition takes 1 to %d'
                                % (n_data, BINS_MAX_DATA))
    if device_count() < 1:
        raise MaxEntDeviceError('no HIP device visible; the covariance eigenbasis of bins has no CPU fallback')
    mean = np.empty((n_sets, n_data))
    var = np.empty((n_sets, n_data))
    T = np.empty((n_sets, n_data, n_data))
    rank = np.zeros(n_sets, dtype=np.int32)
    sweeps = np.zeros(n_sets, dtype=np.int32)
    rc = lib.mxe_bins_eig(int(device), n_sets, n_bins, n_data, _p(b), float(threshold), _p(mean), _p(var), _p(T),
                          _p(rank), _p(sweeps))
    if rc == _MXE_ERR_NUMERIC:
        raise MaxEntDeviceError('mxe_bins_eig: the Jacobi iteration of set(s) %s did not converge (sweeps %s), or the '
                                'squares of the bins overflow' % (np.nonzero(sweeps >= 60)[0].tolist(), int(sweeps.max())))
    if rc == _MXE_ERR_ARG:           # (sizes were checked above: what the library refuses here is a NaN or an Inf, before any launch)
        raise ValueError('bins_eig: bins hold %d values that are not finite' % int((~np.isfinite(b)).sum()))
    if rc != 0:
        raise MaxEntDeviceError('mxe_bins_eig failed: ' + lib.mxe_strerror(rc).decode())
    out = []
    for s in range(n_sets):
        k = int(rank[s])
        out.append(dict(mean=mean[s].copy(), sigma=np.sqrt(var[s, :k]), T=T[s, :k].copy(), rank=k, sweeps=int(sweeps[s])))
    return out[0] if single else out


def shrinkage_argument(shrinkage, n_bins):
    """The ``shrinkage`` argument of the bins setters as ``lambda_in`` of ``mxe_bins_eig_shrunk``: None for ``None`` and
    ``0.0`` (the sample covariance, ``mxe_bins_eig``), -1.0 for ``'auto'`` (the intensity is estimated from the bins, which
    takes four of them), the value itself for a number in (0, 1].  Anything else is a ValueError; nothing is touched."""
    if shrinkage is None:
        return None
    if isinstance(shrinkage, str):
        if shrinkage != 'auto':
            raise ValueError("shrinkage must be None, 'auto' or a number in [0, 1]; got %r" % (shrinkage,))
        if int(n_bins) < 4:
            raise ValueError("shrinkage='auto' estimates the variance of every correlation and needs at least 4 bins; "
                             "got %d" % int(n_bins))
        return -1.0
    if isinstance(shrinkage, (bool, np.bool_)) or not isinstance(shrinkage, (int, float, np.integer, np.floating)):
        raise ValueError("shrinkage must be None, 'auto' or a number in [0, 1]; got %r" % (shrinkage,))
    lam = float(shrinkage)
    if not (0.0 <= lam <= 1.0):
        raise ValueError("shrinkage must be None, 'auto' or a number in [0, 1]; got %r" % (shrinkage,))
    return None if lam == 0.0 else lam


def bins_eig_shrunk(bins, threshold, shrinkage, device=0, timing=None):
    """``mxe_bins_eig_shrunk``: :func:`bins_eig` with the shrinkage covariance of the mean
    C* = (1 - lambda) X^T X + lambda diag(c) in place of X^T X.  ``shrinkage``: ``'auto'`` (lambda* is estimated per set
    from its bins) or a number in [0, 1] (that lambda for every set).  Returns the dicts of :func:`bins_eig` with three
    more entries: ``shrinkage`` (the lambda used), ``shrinkage_raw`` (the unclipped estimate; NaN for a fixed lambda and
    where no two columns are correlated at all) and ``variance`` (n_data: c_j, the variances of the mean, the diagonal
    of both C and C*).  ``timing``: a dict that receives the device time ``ms`` of the call's kernels."""
    lib = load_library()
    b = np.asarray(bins)
    single = b.ndim == 2
    if single:
        b = b[None]
    if b.ndim != 3 or np.iscomplexobj(b):
        raise ValueError('bins_eig_shrunk: bins must be real, (n_sets, n_bins, n_data) or (n_bins, n_data); got %s' % (np.shape(bins),))
    b = _c(b)
    n_sets, n_bins, n_data = b.shape
    if n_sets < 1 or n_bins < 2:
        raise ValueError('bins_eig_shrunk: at least one set and two bins are needed; got %d set(s) of %d bin(s)' % (n_sets, n_bins))
    lam_in = shrinkage_argument(shrinkage, n_bins)
    if lam_in is None:
        if shrinkage is None:
            raise ValueError("bins_eig_shrunk: shrinkage must be 'auto' or a number in [0, 1]; bins_eig is the call without")
        lam_in = 0.0
    if n_data < 1 or n_data > BINS_MAX_DATA:
        raise MaxEntDeviceError('mxe_bins_eig_shrunk: %d data points per set; the device decomposition takes 1 to %d'
                                % (n_data, BINS_MAX_DATA))
    if device_count() < 1:
        raise MaxEntDeviceError('no HIP device visible; the shrinkage covariance of bins has no CPU fallback')
    mean = np.empty((n_sets, n_data))
    var = np.empty((n_sets, n_data))
    T = np.empty((n_sets, n_data, n_data))
    rank = np.zeros(n_sets, dtype=np.int32)
    sweeps = np.zeros(n_sets, dtype=np.int32)
    lam = np.empty(n_sets)
    raw = np.empty(n_sets)
    diag = np.empty((n_sets, n_data))
    ms = ctypes.c_float(0)
    rc = lib.mxe_bins_eig_shrunk(int(device), n_sets, n_bins, n_data, _p(b), float(threshold), float(lam_in), _p(mean), _p(var),
                                 _p(T), _p(rank), _p(sweeps), _p(lam), _p(raw), _p(diag), ctypes.byref(ms))
    if rc == _MXE_ERR_NUMERIC:
        raise MaxEntDeviceError('mxe_bins_eig_shrunk: the Jacobi iteration of set(s) %s did not converge (sweeps %s), or the '
                                'squares of the bins overflow' % (np.nonzero(sweeps >= 60)[0].tolist(), int(sweeps.max())))
    if rc == _MXE_ERR_ARG:           # (sizes and lambda were checked above: what is left is a NaN or an Inf, or a bad threshold)
        raise ValueError('bins_eig_shrunk: bins hold %d values that are not finite (threshold %r)'
                         % (int((~np.isfinite(b)).sum()), threshold))
    if rc != 0:
        raise MaxEntDeviceError('mxe_bins_eig_shrunk failed: ' + lib.mxe_strerror(rc).decode())
    if timing is not None:
        timing['ms'] = float(ms.value)
    out = []
    for s in range(n_sets):
        k = int(rank[s])
        out.append(dict(mean=mean[s].copy(), sigma=np.sqrt(var[s, :k]), T=T[s, :k].copy(), rank=k, sweeps=int(sweeps[s]),
                        shrinkage=float(lam[s]), shrinkage_raw=float(raw[s]), variance=diag[s].copy()))
    return out[0] if single else out


def bins_resample(bins, counts, T, rank, device=0, want_dev=True, timing=None):
    """``mxe_bins_resample``: the rotated data of every resample of every set, one launch.  ``bins``: (n_sets, n_bins,
    n_data) or (n_bins, n_data); ``counts``: (n_res, n_bins) multiplicities, one table for all sets; ``T``: (n_sets, n_data,
    n_data) eigenvector rows as ``mxe_bins_eig`` writes them (zero rows behind the kept ones), ``rank``: (n_sets,).  Returns
    a dict: ``mean`` (n_sets, n_data) -- the bits of ``bins_eig`` --, ``G`` (n_sets, n_res, n_data) = T mean + dev, ``dev``
    (the rotated deviations of the resampled means, with ``want_dev``); rows k >= rank are zeros.  2-d ``bins``: without
    the leading axis.  ``timing``: a dict that receives the device time ``ms`` of the kernel."""
    lib = load_library()
    b = np.asarray(bins)
    single = b.ndim == 2
    if single:
        b = b[None]
    if b.ndim != 3 or np.iscomplexobj(b):
        raise ValueError('bins_resample: bins must be real, (n_sets, n_bins, n_data) or (n_bins, n_data); got %s' % (np.shape(bins),))
    b = _c(b)
    n_sets, n_bins, n_data = b.shape
    cnt = np.asarray(counts)
    if cnt.ndim != 2 or cnt.shape[1] != n_bins or cnt.shape[0] < 1 or cnt.dtype.kind not in 'iu':
        raise ValueError('bins_resample: counts must be integers of shape (n_res >= 1, n_bins = %d); got %s %s'
                         % (n_bins, cnt.dtype, cnt.shape))
    cnt = _c(cnt, np.int32)
    n_res = cnt.shape[0]
    Tm = _c(np.asarray(T, dtype=float).reshape(n_sets, n_data, n_data))
    rk = _c(np.asarray(rank).reshape(n_sets), np.int32)
    if device_count() < 1:
        raise MaxEntDeviceError('no HIP device visible; the resampling of bins has no CPU fallback')
    mean = np.empty((n_sets, n_data))
    G = np.empty((n_sets, n_res, n_data))
    dev = np.empty((n_sets, n_res, n_data)) if want_dev else None
    ms = ctypes.c_float(0)
    rc = lib.mxe_bins_resample(int(device), n_sets, n_bins, n_data, _p(b), n_res, _p(cnt), _p(Tm), _p(rk), _p(mean), _p(G),
                               _p(dev), ctypes.byref(ms))
    if rc == _MXE_ERR_ARG:
        raise ValueError('mxe_bins_resample refused its arguments: %d set(s) of %d bins x %d values (2 bins and 1 to %d values are '
                         'needed), %d resample(s), counts that are negative or a row of them that sums to 0, a rank outside '
                         '0..n_data, or values of bins or T that are not finite' % (n_sets, n_bins, n_data, BINS_MAX_DATA, n_res))
    if rc != 0:
        raise MaxEntDeviceError('mxe_bins_resample failed: ' + lib.mxe_strerror(rc).decode())
    if timing is not None:
        timing['ms'] = float(ms.value)
    out = dict(mean=mean, G=G)
    if want_dev:
        out['dev'] = dev
    if single:
        out = dict((k, v[0]) for k, v in out.items())
    return out


def bins_check(bins, T=None, rank=None, device=0, timing=None):
    """``mxe_bins_check``: the blocking ladder and the normality of the block means of every set, one launch.  ``bins``:
    (n_sets, n_bins, n_data) or (n_bins, n_data), the bin index being Monte Carlo time; ``T`` (n_sets, n_data, n_data) and
    ``rank`` (n_sets,): the eigenvector rows as ``mxe_bins_eig`` writes them (zero rows behind the kept ones) -- the columns
    are then the eigen-directions --, or both None: the columns are the data values.  Returns a dict: ``mean`` (n_sets,
    n_data) -- the bits of ``bins_eig`` --, ``err2``, ``skew``, ``kurt`` (n_sets, L, n_data) with L = floor(log2 n_bins)
    levels of block length 2^k, ``levels`` = L.  2-d ``bins``: without the leading axis.  ``timing``: a dict that receives
    the device time ``ms`` of the kernel.  Sizes and arguments the library would refuse raise ValueError before it is
    called."""
    b = np.asarray(bins)
    single = b.ndim == 2
    if single:
        b = b[None]
    if b.ndim != 3 or np.iscomplexobj(b):
        raise ValueError('bins_check: bins must be real, (n_sets, n_bins, n_data) or (n_bins, n_data); got %s' % (np.shape(bins),))
    n_sets, n_bins, n_data = b.shape
    if n_sets < 1 or n_bins < 2 or n_data < 1 or n_data > BINS_MAX_DATA or n_bins * n_data > 2 ** 31 - 1:
        raise ValueError('bins_check: %d set(s) of %d bins x %d values; at least one set, two bins and 1 to %d values are '
                         'needed, and at most 2^31 - 1 values per set' % (n_sets, n_bins, n_data, BINS_MAX_DATA))
    if (T is None) != (rank is None):
        raise ValueError('bins_check: T and rank come together (the eigen basis) or not at all (the data basis)')
    Tm = rk = None
    if T is not None:
        Tm = np.asarray(T, dtype=float)
        rk = np.asarray(rank)
        if Tm.size != n_sets * n_data * n_data or rk.size != n_sets:
            raise ValueError('bins_check: T of shape %s and rank of shape %s do not fit %d set(s) of %d values'
                             % (Tm.shape, rk.shape, n_sets, n_data))
        Tm = _c(Tm.reshape(n_sets, n_data, n_data))
        rk = _c(rk.reshape(n_sets), np.int32)
        if np.any(rk < 0) or np.any(rk > n_data):
            raise ValueError('bins_check: a rank outside 0..%d' % n_data)
    b = _c(b)
    lib = load_library()
    if device_count() < 1:
        raise MaxEntDeviceError('no HIP device visible; the checks of the bins have no CPU fallback')
    L = int(n_bins).bit_length() - 1
    mean = np.empty((n_sets, n_data))
    err2, skew, kurt = (np.empty((n_sets, L, n_data)) for _ in range(3))
    levels = np.zeros(1, dtype=np.int32)
    ms = ctypes.c_float(0)
    rc = lib.mxe_bins_check(int(device), n_sets, n_bins, n_data, _p(b), _p(Tm), _p(rk), _p(mean), _p(err2), _p(skew),
                            _p(kurt), _p(levels), ctypes.byref(ms))
    if rc == _MXE_ERR_ARG:           # (sizes, T and rank were checked above: what is left is a NaN or an Inf, before any launch)
        raise ValueError('mxe_bins_check refused its arguments: values of bins or T that are not finite (%d in bins)'
                         % int((~np.isfinite(b)).sum()))
    if rc != 0:
        raise MaxEntDeviceError('mxe_bins_check failed: ' + lib.mxe_strerror(rc).decode())
    if int(levels[0]) != L:
        raise MaxEntDeviceError('mxe_bins_check: %d levels came back where %d were expected' % (int(levels[0]), L))
    if timing is not None:
        timing['ms'] = float(ms.value)
    out = dict(mean=mean, err2=err2, skew=skew, kurt=kurt)
    if single:
        out = dict((k, v[0]) for k, v in out.items())
    out['levels'] = L
    return out


def entropy(kind, H, D, device=0):
    """``mxe_entropy``: S, dS/dH and diag(d2S/dH2) of hidden images given directly; ``H``: (P, n) or (n,)."""
    lib = load_library()
    if device_count() < 1:
        raise MaxEntDeviceError('no HIP device visible; the entropy functions have no CPU fallback')
    H2 = _c(np.atleast_2d(H))
    D = _c(D)
    P, n = H2.shape
    S, dS, ddS = np.empty(P), np.empty((P, n)), np.empty((P, n))
    rc = lib.mxe_entropy(int(device), int(kind), n, P, _p(H2), _p(D), _p(S), _p(dS), _p(ddS))
    if rc != 0:
        raise MaxEntDeviceError('mxe_entropy failed: ' + lib.mxe_strerror(rc).decode())
    if np.ndim(H) == 1:
        return S[0], dS[0], ddS[0]
    return S, dS, ddS


def normals(seed, stream, n_samples, n, device=0):
    """``mxe_normals``: the standard normals (n_samples, n) of the stream ``(seed, stream)``, by the device function
    ``mxe_posterior_sample`` draws with; :func:`maxent_amd.posterior.sample_normals` is the host mirror."""
    lib = load_library()
    if device_count() < 1:
        raise MaxEntDeviceError('no HIP device visible; mxe_normals has no CPU fallback (posterior.sample_normals is the host mirror)')
    if int(n_samples) < 1 or int(n) < 1:
        raise ValueError('normals: n_samples and n must be at least 1')
    z = np.empty((int(n_samples), int(n)))
    rc = lib.mxe_normals(int(device), int(seed) & (2 ** 64 - 1), int(stream) & (2 ** 64 - 1), int(n_samples), int(n), _p(z))
    if rc != 0:
        raise MaxEntDeviceError('mxe_normals failed: ' + lib.mxe_strerror(rc).decode())
    return z


def mock_data(K, H0, err, seed, streams, n_mock, T=None, rank=None, device=0, timing=None):
    """``mxe_mock_data``: mock data drawn from hidden images with the noise of a job, all sets in one launch.  ``K``:
    (n_data, n_omega), the job's kernel as the job has it; ``H0``: (n_sets, n_omega) or (n_omega,); ``err``: (n_sets,
    n_data) error bars (> 0); ``streams``: (n_sets,) stream ids of the generator of :func:`normals`; ``T`` (n_sets, n_data,
    n_data) and ``rank`` (n_sets,): a rotation per set applied to K H0 (zero rows behind the kept ones), or both None.
    Returns a dict: ``model`` (n_sets, n_data) = (T) K H0, ``G`` (n_sets, n_mock, n_data) = model + err z with z the
    normals ``(seed, streams[s])`` -- :func:`maxent_amd.mock.mock_rows` is the host mirror --; rows >= rank are zeros.
    1-d ``H0``: without the leading axis.  ``timing``: a dict that receives the device time ``ms`` of the kernel.
    Arguments the library would refuse raise ValueError before anything is launched."""
    Km = np.asarray(K)
    H = np.asarray(H0)
    single = H.ndim == 1
    if single:
        H = H[None]
    if Km.ndim != 2 or H.ndim != 2 or np.iscomplexobj(Km) or np.iscomplexobj(H) or H.shape[1] != Km.shape[1]:
        raise ValueError('mock_data: K must be real (n_data, n_omega) and H0 real (n_sets, n_omega); got %s and %s'
                         % (np.shape(K), np.shape(H0)))
    Km, H = _c(Km), _c(H)
    n_data, n_omega = Km.shape
    n_sets = H.shape[0]
    n_mock = int(n_mock)
    e = np.asarray(err, dtype=float)
    if e.size != n_sets * n_data:
        raise ValueError('mock_data: err of shape %s does not fit %d set(s) of %d values' % (e.shape, n_sets, n_data))
    e = _c(e.reshape(n_sets, n_data))
    st = np.ascontiguousarray([int(s) & (2 ** 64 - 1) for s in np.atleast_1d(streams)], dtype=np.uint64)
    if st.shape != (n_sets,):
        raise ValueError('mock_data: %d stream(s) for %d set(s)' % (st.size, n_sets))
    if n_sets < 1 or n_data < 1 or n_omega < 1 or n_mock < 1:
        raise ValueError('mock_data: %d set(s), %d mock(s), %d data values, %d omega points; at least one of each is needed'
                         % (n_sets, n_mock, n_data, n_omega))
    if (T is None) != (rank is None):
        raise ValueError('mock_data: T and rank come together or not at all')
    Tm = rk = None
    if T is not None:
        Tm = np.asarray(T, dtype=float)
        rk = np.asarray(rank)
        if Tm.size != n_sets * n_data * n_data or rk.size != n_sets:
            raise ValueError('mock_data: T of shape %s and rank of shape %s do not fit %d set(s) of %d values'
                             % (Tm.shape, rk.shape, n_sets, n_data))
        Tm = _c(Tm.reshape(n_sets, n_data, n_data))
        rk = _c(rk.reshape(n_sets), np.int32)
        if np.any(rk < 0) or np.any(rk > n_data):
            raise ValueError('mock_data: a rank outside 0..%d' % n_data)
    bad = [name for name, a in (('K', Km), ('H0', H), ('err', e), ('T', Tm)) if a is not None and not np.all(np.isfinite(a))]
    if bad:
        raise ValueError('mock_data: values that are not finite in ' + ', '.join(bad))
    if not np.all(e > 0.0):
        raise ValueError('mock_data: every error bar must be positive')
    lib = load_library()
    if device_count() < 1:
        raise MaxEntDeviceError('no HIP device visible; mxe_mock_data has no CPU fallback (mock.mock_rows is the host mirror)')
    model = np.empty((n_sets, n_data))
    G = np.empty((n_sets, n_mock, n_data))
    ms = ctypes.c_float(0)
    rc = lib.mxe_mock_data(int(device), n_sets, n_mock, n_data, n_omega, _p(Km), _p(H), _p(e), _p(Tm), _p(rk),
                           int(seed) & (2 ** 64 - 1), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), _p(model), _p(G),
                           ctypes.byref(ms))
    if rc == _MXE_ERR_ARG:
        raise ValueError('mxe_mock_data refused its arguments: sizes whose products exceed 2^31 - 1 (%d sets x %d mocks x %d '
                         'values, %d omega points)' % (n_sets, n_mock, n_data, n_omega))
    if rc != 0:
        raise MaxEntDeviceError('mxe_mock_data failed: ' + lib.mxe_strerror(rc).decode())
    if timing is not None:
        timing['ms'] = float(ms.value)
    out = dict(model=model, G=G)
    if single:
        out = dict((k, v[0]) for k, v in out.items())
    return out


#: largest matrix ``mxe_hermitian_eig`` takes (MXE_HERMEIG_MAX_M of include/maxent_hip.h)
HERMEIG_MAX_M = 64
#: sweeps after which ``mxe_hermitian_eig`` gives a matrix up (info -2)
HERMEIG_MAX_SWEEPS = 30
HERMEIG_WANT = ('lambda', 'vec', 'proj', 'neg', 'dist', 'pair', 'asym')


def hermitian_eig(A, floor=0.0, want=HERMEIG_WANT, device=0, timing=None):
    """``mxe_hermitian_eig``: the eigen-decomposition of the Hermitian part of every matrix of a batch, one launch.  ``A``:
    (n_mat, m, m) or (m, m), real or complex, m <= ``HERMEIG_MAX_M``; it need not be Hermitian, the device works on
    (A + A^H) / 2.  Returns a dict with the entries named in ``want`` -- ``lambda`` (n_mat, m) ascending, ``vec`` (n_mat, m,
    m), column k the eigenvector of ``lambda[k]`` (unit norm, the component of largest magnitude real and positive),
    ``proj`` (n_mat, m, m) = V max(Lambda, floor) V^H, exactly Hermitian, ``neg`` = sum over lambda < floor of (floor -
    lambda), ``dist`` = || proj - Herm(A) ||_F, ``pair`` = max_{i<j} |a_ij| - sqrt(max(a_ii, 0) max(a_jj, 0)), ``asym`` =
    || A - A^H ||_F -- and always ``info`` (n_mat,) int32: the sweeps that rotated, -1 for a matrix that is not finite (all
    its outputs are NaN), -2 when ``HERMEIG_MAX_SWEEPS`` sweeps did not end the iteration.  ``vec`` and ``proj`` are
    complex when ``A`` is.  2-d ``A``: without the leading axis.  ``timing``: a dict that receives the device time ``ms``
    of the kernel.  Arguments the library would refuse raise ValueError before it is called."""
    a = np.asarray(A)
    single = a.ndim == 2
    if single:
        a = a[None]
    if a.ndim != 3 or a.shape[1] != a.shape[2] or a.dtype.kind not in 'biufc':
        raise ValueError('hermitian_eig: A must be numeric, (n_mat, m, m) or (m, m); got %s' % (np.shape(A),))
    n_mat, m = a.shape[0], a.shape[1]
    if n_mat < 1 or m < 1:
        raise ValueError('hermitian_eig: %d matrices of %d x %d; at least one matrix of one element is needed' % (n_mat, m, m))
    if m > HERMEIG_MAX_M:
        raise ValueError('hermitian_eig: matrices of %d x %d; at most %d x %d fit the LDS' % (m, m, HERMEIG_MAX_M, HERMEIG_MAX_M))
    cplx = np.iscomplexobj(a)
    if n_mat * m * m * (2 if cplx else 1) > 2 ** 31 - 1:
        raise ValueError('hermitian_eig: %d matrices of %d x %d hold more than 2^31 - 1 numbers' % (n_mat, m, m))
    try:
        floor = float(floor)
    except (TypeError, ValueError):
        raise ValueError('hermitian_eig: floor must be a real number; got %r' % (floor,))
    if not np.isfinite(floor):
        raise ValueError('hermitian_eig: floor must be finite; got %r' % (floor,))
    want = (want,) if isinstance(want, str) else tuple(want)
    unknown = [w for w in want if w not in HERMEIG_WANT]
    if unknown:
        raise ValueError('hermitian_eig: want names %r; known are %s' % (unknown, ', '.join(HERMEIG_WANT)))
    a = _c(a, np.complex128 if cplx else np.float64)
    lib = load_library()
    if device_count() < 1:
        raise MaxEntDeviceError('no HIP device visible; mxe_hermitian_eig has no CPU fallback')
    mat_dtype = np.complex128 if cplx else np.float64
    shapes = dict((('lambda', ((n_mat, m), np.float64)), ('vec', ((n_mat, m, m), mat_dtype)), ('proj', ((n_mat, m, m), mat_dtype)),
                   ('neg', ((n_mat,), np.float64)), ('dist', ((n_mat,), np.float64)), ('pair', ((n_mat,), np.float64)),
                   ('asym', ((n_mat,), np.float64))))
    out = dict((w, np.empty(*shapes[w])) for w in want)
    info = np.empty(n_mat, dtype=np.int32)
    ptr = lambda x: None if x is None else x.ctypes.data_as(_dp)
    ms = ctypes.c_float(0)
    rc = lib.mxe_hermitian_eig(int(device), n_mat, m, 1 if cplx else 0, ptr(a), floor,
                               *([ptr(out.get(w)) for w in HERMEIG_WANT] + [_p(info), ctypes.byref(ms)]))
    if rc != 0:
        raise MaxEntDeviceError('mxe_hermitian_eig failed: ' + lib.mxe_strerror(rc).decode())
    if timing is not None:
        timing['ms'] = float(ms.value)
    out['info'] = info
    if single:
        out = dict((k, v[0]) for k, v in out.items())
    return out


#: largest matrix and singular space ``mxe_fullmatrix_solve`` takes (MXE_FULLMATRIX_MAX_M, MXE_FULLMATRIX_MAX_NS)
FULLMATRIX_MAX_M = 4
FULLMATRIX_MAX_NS = 64


def fullmatrix_P(m, use_complex):
    """the number of basis matrices E_p of the Hermitian m x m matrices: m^2, or m (m + 1) / 2 for real symmetric ones"""
    return m * m if use_complex else m * (m + 1) // 2


def fullmatrix_solve(V, c, D, alpha, ghat, cperp, m, use_complex, u0=None, maxiter=1000, tol_h=1e-9, device=0, timing=None):
    """``mxe_fullmatrix_solve``: the whole-matrix continuation of a batch of problems that share ``V`` (n_omega, n_s),
    ``c`` (n_s,), ``D`` (n_omega,) and the scaled ``alpha`` mesh (n_alpha,); ``ghat`` (n_prob, P, n_s) and ``cperp``
    (n_prob,) are the data of every problem in the coordinates of the basis E_p (include/maxent_hip.h), ``u0`` the start
    (zeros by default).  Returns a dict: ``u`` (n_prob, n_alpha, P, n_s), ``H`` (n_prob, m, m, n_alpha, n_omega) -- complex
    with ``use_complex`` --, ``chi2``, ``S``, ``Q`` (n_prob, n_alpha), ``n_iter`` (int32), ``converged`` (bool).
    ``timing``: a dict that receives the device time ``ms`` of the kernel.  Arguments the library would refuse raise
    ValueError before it is called."""
    V, c, D, alpha = _c(V), _c(c), _c(D), _c(alpha)
    ghat, cperp = _c(ghat), _c(cperp)
    m, use_complex = int(m), bool(use_complex)
    if m < 1 or m > FULLMATRIX_MAX_M:
        raise ValueError('fullmatrix_solve: matrices of %d x %d; 1 to %d are supported' % (m, m, FULLMATRIX_MAX_M))
    if V.ndim != 2 or V.shape[0] < 1 or V.shape[1] < 1:
        raise ValueError('fullmatrix_solve: V must be (n_omega, n_s); got %s' % (V.shape,))
    n_omega, n_s = V.shape
    if n_s > FULLMATRIX_MAX_NS:
        raise ValueError('fullmatrix_solve: %d singular values; at most %d are supported: cut the singular space with '
                         'reduce_singular_space' % (n_s, FULLMATRIX_MAX_NS))
    P = fullmatrix_P(m, use_complex)
    if c.shape != (n_s,) or D.shape != (n_omega,) or alpha.ndim != 1 or alpha.size < 1:
        raise ValueError('fullmatrix_solve: c must be (n_s,), D (n_omega,), alpha one-dimensional and not empty')
    if ghat.ndim != 3 or ghat.shape[0] < 1 or ghat.shape[1:] != (P, n_s) or cperp.shape != (ghat.shape[0],):
        raise ValueError('fullmatrix_solve: ghat must be (n_prob, %d, %d) and cperp (n_prob,); got %s and %s'
                         % (P, n_s, ghat.shape, cperp.shape))
    n_prob, n_alpha = ghat.shape[0], alpha.size
    if u0 is not None:
        u0 = _c(u0)
        if u0.shape != ghat.shape:
            raise ValueError('fullmatrix_solve: u0 must have the shape of ghat, %s; got %s' % (ghat.shape, u0.shape))
    for name, a in (('V', V), ('c', c), ('D', D), ('alpha', alpha), ('ghat', ghat), ('cperp', cperp), ('u0', u0)):
        if a is not None and not np.all(np.isfinite(a)):
            raise ValueError('fullmatrix_solve: %s is not finite' % name)
    if not (np.all(c > 0) and np.all(D > 0) and np.all(alpha > 0)):
        raise ValueError('fullmatrix_solve: c, D and alpha must be positive')
    maxiter, tol_h = int(maxiter), float(tol_h)
    if maxiter < 0 or not (tol_h > 0 and np.isfinite(tol_h)):
        raise ValueError('fullmatrix_solve: maxiter must be >= 0 and tol_h positive and finite')
    planes = 2 if use_complex else 1
    if max(n_prob * n_alpha * planes * m * m * n_omega, n_prob * n_alpha * P * n_s, n_omega * n_s,
           P * (P + 1) // 2 * n_omega) > 2 ** 31 - 1:
        raise ValueError('fullmatrix_solve: the arrays of this call hold more than 2^31 - 1 numbers')
    lib = load_library()
    if device_count() < 1:
        raise MaxEntDeviceError('no HIP device visible; mxe_fullmatrix_solve has no CPU fallback')
    u = np.empty((n_prob, n_alpha, P, n_s))
    H = np.empty((n_prob, n_alpha, planes, m, m, n_omega))
    chi2, S, Q = (np.empty((n_prob, n_alpha)) for _ in range(3))
    n_iter, conv = (np.empty((n_prob, n_alpha), dtype=np.int32) for _ in range(2))
    ms = ctypes.c_float(0)
    rc = lib.mxe_fullmatrix_solve(int(device), n_prob, m, 1 if use_complex else 0, n_omega, n_s, n_alpha, _p(V), _p(c), _p(D),
                                  _p(alpha), _p(ghat), _p(cperp), _p(u0), maxiter, tol_h, _p(u), _p(H), _p(chi2), _p(S),
                                  _p(Q), _p(n_iter), _p(conv), ctypes.byref(ms))
    if rc != 0:
        raise MaxEntDeviceError('mxe_fullmatrix_solve failed: ' + lib.mxe_strerror(rc).decode())
    if timing is not None:
        timing['ms'] = float(ms.value)
    Hm = H[:, :, 0] + 1.0j * H[:, :, 1] if use_complex else H[:, :, 0]          # (n_prob, n_alpha, m, m, n_omega)
    return dict(u=u, H=np.ascontiguousarray(np.moveaxis(Hm, 1, 3)), chi2=chi2, S=S, Q=Q, n_iter=n_iter,
                converged=conv != 0)


def fullmatrix_solve_metric(V, R, A, D, alpha, ghat, cperp, m, use_complex, u0=None, maxiter=1000, tol_h=1e-9, device=0,
                            timing=None):
    """``mxe_fullmatrix_solve_metric``: :func:`fullmatrix_solve` with one error bar per matrix element.  In the place of
    ``c`` stand the dense factors ``R`` (P, n_s, n_s), diag(1 / sigma_p) U S = Q^_p R_p, and ``A`` (P, n_s, n_s),
    A_p = R_p^T R_p, of every component E_p, shared by the problems; ``V`` (n_omega, n_s) is the right singular basis itself
    and ``ghat`` (n_prob, P, n_s) = Q^_p^T (G_p / sigma_p).  Returns what :func:`fullmatrix_solve` returns.  Arguments the
    library would refuse raise ValueError before it is called."""
    V, R, A, D, alpha = _c(V), _c(R), _c(A), _c(D), _c(alpha)
    ghat, cperp = _c(ghat), _c(cperp)
    m, use_complex = int(m), bool(use_complex)
    if m < 1 or m > FULLMATRIX_MAX_M:
        raise ValueError('fullmatrix_solve_metric: matrices of %d x %d; 1 to %d are supported' % (m, m, FULLMATRIX_MAX_M))
    if V.ndim != 2 or V.shape[0] < 1 or V.shape[1] < 1:
        raise ValueError('fullmatrix_solve_metric: V must be (n_omega, n_s); got %s' % (V.shape,))
    n_omega, n_s = V.shape
    if n_s > FULLMATRIX_MAX_NS:
        raise ValueError('fullmatrix_solve_metric: %d singular values; at most %d are supported: cut the singular space with '
                         'reduce_singular_space' % (n_s, FULLMATRIX_MAX_NS))
    P = fullmatrix_P(m, use_complex)
    if R.shape != (P, n_s, n_s) or A.shape != (P, n_s, n_s):
        raise ValueError('fullmatrix_solve_metric: R and A must be (%d, %d, %d); got %s and %s' % (P, n_s, n_s, R.shape, A.shape))
    if D.shape != (n_omega,) or alpha.ndim != 1 or alpha.size < 1:
        raise ValueError('fullmatrix_solve_metric: D must be (n_omega,), alpha one-dimensional and not empty')
    if ghat.ndim != 3 or ghat.shape[0] < 1 or ghat.shape[1:] != (P, n_s) or cperp.shape != (ghat.shape[0],):
        raise ValueError('fullmatrix_solve_metric: ghat must be (n_prob, %d, %d) and cperp (n_prob,); got %s and %s'
                         % (P, n_s, ghat.shape, cperp.shape))
    n_prob, n_alpha = ghat.shape[0], alpha.size
    if u0 is not None:
        u0 = _c(u0)
        if u0.shape != ghat.shape:
            raise ValueError('fullmatrix_solve_metric: u0 must have the shape of ghat, %s; got %s' % (ghat.shape, u0.shape))
    for name, a in (('V', V), ('R', R), ('A', A), ('D', D), ('alpha', alpha), ('ghat', ghat), ('cperp', cperp), ('u0', u0)):
        if a is not None and not np.all(np.isfinite(a)):
            raise ValueError('fullmatrix_solve_metric: %s is not finite' % name)
    if not (np.all(D > 0) and np.all(alpha > 0)):
        raise ValueError('fullmatrix_solve_metric: D and alpha must be positive')
    maxiter, tol_h = int(maxiter), float(tol_h)
    if maxiter < 0 or not (tol_h > 0 and np.isfinite(tol_h)):
        raise ValueError('fullmatrix_solve_metric: maxiter must be >= 0 and tol_h positive and finite')
    planes = 2 if use_complex else 1
    if max(n_prob * n_alpha * planes * m * m * n_omega, n_prob * n_alpha * P * n_s, n_omega * n_s,
           P * (P + 1) // 2 * n_omega) > 2 ** 31 - 1:
        raise ValueError('fullmatrix_solve_metric: the arrays of this call hold more than 2^31 - 1 numbers')
    lib = load_library()
    if device_count() < 1:
        raise MaxEntDeviceError('no HIP device visible; mxe_fullmatrix_solve_metric has no CPU fallback')
    u = np.empty((n_prob, n_alpha, P, n_s))
    H = np.empty((n_prob, n_alpha, planes, m, m, n_omega))
    chi2, S, Q = (np.empty((n_prob, n_alpha)) for _ in range(3))
    n_iter, conv = (np.empty((n_prob, n_alpha), dtype=np.int32) for _ in range(2))
    ms = ctypes.c_float(0)
    rc = lib.mxe_fullmatrix_solve_metric(int(device), n_prob, m, 1 if use_complex else 0, n_omega, n_s, n_alpha, _p(V), _p(R),
                                         _p(A), _p(D), _p(alpha), _p(ghat), _p(cperp), _p(u0), maxiter, tol_h, _p(u), _p(H),
                                         _p(chi2), _p(S), _p(Q), _p(n_iter), _p(conv), ctypes.byref(ms))
    if rc != 0:
        raise MaxEntDeviceError('mxe_fullmatrix_solve_metric failed: ' + lib.mxe_strerror(rc).decode())
    if timing is not None:
        timing['ms'] = float(ms.value)
    Hm = H[:, :, 0] + 1.0j * H[:, :, 1] if use_complex else H[:, :, 0]          # (n_prob, n_alpha, m, m, n_omega)
    return dict(u=u, H=np.ascontiguousarray(np.moveaxis(Hm, 1, 3)), chi2=chi2, S=S, Q=Q, n_iter=n_iter,
                converged=conv != 0)


def fullmatrix_posterior_var(V, c, D, alpha, u, m, use_complex, F=None, want_diag=False, device=0, timing=None):
    """``mxe_fullmatrix_posterior_var``: posterior variances of the whole-matrix continuation.  ``V`` (n_omega, n_s),
    ``c`` (n_s,), ``D`` (n_omega,) as for :func:`fullmatrix_solve`; a job is one pair of ``alpha`` (n_job,) and ``u``
    (n_job, P, n_s); ``F`` (n_f, P, n_omega): the coordinates Tr(E_p F_i) of Hermitian weights on H, shared by the jobs.
    Returns a dict: ``value``, ``var``, ``prior`` (n_job, n_f) and, with ``want_diag``, ``diag_var``, ``diag_prior``, ``h``
    (n_job, P, n_omega), the variance of every coordinate h_p,i, the variance the entropy alone leaves, and h itself.  A job
    whose ``u`` or H is not finite or whose curvature is not positive definite is NaN throughout; ``u`` is therefore the one
    input that may hold a NaN.  ``timing``: a dict that receives the device time ``ms`` of the kernel.  The refusals are
    those of :func:`fullmatrix_solve`: arguments the library would refuse raise ValueError before it is called."""
    V, c, D, alpha, u = _c(V), _c(c), _c(D), _c(alpha), _c(u)
    m, use_complex, want_diag = int(m), bool(use_complex), bool(want_diag)
    if m < 1 or m > FULLMATRIX_MAX_M:
        raise ValueError('fullmatrix_posterior_var: matrices of %d x %d; 1 to %d are supported' % (m, m, FULLMATRIX_MAX_M))
    if V.ndim != 2 or V.shape[0] < 1 or V.shape[1] < 1:
        raise ValueError('fullmatrix_posterior_var: V must be (n_omega, n_s); got %s' % (V.shape,))
    n_omega, n_s = V.shape
    if n_s > FULLMATRIX_MAX_NS:
        raise ValueError('fullmatrix_posterior_var: %d singular values; at most %d are supported: cut the singular space with '
                         'reduce_singular_space' % (n_s, FULLMATRIX_MAX_NS))
    P = fullmatrix_P(m, use_complex)
    if c.shape != (n_s,) or D.shape != (n_omega,) or alpha.ndim != 1 or alpha.size < 1:
        raise ValueError('fullmatrix_posterior_var: c must be (n_s,), D (n_omega,), alpha one-dimensional and not empty')
    n_job = alpha.size
    if u.shape != (n_job, P, n_s):
        raise ValueError('fullmatrix_posterior_var: u must be (n_job, %d, %d) for %d alphas; got %s' % (P, n_s, n_job, u.shape))
    if F is not None:
        F = _c(F)
        if F.ndim != 3 or F.shape[1:] != (P, n_omega):
            raise ValueError('fullmatrix_posterior_var: F must be (n_f, %d, %d); got %s' % (P, n_omega, F.shape))
        if F.shape[0] == 0:
            F = None
    n_f = 0 if F is None else F.shape[0]
    if n_f == 0 and not want_diag:
        raise ValueError('fullmatrix_posterior_var: nothing to compute: give F or want_diag')
    for name, a in (('V', V), ('c', c), ('D', D), ('alpha', alpha), ('F', F)):
        if a is not None and not np.all(np.isfinite(a)):
            raise ValueError('fullmatrix_posterior_var: %s is not finite' % name)
    if not (np.all(c > 0) and np.all(D > 0) and np.all(alpha > 0)):
        raise ValueError('fullmatrix_posterior_var: c, D and alpha must be positive')
    if max(n_job * P * n_omega, n_job * P * n_s, n_omega * n_s, n_f * P * n_omega, n_job * n_f, 16 * P * n_omega,
           P * (P + 1) // 2 * n_omega) > 2 ** 31 - 1:
        raise ValueError('fullmatrix_posterior_var: the arrays of this call hold more than 2^31 - 1 numbers')
    lib = load_library()
    if device_count() < 1:
        raise MaxEntDeviceError('no HIP device visible; mxe_fullmatrix_posterior_var has no CPU fallback')
    value, var, prior = (np.empty((n_job, n_f)) for _ in range(3))
    dv, dp, h = (np.empty((n_job, P, n_omega)) if want_diag else None for _ in range(3))
    ms = ctypes.c_float(0)
    rc = lib.mxe_fullmatrix_posterior_var(int(device), n_job, m, 1 if use_complex else 0, n_omega, n_s, n_f, _p(V), _p(c), _p(D),
                                          _p(alpha), _p(u), _p(F), 1 if want_diag else 0, _p(value), _p(var), _p(prior),
                                          _p(dv), _p(dp), _p(h), ctypes.byref(ms))
    if rc != 0:
        raise MaxEntDeviceError('mxe_fullmatrix_posterior_var failed: ' + lib.mxe_strerror(rc).decode())
    if timing is not None:
        timing['ms'] = float(ms.value)
    out = dict(value=value, var=var, prior=prior)
    if want_diag:
        out.update(diag_var=dv, diag_prior=dp, h=h)
    return out


def fullmatrix_logdet(V, c, D, alpha, u, m, use_complex, want_ngood=True, device=0, timing=None):
    """``mxe_fullmatrix_logdet``: the evidence of alpha of the whole-matrix continuation.  ``V``, ``c``, ``D``, ``alpha``
    (n_job,) and ``u`` (n_job, P, n_s) as for :func:`fullmatrix_posterior_var`.  Returns a dict: ``logdet`` (n_job,),
    log det(I + c W c / alpha) of order d = P n_s, and, with ``want_ngood``, ``n_good`` (n_job,), the number of good data
    tr(c W c (alpha I + c W c)^-1).  A job whose ``u`` or H is not finite or whose curvature is not positive definite is
    NaN; ``u`` is therefore the one input that may hold a NaN.  ``timing``: a dict that receives the device time ``ms`` of
    the kernel.  Arguments the library would refuse raise ValueError before it is called."""
    V, c, D, alpha, u = _c(V), _c(c), _c(D), _c(alpha), _c(u)
    m, use_complex, want_ngood = int(m), bool(use_complex), bool(want_ngood)
    if m < 1 or m > FULLMATRIX_MAX_M:
        raise ValueError('fullmatrix_logdet: matrices of %d x %d; 1 to %d are supported' % (m, m, FULLMATRIX_MAX_M))
    if V.ndim != 2 or V.shape[0] < 1 or V.shape[1] < 1:
        raise ValueError('fullmatrix_logdet: V must be (n_omega, n_s); got %s' % (V.shape,))
    n_omega, n_s = V.shape
    if n_s > FULLMATRIX_MAX_NS:
        raise ValueError('fullmatrix_logdet: %d singular values; at most %d are supported: cut the singular space with '
                         'reduce_singular_space' % (n_s, FULLMATRIX_MAX_NS))
    P = fullmatrix_P(m, use_complex)
    if c.shape != (n_s,) or D.shape != (n_omega,) or alpha.ndim != 1 or alpha.size < 1:
        raise ValueError('fullmatrix_logdet: c must be (n_s,), D (n_omega,), alpha one-dimensional and not empty')
    n_job = alpha.size
    if u.shape != (n_job, P, n_s):
        raise ValueError('fullmatrix_logdet: u must be (n_job, %d, %d) for %d alphas; got %s' % (P, n_s, n_job, u.shape))
    for name, a in (('V', V), ('c', c), ('D', D), ('alpha', alpha)):
        if not np.all(np.isfinite(a)):
            raise ValueError('fullmatrix_logdet: %s is not finite' % name)
    if not (np.all(c > 0) and np.all(D > 0) and np.all(alpha > 0)):
        raise ValueError('fullmatrix_logdet: c, D and alpha must be positive')
    if max(n_job * P * n_s, n_omega * n_s, P * (P + 1) // 2 * n_omega) > 2 ** 31 - 1:
        raise ValueError('fullmatrix_logdet: the arrays of this call hold more than 2^31 - 1 numbers')
    lib = load_library()
    if device_count() < 1:
        raise MaxEntDeviceError('no HIP device visible; mxe_fullmatrix_logdet has no CPU fallback')
    logdet = np.empty(n_job)
    n_good = np.empty(n_job) if want_ngood else None
    ms = ctypes.c_float(0)
    rc = lib.mxe_fullmatrix_logdet(int(device), n_job, m, 1 if use_complex else 0, n_omega, n_s, _p(V), _p(c), _p(D), _p(alpha),
                                   _p(u), 1 if want_ngood else 0, _p(logdet), _p(n_good), ctypes.byref(ms))
    if rc != 0:
        raise MaxEntDeviceError('mxe_fullmatrix_logdet failed: ' + lib.mxe_strerror(rc).decode())
    if timing is not None:
        timing['ms'] = float(ms.value)
    out = dict(logdet=logdet)
    if want_ngood:
        out['n_good'] = n_good
    return out


class DeviceContext(object):
    """One solver context on one GPU: holds the truncated SVD of the kernel.

    Parameters mirror ``mxe_ctx_create``: ``U`` (n_tau x n_s), ``S`` (n_s),
    ``V`` (n_omega x n_s) as ``KernelSVD.U/.S/.V`` give them after
    ``reduce_singular_space`` (reference kernels.py:53-122).
    """

    def __init__(self, U, S, V, device=0, keep=None):
        """``keep``: stage only the first ``keep`` singular directions on the device (the caller has made sure that the others
        cannot be told from zero in its job: :func:`maxent_amd.batch_solver.directions_to_keep`).  The context still speaks
        ``n_s`` directions to its caller: start vectors are cut, returned v are filled up with zeros."""
        self._lib = load_library()
        self._h = _vp(None)
        S = _c(S)
        V = _c(V)
        self.n_s = int(S.shape[0])
        self.n_omega = int(V.shape[0])
        if V.shape[1] != self.n_s:
            raise ValueError('V must be n_omega x n_s')
        if U is not None:
            U = _c(U)
            if U.shape[1] != self.n_s:
                raise ValueError('U must be n_tau x n_s')
            self.n_tau = int(U.shape[0])
        else:
            self.n_tau = 1
        self._n_s_dev = self.n_s
        if keep is not None and int(keep) < self.n_s:
            if U is None or int(keep) < 1:
                raise ValueError('keep needs the unrotated U and at least one direction')
            self._n_s_dev = int(keep)
            U, S, V = _c(U[:, :self._n_s_dev]), _c(S[:self._n_s_dev]), _c(V[:, :self._n_s_dev])
        if device_count() < 1:
            raise MaxEntDeviceError('no HIP device visible; the solver has no '
                                    'CPU fallback')
        self._check(self._lib.mxe_ctx_create(
            int(device), self.n_tau, self.n_omega, self._n_s_dev,
            _p(U), _p(S), _p(V), ctypes.byref(self._h)), 'mxe_ctx_create')
        self.device = int(device)
        self._n_chain = 0
        self._n_alpha = 0
        self._ds_rows = []
        self._elem_rows = np.zeros(0, dtype=np.int64)      # rows of the data set of every element that is set

    # -- plumbing ------------------------------------------------------
    def _check(self, rc, what):
        if rc != 0:
            msg = self._lib.mxe_strerror(rc).decode()
            if rc == -2 and self._h:
                msg += ': ' + self._lib.mxe_last_hip_error(self._h).decode()
            raise MaxEntDeviceError('{} failed: {}'.format(what, msg))

    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            self._lib.mxe_ctx_destroy(self._h)
            self._h = _vp(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- data sets and elements ------------------------------------------
    def add_dataset(self, err, U_rot=None):
        """(U, err) pair -> whitened basis; returns the data-set id."""
        if U_rot is not None:
            U_rot = _c(U_rot)
            if self._n_s_dev < self.n_s:
                U_rot = _c(U_rot[:, :self._n_s_dev])
            n_rows = U_rot.shape[0]
        else:
            n_rows = self.n_tau
        err = _c(np.asarray(err, dtype=float) * np.ones(n_rows))
        i = ctypes.c_int(-1)
        self._check(self._lib.mxe_dataset_add(self._h, int(n_rows), _p(U_rot),
                                              _p(err), ctypes.byref(i)),
                    'mxe_dataset_add')
        self._ds_rows.append(int(n_rows))
        return i.value

    def clear_datasets(self):
        self._check(self._lib.mxe_dataset_clear(self._h), 'mxe_dataset_clear')
        self._ds_rows = []

    def set_elements(self, dataset_of_elem, G_list, D, entropy):
        """G_list: one data vector per element (already in its data set's
        rotated space); D: n_elem x n_omega (including delta-omega)."""
        ds = _c(dataset_of_elem, np.int32)
        n_elem = len(ds)
        if isinstance(G_list, np.ndarray) and G_list.ndim == 2:
            # one row per element, all of one length
            rows = np.asarray(self._ds_rows)[ds]
            if G_list.shape[0] != n_elem or np.any(rows != G_list.shape[1]):
                raise ValueError('G has shape {}, the data sets of its {} elements have {} rows'.format(
                    G_list.shape, n_elem, sorted(set(rows.tolist()))))
            G = _c(G_list)
            offs = np.arange(n_elem, dtype=np.int64) * G_list.shape[1]
            D = _c(D).reshape(n_elem, self.n_omega)
            ent = _c(entropy, np.int32)
            self._check(self._lib.mxe_elements_set(self._h, n_elem, _p(ds), _p(G), _p(offs), _p(D), _p(ent)),
                        'mxe_elements_set')
            self.n_elem = n_elem
            self._elem_rows = rows.astype(np.int64)
            return
        offs = np.zeros(n_elem, dtype=np.int64)
        chunks = []
        pos = 0
        for e in range(n_elem):
            g = _c(G_list[e]).ravel()
            if g.shape[0] != self._ds_rows[ds[e]]:
                raise ValueError('G of element {} has length {}, its data set '
                                 'has {} rows'.format(e, g.shape[0],
                                                      self._ds_rows[ds[e]]))
            offs[e] = pos
            pos += g.shape[0]
            chunks.append(g)
        G = _c(np.concatenate(chunks))
        D = _c(D).reshape(n_elem, self.n_omega)
        ent = _c(entropy, np.int32)
        self._check(self._lib.mxe_elements_set(self._h, n_elem, _p(ds), _p(G),
                                               _p(offs), _p(D), _p(ent)),
                    'mxe_elements_set')
        self.n_elem = n_elem
        self._elem_rows = np.asarray(self._ds_rows, dtype=np.int64)[ds]

    def update_data(self, G):
        """``mxe_elements_update_data``: new data vectors (one row per element, all of one length) for the elements that
        are set; data sets, default models, entropies and the staged chains stay"""
        G = _c(G)
        if G.ndim != 2 or G.shape[0] != self.n_elem:
            raise ValueError('G has shape {}, {} elements are set'.format(G.shape, self.n_elem))
        offs = np.arange(G.shape[0], dtype=np.int64) * G.shape[1]
        self._check(self._lib.mxe_elements_update_data(self._h, G.shape[0], _p(G), _p(offs)), 'mxe_elements_update_data')

    # -- the hot path ----------------------------------------------------
    def upload_chains(self, elem_of_chain, alpha_scaled, v0, opts=None):
        el = _c(elem_of_chain, np.int32)
        al = _c(alpha_scaled)
        if al.ndim == 1:
            al = np.ascontiguousarray(np.broadcast_to(al, (len(el), al.shape[0])))
        n_chain, n_alpha = al.shape
        v0 = _c(v0).reshape(n_chain, self.n_s)
        if self._n_s_dev < self.n_s:
            v0 = _c(v0[:, :self._n_s_dev])
        if opts is None:
            opts = default_opts()
        self._check(self._lib.mxe_chains_upload(self._h, n_chain, n_alpha,
                                                _p(el), _p(al), _p(v0),
                                                ctypes.byref(opts)),
                    'mxe_chains_upload')
        self._n_chain, self._n_alpha = n_chain, n_alpha

    def launch(self):
        self._check(self._lib.mxe_chains_launch(self._h), 'mxe_chains_launch')

    def sync(self):
        self._check(self._lib.mxe_sync(self._h), 'mxe_sync')

    def finish(self):
        """``mxe_chains_finish``: the alphas the lock-step layout gave up on, solved again in the one-chain
        layout (blocking); returns how many that was"""
        n = ctypes.c_int32(0)
        self._check(self._lib.mxe_chains_finish(self._h, ctypes.byref(n)), 'mxe_chains_finish')
        return int(n.value)

    def result_arrays(self, pinned_rows=None):
        """the per-alpha arrays :meth:`fetch` fills, uninitialised: chi2 / S / Q and n_iter / converged / n_evals as the
        rows of ONE block each -- the library then brings each block in one copy.  ``pinned_rows`` = n: both blocks and
        ``_rows`` [n][n_chain][n_omega] (the destination of :meth:`select3_prefetch_rows`) in one page-locked allocation,
        for :meth:`prefetch`"""
        nc, na = self._n_chain, self._n_alpha
        if pinned_rows is None:
            d = np.empty((3, nc, na))
            i = np.empty((3, nc, na), dtype=np.int32)
            return dict(chi2=d[0], S=d[1], Q=d[2], n_iter=i[0], converged=i[1], n_evals=i[2])
        nd, ni, nr = 3 * nc * na * 8, 3 * nc * na * 4, int(pinned_rows) * nc * self.n_omega * 8
        ni += (-ni) % 8
        buf = pinned_empty((nd + ni + nr,), np.uint8, min_bytes=0)
        d = buf[:nd].view(np.float64).reshape(3, nc, na)
        i = buf[nd:nd + 3 * nc * na * 4].view(np.int32).reshape(3, nc, na)
        rows = buf[nd + ni:].view(np.float64).reshape(int(pinned_rows), nc, self.n_omega)
        return dict(chi2=d[0], S=d[1], Q=d[2], n_iter=i[0], converged=i[1], n_evals=i[2], _d=d, _i=i, _rows=rows,
                    _pinned=is_pinned(buf))

    def prefetch(self, out):
        """``mxe_chains_prefetch``: the scalars of the launch copied into ``out`` (of ``result_arrays(pinned_rows=...)``) behind
        the kernel; :meth:`fetch` with the same ``out`` then waits and copies nothing"""
        self._check(self._lib.mxe_chains_prefetch(self._h, _p(out['_d']), _p(out['_i'])), 'mxe_chains_prefetch')
        self._held = getattr(self, '_held', [])
        self._held.append(out)          # (the destinations of copies in flight stay allocated until a call has waited for the stream)

    def select3_prefetch_rows(self, first, count, rows):
        """``mxe_select3_prefetch_rows``: behind :meth:`select3_launch`; :meth:`select3_fetch_rows` with the same arguments
        then waits and converts the indices"""
        self._check(self._lib.mxe_select3_prefetch_rows(self._h, int(first), int(count), _p(rows) if count > 0 else None),
                    'mxe_select3_prefetch_rows')
        self._held = getattr(self, '_held', [])
        self._held.append(rows)

    def fetch(self, want_v=True, want_H=True, out=None):
        """``out``: the arrays of :meth:`result_arrays`, made by the caller before the launch"""
        nc, na = self._n_chain, self._n_alpha
        if out is None:
            out = self.result_arrays()
        elif out['chi2'].shape != (nc, na):
            raise ValueError('result arrays of another launch')
        v = np.empty((nc, na, self._n_s_dev)) if want_v else None
        H = pinned_empty((nc, na, self.n_omega)) if want_H else None
        self._check(self._lib.mxe_chains_fetch(
            self._h, _p(v), _p(H), _p(out['chi2']), _p(out['S']), _p(out['Q']),
            _p(out['n_iter']), _p(out['converged']), _p(out['n_evals'])),
            'mxe_chains_fetch')
        self._held = []                 # (the stream has been waited for)
        if v is not None and self._n_s_dev < self.n_s:
            full = np.zeros((nc, na, self.n_s))
            full[..., :self._n_s_dev] = v
            v = full
        out['v'] = v
        out['H'] = H
        return out

    def logdet(self):
        """log det(I + M W / alpha) per problem of the last launch, [n_chain][n_alpha]."""
        out = np.empty((self._n_chain, self._n_alpha))
        self._check(self._lib.mxe_logdet(self._h, _p(out)), 'mxe_logdet')
        return out

    def fetch_n_act(self):
        """diagnostic: size of the coupled block per problem, [n_chain][n_alpha]."""
        out = np.empty((self._n_chain, self._n_alpha), dtype=np.int32)
        self._check(self._lib.mxe_chains_fetch_nact(self._h, _p(out)), 'mxe_chains_fetch_nact')
        return out

    def solve_chains(self, elem_of_chain, alpha_scaled, v0, opts=None,
                     want_v=True, want_H=True):
        """Blocking solve: upload, one launch, fetch (``mxe_solve_chains``)."""
        self.upload_chains(elem_of_chain, alpha_scaled, v0, opts)
        self.launch()
        self.finish()
        return self.fetch(want_v, want_H)

    def eval_batch(self, elem_of_problem, alpha_scaled, x, input_is_H=False, chi2_factor=1.0,
                   want=('Q', 'chi2', 'S', 'H', 'g', 'W')):
        """``mxe_eval_batch``: cost function and derivative ingredients at caller-supplied points.
        ``x``: (P, n_s) vectors v, or (P, n_omega) hidden images with ``input_is_H``.  ``want``: any of
        Q, chi2, S, H, u, w, q, h, g, W, W2.  Returns a dict of arrays."""
        if self._n_s_dev < self.n_s:
            raise MaxEntDeviceError('eval_batch on a context that keeps %d of %d singular directions' % (self._n_s_dev, self.n_s))
        el = _c(np.atleast_1d(elem_of_problem), np.int32)
        P = len(el)
        al = _c(np.broadcast_to(np.asarray(alpha_scaled, dtype=float), (P,)))
        x = _c(x).reshape(P, self.n_omega if input_is_H else self.n_s)
        shapes = dict(Q=(P,), chi2=(P,), S=(P,), H=(P, self.n_omega), u=(P, self.n_omega),
                      w=(P, self.n_omega), q=(P, self.n_omega), h=(P, self.n_s), g=(P, self.n_s),
                      W=(P, self.n_s, self.n_s), W2=(P, self.n_s, self.n_s))
        out = {}
        for k in want:
            if k not in shapes:
                raise TypeError('unknown output {!r}'.format(k))
            out[k] = np.empty(shapes[k])
        args = [_p(out.get(k)) for k in ('Q', 'chi2', 'S', 'H', 'u', 'w', 'q', 'h', 'g', 'W', 'W2')]
        self._check(self._lib.mxe_eval_batch(self._h, P, _p(el), _p(al), _p(x), int(bool(input_is_H)),
                                             float(chi2_factor), *args), 'mxe_eval_batch')
        return out

    def _posterior_problems(self, name, elem_of_problem, alpha_scaled):
        """the problems of :meth:`posterior_var` / :meth:`posterior_sample` as the library takes them: ``(el, P, al)``"""
        if self._n_s_dev < self.n_s:
            raise MaxEntDeviceError('%s on a context that keeps %d of %d singular directions' % (name, self._n_s_dev, self.n_s))
        el = _c(np.atleast_1d(elem_of_problem), np.int32)
        P = len(el)
        al = _c(np.broadcast_to(np.asarray(alpha_scaled, dtype=float), (P,)))
        if not np.all(al > 0) or not np.all(np.isfinite(al)):
            raise ValueError('%s: every alpha must be positive and finite' % name)
        return el, P, al

    def _posterior_rows(self, name, P, H, problem_index, unlaunched_ok=False):
        """the hidden images of the P problems as the library takes them: ``(H, pi)``, one of them None.
        ``unlaunched_ok``: before any launch the rows of ``problem_index`` are not checked here."""
        if H is not None:
            return _c(H).reshape(P, self.n_omega), None
        pi = _c(np.arange(P) if problem_index is None else np.atleast_1d(problem_index), np.int32)
        n_last = self._n_chain * self._n_alpha
        check_rows = P and (n_last or not unlaunched_ok)
        if len(pi) != P or (check_rows and (pi.min() < 0 or pi.max() >= n_last)):
            raise ValueError('%s: problem_index must name %d problems of the last launch (%d x %d)'
                             % (name, P, self._n_chain, self._n_alpha))
        return None, pi

    def posterior_var(self, elem_of_problem, alpha_scaled, H=None, problem_index=None, F=None, chi2_factor=1.0,
                      want_diag=False, timing=None):
        """``mxe_posterior_var``: Gaussian posterior variances around the minimiser, on the staged elements.
        ``H``: (P, n_omega) hidden images, or None for rows ``problem_index`` (chain * n_alpha + alpha index) of the last
        launch, read on the device.  ``F``: (n_f, n_omega) weights on H.  Returns a dict: ``var`` and ``prior`` (P, n_f) --
        f^T Gamma f and f^T diag(w) f / alpha~ -- and, with ``want_diag``, ``diag`` (P, n_omega) = Gamma_ii.  A problem whose
        H row is not finite or whose curvature matrix is not positive definite has NaN everywhere.  ``timing``: a dict that
        receives the device time ``ms`` of the kernel."""
        el, P, al = self._posterior_problems('posterior_var', elem_of_problem, alpha_scaled)
        H, pi = self._posterior_rows('posterior_var', P, H, problem_index)
        if F is not None:
            F = _c(np.atleast_2d(F))
            if F.shape[1] != self.n_omega:
                raise ValueError('posterior_var: F has %d columns, the omega mesh %d points' % (F.shape[1], self.n_omega))
            if not np.all(np.isfinite(F)):
                raise ValueError('posterior_var: F holds values that are not finite')
        n_f = 0 if F is None else F.shape[0]
        if n_f == 0 and not want_diag:
            raise ValueError('posterior_var: neither functionals nor the diagonal asked for')
        var, prior = np.empty((P, n_f)), np.empty((P, n_f))
        diag = np.empty((P, self.n_omega)) if want_diag else None
        ms = ctypes.c_float(0)
        self._check(self._lib.mxe_posterior_var(self._h, P, _p(el), _p(al), _p(H), _p(pi), float(chi2_factor), n_f,
                                                _p(F) if n_f else None, _p(var) if n_f else None, _p(diag),
                                                _p(prior) if n_f else None, ctypes.byref(ms)), 'mxe_posterior_var')
        if timing is not None:
            timing['ms'] = float(ms.value)
        out = dict(var=var, prior=prior)
        if want_diag:
            out['diag'] = diag
        return out

    def posterior_sample(self, elem_of_problem, alpha_scaled, H=None, problem_index=None, chi2_factor=1.0, n_samples=1, seed=0,
                         stream=None, z=None, timing=None):
        """``mxe_posterior_sample``: draws ``delta`` (P, n_samples, n_omega) from the Gaussian posterior N(0, Gamma) around
        the minimiser, on the staged elements; a sample of H is the minimiser plus its row.  ``H``, ``problem_index`` and
        ``chi2_factor`` as in :meth:`posterior_var`.  ``z=None``: problem p draws from the counter-based stream
        ``(seed, stream[p])`` (``stream``: P 64-bit ids, default 0 .. P-1; see :func:`normals`); else ``z``
        (P, n_samples, n_omega + n_s) standard normals that are used as given.  A problem whose H row is not finite or whose
        curvature matrix is not positive definite has NaN in all its samples.  ``timing``: a dict that receives the device
        time ``ms``."""
        el, P, al = self._posterior_problems('posterior_sample', elem_of_problem, alpha_scaled)
        n_samples = int(n_samples)
        if n_samples < 1:
            raise ValueError('posterior_sample: n_samples must be at least 1')
        nz = self.n_omega + self.n_s
        if P * n_samples * nz > 2 ** 31 - 1:
            raise ValueError('posterior_sample: P n_samples (n_omega + n_s) = %d exceeds 2^31 - 1; draw in several calls'
                             % (P * n_samples * nz))
        # (nothing launched: the library answers MXE_ERR_STATE)
        H, pi = self._posterior_rows('posterior_sample', P, H, problem_index, unlaunched_ok=True)
        st = None
        if z is not None:
            z = _c(z)
            if z.shape != (P, n_samples, nz):
                raise ValueError('posterior_sample: z must have the shape (P, n_samples, n_omega + n_s) = %r, got %r'
                                 % ((P, n_samples, nz), z.shape))
            if not np.all(np.isfinite(z)):
                raise ValueError('posterior_sample: z holds values that are not finite')
        else:
            st = np.ascontiguousarray(np.arange(P) if stream is None else np.atleast_1d(stream), dtype=np.uint64)
            if st.shape != (P,):
                raise ValueError('posterior_sample: stream must hold one id per problem')
        out = np.empty((P, n_samples, self.n_omega))
        ms = ctypes.c_float(0)
        self._check(self._lib.mxe_posterior_sample(
            self._h, P, _p(el), _p(al), _p(H), _p(pi), float(chi2_factor), n_samples, int(seed) & (2 ** 64 - 1),
            None if st is None else st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), _p(z), _p(out), ctypes.byref(ms)),
            'mxe_posterior_sample')
        if timing is not None:
            timing['ms'] = float(ms.value)
        return out

    def fit_diagnostics(self, elem_of_problem, alpha_scaled, H=None, problem_index=None, chi2_factor=1.0, ld=None,
                        timing=None):
        """``mxe_fit_diagnostics``: leverages, number of good data and whitened residuals of the fits, on the staged
        elements.  ``H``, ``problem_index`` and ``chi2_factor`` as in :meth:`posterior_var`.  Returns a dict: ``n_good``
        and ``chi2`` (P,), ``residual`` and ``leverage`` (P, ld) -- ``ld``: default the largest row count among the data
        sets of the problems; entries behind a data set's rows are 0 --, and ``rows`` (P,), the row count of every
        problem's data set.  A problem whose H row is not finite or whose curvature matrix is not positive definite has
        NaN everywhere.  ``timing``: a dict that receives the device time ``ms`` of the kernel."""
        el, P, al = self._posterior_problems('fit_diagnostics', elem_of_problem, alpha_scaled)
        # (nothing launched: the library answers MXE_ERR_STATE)
        H, pi = self._posterior_rows('fit_diagnostics', P, H, problem_index, unlaunched_ok=True)
        if P and (el.min() < 0 or el.max() >= len(self._elem_rows)):
            raise ValueError('fit_diagnostics: elements 0 .. %d are set' % (len(self._elem_rows) - 1))
        rows = self._elem_rows[el]
        ld = int(rows.max()) if ld is None else int(ld)
        ngood, chi2 = np.empty(P), np.empty(P)
        resid, lev = np.empty((P, max(ld, 0))), np.empty((P, max(ld, 0)))
        ms = ctypes.c_float(0)
        self._check(self._lib.mxe_fit_diagnostics(self._h, P, _p(el), _p(al), _p(H), _p(pi), float(chi2_factor), ld,
                                                  _p(ngood), _p(chi2), _p(resid), _p(lev), ctypes.byref(ms)),
                    'mxe_fit_diagnostics')
        if timing is not None:
            timing['ms'] = float(ms.value)
        return dict(n_good=ngood, chi2=chi2, residual=resid, leverage=lev, rows=rows)

    def response(self, elem_of_problem, alpha_scaled, F, H=None, problem_index=None, chi2_factor=1.0, space='model',
                 weighted=True, max_values=None, timing=None):
        """``mxe_response``: the linear response of the minimiser, on the staged elements.  ``F``: right-hand sides,
        (n_rhs, ld) for every problem alike or (P, n_rhs, ld) -- ``space='model'``: perturbations of the true H
        (ld = n_omega), ``X = [diag(w)] V' c B^-1 c V'^T F``: with ``weighted`` the rows ``R f`` of the resolution operator,
        without it those of the symmetric ``S``; ``space='data'``: whitened perturbations of the data in the rows of each
        problem's data set (ld at least the largest row count; entries behind a set's rows are ignored),
        ``X = [diag(w)] V' c B^-1 U^^T F``.  ``H``, ``problem_index`` and ``chi2_factor`` as in :meth:`posterior_var`.
        Returns X (P, n_rhs, n_omega).  A problem whose H row is not finite or whose curvature matrix is not positive
        definite has NaN everywhere.  The problems go in calls of at most ``max_values`` values of the largest array
        (default 2^31 - 1, the library's limit); the bits of a problem do not depend on the call it is in.  ``timing``: a
        dict that receives the device time ``ms`` of the kernels and the number of ``launches``."""
        el, P, al = self._posterior_problems('response', elem_of_problem, alpha_scaled)
        if space not in ('model', 'data'):
            raise ValueError("response: space must be 'model' or 'data', got %r" % (space,))
        # (nothing launched: the library answers MXE_ERR_STATE)
        H, pi = self._posterior_rows('response', P, H, problem_index, unlaunched_ok=True)
        F = np.asarray(F, dtype=float)
        if F.ndim == 2:
            F = np.broadcast_to(F, (P,) + F.shape)
        if F.ndim != 3 or F.shape[0] != P or F.shape[1] < 1:
            raise ValueError('response: F must have the shape (n_rhs, ld) or (P, n_rhs, ld), got %r' % (F.shape,))
        n_rhs, ld = F.shape[1], F.shape[2]
        if space == 'model':
            if ld != self.n_omega:
                raise ValueError('response: F has %d columns, the omega mesh %d points' % (ld, self.n_omega))
        else:
            if P and (el.min() < 0 or el.max() >= len(self._elem_rows)):
                raise ValueError('response: elements 0 .. %d are set' % (len(self._elem_rows) - 1))
            if ld < 1 or ld < int(self._elem_rows[el].max()):
                raise ValueError('response: F has %d columns, the largest data set %d rows' % (ld, int(self._elem_rows[el].max())))
        if not np.all(np.isfinite(F)):
            raise ValueError('response: F holds values that are not finite')
        per = n_rhs * max(ld, self.n_omega)
        limit = 2 ** 31 - 1 if max_values is None else min(int(max_values), 2 ** 31 - 1)
        cap = limit // per
        if cap < 1:
            raise ValueError('response: n_rhs max(ld, n_omega) = %d exceeds %d values; hand the right-hand sides in in '
                             'several calls' % (per, limit))
        out = np.empty((P, n_rhs, self.n_omega))
        ms_total, launches = 0.0, 0
        for p0 in range(0, P, cap):
            p1 = min(p0 + cap, P)
            ms = ctypes.c_float(0)
            Fp = _c(F[p0:p1])
            Xp = out[p0:p1]                   # (a C-contiguous slice of problems: the library writes it in place)
            self._check(self._lib.mxe_response(
                self._h, p1 - p0, _p(el[p0:p1]), _p(al[p0:p1]), None if H is None else _p(H[p0:p1]),
                None if pi is None else _p(pi[p0:p1]), float(chi2_factor), 0 if space == 'model' else 1,
                int(bool(weighted)), n_rhs, ld, _p(Fp), Xp.ctypes.data_as(_dp), ctypes.byref(ms)), 'mxe_response')
            ms_total += float(ms.value)
            launches += 1
        if timing is not None:
            timing['ms'] = ms_total
            timing['launches'] = launches
        return out

    def resample_reduce(self, group_offset, scale, H=None, problem_index=None, F=None, want=('mean', 'var', 'fval', 'fmean', 'fcov'),
                        timing=None):
        """``mxe_resample_reduce``: mean, spread and functional covariances of groups of hidden images.  Group g owns the
        rows ``group_offset[g] .. group_offset[g + 1] - 1``; ``H``: (rows, n_omega) on the host, or None for the rows
        ``problem_index`` (chain * n_alpha + alpha index) of the last launch, read on the device.  ``scale``: (n_groups,),
        the factor on the centred sums of squares.  ``F``: (n_f, n_omega) weights on H.  Returns a dict with ``used``
        (n_groups: finite rows -- the others are left out) and what ``want`` names: ``mean``, ``var`` (n_groups, n_omega),
        ``fval`` (rows, n_f), ``fmean`` (n_groups, n_f), ``fcov`` (n_groups, n_f, n_f).  A group with fewer than two used
        rows has NaN variances.  ``timing``: a dict that receives the device time ``ms`` of the kernel."""
        off = _c(np.atleast_1d(group_offset), np.int32)
        ng = len(off) - 1
        if ng < 1 or off[0] != 0 or np.any(np.diff(off) < 0):
            raise ValueError('resample_reduce: group_offset must start at 0, not decrease and name at least one group')
        rows = int(off[-1])
        sc = _c(np.broadcast_to(np.asarray(scale, dtype=float), (ng,)))
        if not np.all(np.isfinite(sc)):
            raise ValueError('resample_reduce: every scale must be finite')
        pi = None
        if H is not None:
            H = _c(H).reshape(rows, self.n_omega)
        else:
            pi = _c(np.arange(rows) if problem_index is None else np.atleast_1d(problem_index), np.int32)
            n_last = self._n_chain * self._n_alpha           # (0: nothing was staged -- the library answers MXE_ERR_STATE)
            if len(pi) != rows or (rows and n_last and (pi.min() < 0 or pi.max() >= n_last)):
                raise ValueError('resample_reduce: problem_index must name %d problems of the last launch (%d x %d)'
                                 % (rows, self._n_chain, self._n_alpha))
        n_f = 0
        if F is not None and len(F):
            F = _c(np.atleast_2d(F))
            if F.shape[1] != self.n_omega:
                raise ValueError('resample_reduce: F has %d columns, the omega mesh %d points' % (F.shape[1], self.n_omega))
            if not np.all(np.isfinite(F)):
                raise ValueError('resample_reduce: F holds values that are not finite')
            n_f = F.shape[0]
        shapes = dict(mean=(ng, self.n_omega), var=(ng, self.n_omega), fval=(rows, n_f), fmean=(ng, n_f), fcov=(ng, n_f, n_f))
        out = {}
        for k in want:
            if k not in shapes:
                raise TypeError('unknown output {!r}'.format(k))
            out[k] = np.empty(shapes[k])
        used = np.zeros(ng, dtype=np.int32)
        ms = ctypes.c_float(0)
        self._check(self._lib.mxe_resample_reduce(self._h, ng, _p(off), _p(H), _p(pi), _p(sc), n_f, _p(F) if n_f else None,
                                                  _p(out.get('mean')), _p(out.get('var')), _p(out.get('fval')),
                                                  _p(out.get('fmean')), _p(out.get('fcov')), _p(used), ctypes.byref(ms)),
                    'mxe_resample_reduce')
        if timing is not None:
            timing['ms'] = float(ms.value)
        out['used'] = used
        return out

    def resample_quantiles(self, group_offset, q, H=None, problem_index=None, timing=None):
        """``mxe_resample_quantiles``: per omega point the type-7 quantiles (numpy's ``method='linear'``) ``q`` over the
        finite rows of every group of hidden images.  The groups, ``H`` and ``problem_index`` are those of
        :meth:`resample_reduce`.  Returns a dict: ``q`` (n_groups, n_q, n_omega; NaN for a group without a finite row) and
        ``used`` (n_groups, as :meth:`resample_reduce` counts them).  A group of more than ``QUANTILE_MAX_ROWS`` rows
        raises :class:`MaxEntDeviceError` (MXE_ERR_LIMIT).  ``timing``: a dict that receives the device time ``ms`` of the
        two kernels."""
        off = _c(np.atleast_1d(group_offset), np.int32)
        ng = len(off) - 1
        if ng < 1 or off[0] != 0 or np.any(np.diff(off) < 0):
            raise ValueError('resample_quantiles: group_offset must start at 0, not decrease and name at least one group')
        rows = int(off[-1])
        qq = _c(np.atleast_1d(q))
        if qq.ndim != 1 or len(qq) < 1 or not np.all((qq >= 0.0) & (qq <= 1.0)):
            raise ValueError('resample_quantiles: at least one probability, every one in [0, 1], is needed')
        pi = None
        if H is not None:
            H = _c(H).reshape(rows, self.n_omega)
        else:
            pi = _c(np.arange(rows) if problem_index is None else np.atleast_1d(problem_index), np.int32)
            n_last = self._n_chain * self._n_alpha           # (0: nothing was staged -- the library answers MXE_ERR_STATE)
            if len(pi) != rows or (rows and n_last and (pi.min() < 0 or pi.max() >= n_last)):
                raise ValueError('resample_quantiles: problem_index must name %d problems of the last launch (%d x %d)'
                                 % (rows, self._n_chain, self._n_alpha))
        out = np.empty((ng, len(qq), self.n_omega))
        used = np.zeros(ng, dtype=np.int32)
        ms = ctypes.c_float(0)
        rc = self._lib.mxe_resample_quantiles(self._h, ng, _p(off), _p(H), _p(pi), len(qq), _p(qq), _p(out), _p(used),
                                              ctypes.byref(ms))
        if rc == _MXE_ERR_LIMIT:
            raise MaxEntDeviceError('mxe_resample_quantiles failed: a group of %d rows exceeds the limit of %d rows the kernel '
                                    'sorts in LDS' % (int(np.diff(off).max()), QUANTILE_MAX_ROWS))
        self._check(rc, 'mxe_resample_quantiles')
        if timing is not None:
            timing['ms'] = float(ms.value)
        return dict(q=out, used=used)

    def cv_score(self, group_offset, K, Gval, w, T=None, rank=None, H=None, problem_index=None, want_z=True, timing=None):
        """``mxe_cv_score``: the out-of-sample chi2 of groups of hidden images against held-out data.  The groups, ``H``
        and ``problem_index`` are those of :meth:`resample_reduce`; a group is one (element, fold), its rows the alphas of
        the fold's training scan.  ``K``: (n_data, n_omega), the job's kernel as :func:`mock_data` takes it; ``Gval``,
        ``w``: (n_groups, n_data) validation data in the rotated basis and weights >= 0; ``T``, ``rank``: both None or
        (n_groups, n_data, n_data) and (n_groups,) as :func:`bins_eig` returns them (rows behind the rank zero).  Returns a
        dict: ``score`` (rows,), ``z`` (rows, n_data; with ``want_z``) -- ``z[r, k] = sqrt(w[g, k]) ((T_g K H_r)[k] -
        Gval[g, k])`` for k < rank, 0 behind it, ``score = sum_k z^2``; NaN for a row whose H is not finite -- and ``used``
        (n_groups: finite rows).  ``timing``: a dict that receives the device time ``ms`` of the kernels."""
        off = _c(np.atleast_1d(group_offset), np.int32)
        ng = len(off) - 1
        if ng < 1 or off[0] != 0 or np.any(np.diff(off) < 0):
            raise ValueError('cv_score: group_offset must start at 0, not decrease and name at least one group')
        rows = int(off[-1])
        Km = _c(np.atleast_2d(K))
        n_data, n_omega = Km.shape
        if n_data < 1 or n_omega < 1:
            raise ValueError('cv_score: K must be (n_data, n_omega), got %r' % (Km.shape,))
        Gv, wm = _c(Gval).reshape(-1, n_data), _c(w).reshape(-1, n_data)
        if Gv.shape != (ng, n_data) or wm.shape != (ng, n_data):
            raise ValueError('cv_score: Gval and w must be (n_groups, n_data) = %r' % ((ng, n_data),))
        if not (np.all(np.isfinite(Km)) and np.all(np.isfinite(Gv))):
            raise ValueError('cv_score: K or Gval holds values that are not finite')
        if not (np.all(np.isfinite(wm)) and np.all(wm >= 0.0)):
            raise ValueError('cv_score: every weight must be finite and >= 0')
        if (T is None) != (rank is None):
            raise ValueError('cv_score: T and rank go together')
        Tm = rk = None
        if T is not None:
            Tm = _c(T).reshape(-1, n_data, n_data)
            rk = _c(np.broadcast_to(np.asarray(rank, dtype=np.int32), (ng,)), np.int32)
            if Tm.shape[0] != ng or not np.all(np.isfinite(Tm)):
                raise ValueError('cv_score: T must be (n_groups, n_data, n_data) and finite')
            if rk.min() < 0 or rk.max() > n_data:
                raise ValueError('cv_score: every rank must lie in 0 .. n_data')
        pi = None
        if H is not None:
            H = _c(H).reshape(rows, n_omega)
        else:
            if n_omega != self.n_omega:
                raise ValueError('cv_score: K has %d columns, the omega mesh of the launch %d points' % (n_omega, self.n_omega))
            pi = _c(np.arange(rows) if problem_index is None else np.atleast_1d(problem_index), np.int32)
            n_last = self._n_chain * self._n_alpha           # (0: nothing was staged -- the library answers MXE_ERR_STATE)
            if len(pi) != rows or (rows and n_last and (pi.min() < 0 or pi.max() >= n_last)):
                raise ValueError('cv_score: problem_index must name %d problems of the last launch (%d x %d)'
                                 % (rows, self._n_chain, self._n_alpha))
        score = np.empty(rows)
        z = np.empty((rows, n_data)) if want_z else None
        used = np.zeros(ng, dtype=np.int32)
        ms = ctypes.c_float(0)
        rc = self._lib.mxe_cv_score(self._h, ng, _p(off), _p(H), _p(pi), n_data, n_omega, _p(Km), _p(Tm), _p(rk), _p(Gv), _p(wm),
                                    _p(score), _p(z), _p(used), ctypes.byref(ms))
        if rc == _MXE_ERR_ARG:
            raise ValueError('mxe_cv_score refused its arguments (%d rows in %d groups, %d data values, %d omega points, H %s): it '
                             'takes sizes of at least 1 whose products stay within 2^31 - 1, offsets that start at 0 and do not '
                             'decrease, problem_index inside the last launch and its n_omega, T and rank together, ranks in '
                             '0 .. n_data, finite K, T, Gval and finite w >= 0'
                             % (rows, ng, n_data, n_omega, 'handed in' if H is not None else 'of the last launch (%d x %d problems)'
                                % (self._n_chain, self._n_alpha)))
        self._check(rc, 'mxe_cv_score')
        if timing is not None:
            timing['ms'] = float(ms.value)
        out = dict(score=score, used=used)
        if want_z:
            out['z'] = z
        return out

    def evidence_reduce(self, group_offset, logp, log_quad, log_mix=None, H=None, chain_index=None, log_prior=None,
                        row_mode=0, pick=None, F=None,
                        want=('walpha', 'row', 'fval', 'mean', 'between', 'fmean', 'fcov'), timing=None):
        """``mxe_evidence_reduce``: the evidence of every scan and the model averages of every group of scans.  Group g
        owns the scans ``group_offset[g] .. group_offset[g + 1] - 1``; ``logp``: (n_scan, n_alpha) log probabilities (NaN
        and infinities are data); ``log_quad``: (n_alpha,) the log measure of the evidence integral; ``log_mix``: the one of
        the mixture over alpha (default zeros); ``H``: (n_scan, n_alpha, n_omega) on the host, or None for the chains
        ``chain_index`` (default 0 .. n_scan - 1) of the last launch, read on the device; ``log_prior``: (n_scan,) or
        None; ``row_mode``: 0 Bryan mixture, 1 the row at the largest logp, 2 the row ``pick[s]``; ``F``: (n_f, n_omega)
        weights on H.  Returns a dict with ``logZ``, ``kmax``, ``ngood``, ``wmodel`` (n_scan), ``used`` (n_groups) and what
        ``want`` names: ``walpha`` (n_scan, n_alpha), ``row`` (n_scan, n_omega), ``fval`` (n_scan, n_f), ``mean``,
        ``between`` (n_groups, n_omega), ``fmean`` (n_groups, n_f), ``fcov`` (n_groups, n_f, n_f).  ``timing``: a dict that
        receives the device time ``ms`` of the two kernels."""
        off = _c(np.atleast_1d(group_offset), np.int32)
        ng = len(off) - 1
        if ng < 1 or off[0] != 0 or np.any(np.diff(off) < 0):
            raise ValueError('evidence_reduce: group_offset must start at 0, not decrease and name at least one group')
        ns = int(off[-1])
        lq = _c(np.atleast_1d(log_quad))
        na = len(lq)
        lp = _c(logp).reshape(ns, na) if ns else np.zeros((0, na))
        lm = np.zeros(na) if log_mix is None else _c(np.atleast_1d(log_mix))
        if lq.ndim != 1 or na < 1 or lm.shape != lq.shape:
            raise ValueError('evidence_reduce: log_quad and log_mix must hold one value per alpha')
        ci = None
        if H is not None:
            H = _c(H).reshape(ns, na, self.n_omega)
        elif chain_index is not None:
            ci = _c(np.atleast_1d(chain_index), np.int32)
            if len(ci) != ns:
                raise ValueError('evidence_reduce: chain_index must name %d chains' % ns)
        pr = None
        if log_prior is not None:
            pr = _c(np.atleast_1d(log_prior))
            if pr.shape != (ns,):
                raise ValueError('evidence_reduce: log_prior must hold one value per scan')
        pk = None
        if pick is not None:
            pk = _c(np.atleast_1d(pick), np.int32)
            if pk.shape != (ns,):
                raise ValueError('evidence_reduce: pick must hold one index per scan')
        n_f = 0
        if F is not None and len(F):
            F = _c(np.atleast_2d(F))
            if F.shape[1] != self.n_omega:
                raise ValueError('evidence_reduce: F has %d columns, the omega mesh %d points' % (F.shape[1], self.n_omega))
            n_f = F.shape[0]
        nw = self.n_omega
        shapes = dict(walpha=(ns, na), row=(ns, nw), fval=(ns, n_f), mean=(ng, nw), between=(ng, nw), fmean=(ng, n_f),
                      fcov=(ng, n_f, n_f))
        out = {}
        for k in want:
            if k not in shapes:
                raise TypeError('unknown output {!r}'.format(k))
            out[k] = np.empty(shapes[k])
        out.update(logZ=np.empty(ns), wmodel=np.empty(ns), kmax=np.zeros(ns, dtype=np.int32),
                   ngood=np.zeros(ns, dtype=np.int32), used=np.zeros(ng, dtype=np.int32))
        ms = ctypes.c_float(0)
        rc = self._lib.mxe_evidence_reduce(
            self._h, ng, _p(off), na, _p(H), _p(ci), _p(lp), _p(lq), _p(lm), _p(pr), int(row_mode), _p(pk), n_f,
            _p(F) if n_f else None, _p(out['logZ']), _p(out['kmax']), _p(out['ngood']), _p(out.get('walpha')),
            _p(out.get('row')), _p(out.get('fval')), _p(out['wmodel']), _p(out.get('mean')), _p(out.get('between')),
            _p(out.get('fmean')), _p(out.get('fcov')), _p(out['used']), ctypes.byref(ms))
        if rc == _MXE_ERR_ARG:
            raise ValueError('mxe_evidence_reduce refused its arguments: a row_mode outside 0 .. 2, row_mode 2 without pick, a '
                             'pick >= n_alpha, a chain_index outside the last launch (%d chains of %d alphas), a log_quad, log_mix '
                             'or F that is not finite, a log_prior that is NaN or +inf, or sizes whose products exceed 2^31 - 1'
                             % (self._n_chain, self._n_alpha))
        self._check(rc, 'mxe_evidence_reduce')
        if timing is not None:
            timing['ms'] = float(ms.value)
        return out

    def audit(self):
        """``mxe_audit``: exact Newton correction size and relative gradient of every problem of the
        last launch, each [n_chain][n_alpha]."""
        corr = np.empty((self._n_chain, self._n_alpha))
        gmax = np.empty((self._n_chain, self._n_alpha))
        self._check(self._lib.mxe_audit(self._h, _p(corr), _p(gmax)), 'mxe_audit')
        return dict(corr=corr, gmax=gmax)

    # -- the analyzer's alpha on the device, selected rows --------------------
    def select_launch(self, linefit_deg=0):
        self._check(self._lib.mxe_select_launch(self._h, int(linefit_deg)), 'mxe_select_launch')

    def select_fetch(self, want_H=True):
        idx = np.empty(self._n_chain, dtype=np.int32)
        Hs = np.empty((self._n_chain, self.n_omega)) if want_H else None
        self._check(self._lib.mxe_select_fetch(self._h, _p(idx), _p(Hs)), 'mxe_select_fetch')
        return idx, Hs

    def select3_launch(self, linefit_deg=0, gamma=0.2):
        """line fit, chi2 curvature and entropy analyzers of every scan of the last launch, on the ctx stream"""
        self._check(self._lib.mxe_select3_launch(self._h, int(linefit_deg), float(gamma)), 'mxe_select3_launch')

    def select3_fetch(self, want_H=True):
        """(indices [3][n_chain], rows [3][n_chain][n_omega]) of the three analyzers, one copy"""
        idx = np.empty((3, self._n_chain), dtype=np.int32)
        Hs = np.empty((3, self._n_chain, self.n_omega)) if want_H else None
        self._check(self._lib.mxe_select3_fetch(self._h, _p(idx), _p(Hs)), 'mxe_select3_fetch')
        return idx, Hs

    def select3_arrays(self, count=1):
        """uninitialised destinations of :meth:`select3_fetch_rows`: indices [3][n_chain], rows [count][n_chain][n_omega]
        (page-locked when large: one DMA)"""
        return np.empty((3, self._n_chain), dtype=np.int32), pinned_empty((count, self._n_chain, self.n_omega))

    def select3_fetch_rows(self, first=0, count=1, idx=None, rows=None, want_index=True):
        """``mxe_select3_fetch_rows``: the indices of all three analyzers (``want_index``) and the rows of analyzers
        ``first`` .. ``first + count - 1`` -- the others stay on the device until the next selection"""
        if want_index and idx is None:
            idx = np.empty((3, self._n_chain), dtype=np.int32)
        if rows is None and count > 0:
            rows = pinned_empty((count, self._n_chain, self.n_omega))
        if rows is not None and rows.shape != (count, self._n_chain, self.n_omega):
            raise ValueError('rows of another launch')
        self._check(self._lib.mxe_select3_fetch_rows(self._h, _p(idx) if want_index else None, int(first), int(count),
                                                     _p(rows) if count > 0 else None), 'mxe_select3_fetch_rows')
        return idx, rows

    def fetch_rows(self, problem_index):
        pi = _c(np.atleast_1d(problem_index), np.int32)
        out = np.empty((len(pi), self.n_omega))
        self._check(self._lib.mxe_fetch_rows(self._h, len(pi), _p(pi), _p(out)), 'mxe_fetch_rows')
        return out

    def compact_count(self):
        """doubles of the compact result pack of the staged chains (mxe_gather)"""
        P = self._n_chain * self._n_alpha
        return 3 * P + self._n_chain * (self.n_omega + 1)

    def full_count(self):
        return self._n_chain * self._n_alpha * self.n_omega + self.compact_count()

    # -- ranks in separate processes -----------------------------------------
    def comm_init(self, n_ranks, rank, unique_id):
        self._check(self._lib.mxe_comm_init(self._h, int(n_ranks), int(rank), bytes(unique_id)), 'mxe_comm_init')

    def comm_set_loopback(self, on=True):
        """one-GPU test plumbing: the root's own pack through ncclSend / ncclRecv to itself, ncclAllReduce with one rank"""
        self._check(self._lib.mxe_comm_set_loopback(self._h, 1 if on else 0), 'mxe_comm_set_loopback')

    def comm_destroy(self):
        self._check(self._lib.mxe_comm_destroy(self._h), 'mxe_comm_destroy')

    def gather(self, root, counts, full=False, recv=None):
        counts = _c(counts, np.int64)
        self._check(self._lib.mxe_gather(self._h, int(root), 1 if full else 0, _p(counts), _p(recv)), 'mxe_gather')
        return recv

    def allreduce(self, values, op='sum'):
        x = _c(np.atleast_1d(values))
        self._check(self._lib.mxe_comm_allreduce(self._h, _p(x), len(x), 0 if op == 'sum' else 1), 'mxe_comm_allreduce')
        return x

    def apply_output_map(self, B):
        B = _c(B).reshape(self.n_omega, self.n_omega)
        A = np.empty((self._n_chain, self._n_alpha, self.n_omega))
        self._check(self._lib.mxe_apply_output_map(self._h, _p(B), _p(A)),
                    'mxe_apply_output_map')
        return A

    def last_kernel_ms(self):
        ms = ctypes.c_float(0)
        self._check(self._lib.mxe_last_kernel_ms(self._h, ctypes.byref(ms)),
                    'mxe_last_kernel_ms')
        return float(ms.value)

    def timing_mark(self):
        self._check(self._lib.mxe_timing_mark(self._h), 'mxe_timing_mark')

    def ms_since_mark(self):
        ms = ctypes.c_float(0)
        self._check(self._lib.mxe_ms_since_mark(self._h, ctypes.byref(ms)), 'mxe_ms_since_mark')
        return float(ms.value)

    def stream_handle(self):
        return int(self._lib.mxe_stream(self._h) or 0)

    def last_launch_info(self):
        a, b, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        self._check(self._lib.mxe_last_launch_info(self._h, ctypes.byref(a),
                                                   ctypes.byref(b),
                                                   ctypes.byref(c)),
                    'mxe_last_launch_info')
        return dict(waves_per_chain=a.value, n_workgroups=b.value,
                    lds_bytes=c.value,
                    kernel=self._lib.mxe_last_kernel_name(self._h).decode())

    def schedule_info(self):
        """``mxe_schedule_info``: dict(n_solo, placement_rule) of the staged chains (placement_rule 0: not needed, 1: probed and
        holds, 2: does not hold -- no solo workgroups)"""
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        self._check(self._lib.mxe_schedule_info(self._h, ctypes.byref(a), ctypes.byref(b)), 'mxe_schedule_info')
        return dict(n_solo=a.value, placement_rule=b.value)

    def launch_depth(self):
        """``mxe_launch_depth``: rounds of the deepest workgroup and the mean over the workgroups of the last lock-step launch,
        per pass: dict(max_rounds=[a, b], mean_rounds=[a, b])"""
        mx, mean = np.zeros(2, dtype=np.int32), np.zeros(2)
        self._check(self._lib.mxe_launch_depth(self._h, _p(mx), _p(mean)), 'mxe_launch_depth')
        return dict(max_rounds=[int(mx[0]), int(mx[1])], mean_rounds=[float(mean[0]), float(mean[1])])

    def set_result_buffer(self, which):
        self._check(self._lib.mxe_set_result_buffer(self._h, int(which)),
                    'mxe_set_result_buffer')

    def result_device_ptrs(self):
        ptrs = [_vp(None) for _ in range(7)]
        self._check(self._lib.mxe_result_device_ptrs(
            self._h, *[ctypes.byref(x) for x in ptrs]),
            'mxe_result_device_ptrs')
        names = ['H', 'chi2', 'S', 'Q', 'v', 'n_iter', 'converged']
        return dict(zip(names, [x.value for x in ptrs]))
