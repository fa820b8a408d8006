"""Several ranks of one process through the C entry points of the multi-GPU path.  The test
box has one GPU: two contexts on device 0 stand for two devices -- same sharding, staging, launches and
gather call (``mxe_gather_local``), with device copies where distinct devices would use RCCL send / recv.
N > 1 distinct devices are not available to the tests and remain unmeasured."""
import numpy as np
import pytest

import maxent_amd as mx
from maxent_amd import device, synthetic
from maxent_amd.batch_solver import BatchSolver, LazyH

pytestmark = pytest.mark.gpu


def job(n_orb=3, n_tau=60, n_omega=120, n_alpha=12, use_hermiticity=False, **kw):
    tau, omega, K, Gmat, _ = synthetic.matrix_G(n_orb, n_tau, n_omega)
    ew = mx.ElementwiseMaxEnt(use_hermiticity=use_hermiticity, **kw)
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    ew.set_G_tau_data(tau, Gmat)
    ew.omega = omega
    ew.alpha_mesh = mx.LogAlphaMesh(alpha_min=1e-1, alpha_max=1e3, n_points=n_alpha)
    ew.set_error(synthetic.SIGMA)
    return ew


def test_two_ranks_on_one_device_equal_one_rank():
    one = job().run()
    two_job = job(device_ids=(0, 0))
    two = two_job.run()
    assert len(two_job.last_launches[-1]['devices']) == 2
    for name in ('chi2', 'S', 'Q', 'H', 'A', 'A_out', 'v'):
        a, b = np.asarray(getattr(one, name)), np.asarray(getattr(two, name))
        assert a.shape == b.shape
        # the pieces of the alpha scans are cut per launch: answers agree to the solver's tolerance
        assert np.max(np.abs(a - b)) <= 1e-7 * np.max(np.abs(a)), name
    for i in range(3):
        for j in range(3):
            for an in ('LineFitAnalyzer', 'Chi2CurvatureAnalyzer'):
                assert one.analyzer_results[i][j][an]['alpha_index'] == two.analyzer_results[i][j][an]['alpha_index']


def test_gather_brings_every_ranks_pack_and_the_device_linefit_agrees_with_the_host():
    tau, omega, K, Gmat, _ = synthetic.matrix_G(3, 60, 120)
    K.reduce_singular_space(1e-14)
    D = synthetic.flat_D(omega)
    from maxent_amd import hostprep
    alphas = np.array(mx.LogAlphaMesh(alpha_min=1e-1, alpha_max=1e3, n_points=12)) * 60
    specs = []
    for i in range(3):
        for j in range(3):
            kind = device.ENTROPY_NORMAL if i == j else device.ENTROPY_PLUSMINUS
            specs.append(dict(G=Gmat[i, j], err=synthetic.SIGMA * np.ones(60), U_rot=None, D=D, kind=kind,
                              v0=hostprep.initial_v(K.V, D, omega.delta, kind), alpha=alphas))
    opts = mx.LevenbergMinimizer().to_opts()
    solo = BatchSolver(K, (0,))
    ref, _ = solo.solve(K, specs, opts, want_H=True)
    trio = BatchSolver(K, (0, 0, 0))
    got, info = trio.solve(K, specs, opts)
    assert info['devices'] == [0, 0, 0]
    from maxent_amd.analyzers import fit_piecewise
    assert all(isinstance(b['H'], LazyH) and not b['H'].on_host for b in got)      # nothing of H has moved yet
    for e, (a, b) in enumerate(zip(ref, got)):
        np.testing.assert_allclose(b['chi2'], a['chi2'], rtol=1e-7)
        idx, _ = fit_piecewise(np.log(alphas), np.log(b['chi2']))
        assert b['device_linefit_index'] == idx, e
        # the row the gather brought is the H of that alpha; a single-row fetch and the full fetch agree
        row = b['H'][idx]
        assert np.array_equal(row, b['device_linefit_H'])
        if e >= 6:           # the last element of every rank: now the full fetch (of the rank's whole shard)
            assert np.array_equal(np.asarray(b['H'])[idx], row) and b['H'].on_host
        assert np.max(np.abs(np.asarray(b['H']) - np.asarray(a['H']))) <= 1e-7 * np.max(np.abs(np.asarray(a['H'])))
    solo.close()
    trio.close()


def test_contexts_are_kept_between_runs_and_dropped_when_the_kernel_changes():
    ew = job()
    ew.run()
    K = ew.maxent_diagonal.K
    first = K._batch_solvers[(0,)]
    ew.maxent_result = None
    ew.run()
    assert K._batch_solvers[(0,)] is first
    ew.omega = mx.HyperbolicOmegaMesh(-8, 8, 100)      # refills the kernel: new decomposition, new context
    ew.maxent_result = None
    res = ew.run()
    K = ew.maxent_diagonal.K
    assert K._batch_solvers[(0,)] is not first and res.A.shape[-1] == 100


def test_a_new_object_on_the_same_grids_takes_over_the_contexts_unless_results_are_still_out():
    """BatchSolver.for_kernel: an equal decomposition (contents) finds the pooled solver; results that somebody still
    holds unfetched are not disturbed -- the next object then gets contexts of its own"""
    a = job()
    res_a = a.run()
    solver_a = a.maxent_diagonal.K._batch_solvers[(0,)]
    H_a = np.array(job().run().H)                    # (reference values, from yet another object)
    A_out_a = np.array(res_a.A_out)
    # results of a are out (H still on the device): b must not take a's contexts
    b = job()
    res_b = b.run()
    solver_b = b.maxent_diagonal.K._batch_solvers[(0,)]
    assert solver_b is not solver_a
    assert np.array_equal(np.asarray(res_a.H), H_a)
    # with everything fetched or dropped the next object takes over -- and solves other data correctly
    res_a = res_b = None
    tau, omega, K, Gmat, _ = synthetic.matrix_G(3, 60, 120)
    c = job()
    c.set_G_tau_data(tau, 1.5 * Gmat)
    res_c = c.run()
    assert c.maxent_diagonal.K._batch_solvers[(0,)] in (solver_a, solver_b)
    keep, BatchSolver.POOL_SIZE = BatchSolver.POOL_SIZE, 0
    try:
        d = job()
        d.set_G_tau_data(tau, 1.5 * Gmat)
        res_d = d.run()
        assert d.maxent_diagonal.K._batch_solvers[(0,)] not in (solver_a, solver_b)
    finally:
        BatchSolver.POOL_SIZE = keep
    for name in ('chi2', 'S', 'H', 'A_out'):
        assert np.array_equal(np.asarray(getattr(res_c, name)), np.asarray(getattr(res_d, name))), name
    assert not np.allclose(np.asarray(res_c.A_out), A_out_a)


def test_process_ranks_comm_with_one_rank():
    """the entry points a one-process-per-GPU launcher uses (bench.py --gpus N), with the single rank this box has"""
    tau, omega, K, G = synthetic.single_G(40, 80)
    K.reduce_singular_space(1e-14)
    ctx = device.DeviceContext(K.U, K.S, K.V)
    ds = ctx.add_dataset(synthetic.SIGMA * np.ones(40))
    D = synthetic.flat_D(omega)
    ctx.set_elements([ds], [G], D[np.newaxis, :], [device.ENTROPY_NORMAL])
    from maxent_amd import hostprep
    alphas = np.array([100.0, 10.0, 1.0, 0.5, 0.2, 0.1]) * 40
    ctx.upload_chains([0], alphas, hostprep.initial_v(K.V, D, omega.delta, device.ENTROPY_NORMAL)[np.newaxis, :])
    ctx.comm_init(1, 0, device.comm_unique_id())
    ctx.launch()
    ctx.select_launch(0)
    recv = np.empty(ctx.compact_count())
    ctx.gather(0, [ctx.compact_count()], recv=recv)
    out = ctx.fetch()
    assert np.array_equal(recv[:6], out['chi2'][0]) and np.array_equal(recv[12:18], out['Q'][0])
    idx, Hs = ctx.select_fetch()
    assert recv[-1] == idx[0] and np.array_equal(recv[18:18 + 80], out['H'][0, idx[0]])
    assert ctx.allreduce([3.0], 'max')[0] == 3.0
    full = np.empty(ctx.full_count())
    ctx.gather(0, [ctx.full_count()], full=True, recv=full)
    assert np.array_equal(full[:6 * 80].reshape(6, 80), out['H'][0])
    ctx.comm_destroy()
    ctx.close()


def test_the_region_with_steps_in_flight_and_a_communicator_per_context_runs_through_rccl_in_loop_back(monkeypatch):
    """``bench.in_flight_comm_region`` itself -- what ``bench.py --gpus N --in-flight-comm n`` runs on every rank: n contexts per rank,
    cut for n steps in flight, a communicator EACH (all made before the first launch, timed apart), the steps taken in turn with a
    gather on the context's stream behind every one -- with the one rank this box has: the packs go through ncclSend / ncclRecv to
    the rank itself, the settling passes through ncclAllReduce (loop-back).  VERDICT r04: only tools/ and hand runs covered it."""
    import bench
    monkeypatch.setenv('MASTER_PORT', '29431')
    batch = bench.build_batch(4, 100, 200, 20, 0)
    mine = list(range(16))
    n_alpha, n_omega = 20, 200

    class Args(object):
        waves_per_chain = chains_per_wg = alpha_split = wg_per_cu = 0
        warmup, steps = 2, 9
    counts = [3 * len(mine) * n_alpha + len(mine) * (n_omega + 1)]
    elapsed, check, t_comm = bench.in_flight_comm_region(batch, mine, 0, 0, 1, counts, False, Args, 3)
    assert elapsed > 0 and t_comm > 0
    assert check['converged'] == check['alpha_solves'] == len(mine) * n_alpha and check['left_to_finish'] == 0
    assert check['audit_max'] < 1e-6 and 'chain_kernel' in check['kernel']


def test_the_rccl_calls_of_the_gather_execute_with_one_rank():
    """no ncclSend / ncclRecv / ncclAllReduce had ever run.  With the loopback switch the ONE rank of
    this box sends its pack to itself inside ncclGroupStart / ncclGroupEnd and all-reduces with itself: the gathered
    pack must equal the source, compact and full, and the reductions must return their input."""
    tau, omega, K, G = synthetic.single_G(40, 80)
    K.reduce_singular_space(1e-14)
    ctx = device.DeviceContext(K.U, K.S, K.V)
    ds = ctx.add_dataset(synthetic.SIGMA * np.ones(40))
    D = synthetic.flat_D(omega)
    ctx.set_elements([ds, ds], [G, 0.5 * G], np.tile(D, (2, 1)), [device.ENTROPY_NORMAL, device.ENTROPY_NORMAL])
    from maxent_amd import hostprep
    alphas = np.array([100.0, 10.0, 1.0, 0.5, 0.2, 0.1]) * 40
    v0 = hostprep.initial_v(K.V, D, omega.delta, device.ENTROPY_NORMAL)
    ctx.upload_chains([0, 1], alphas, np.stack([v0, v0]))
    with pytest.raises(device.MaxEntDeviceError):
        ctx.comm_set_loopback(True)                 # no communicator yet
    ctx.comm_init(1, 0, device.comm_unique_id())
    ctx.comm_set_loopback(True)
    ctx.launch()
    ctx.select_launch(0)
    out = ctx.fetch()
    idx, Hs = ctx.select_fetch()
    for rep in range(3):                            # (several gathers on one communicator, as bench.py enqueues them)
        recv = np.full(ctx.compact_count(), np.nan)
        ctx.gather(0, [ctx.compact_count()], recv=recv)
        assert np.array_equal(recv[:12], out['chi2'].ravel()) and np.array_equal(recv[12:24], out['S'].ravel())
        assert np.array_equal(recv[36:36 + 2 * 80].reshape(2, 80), Hs) and np.array_equal(recv[-2:], idx)
    full = np.full(ctx.full_count(), np.nan)
    ctx.gather(0, [ctx.full_count()], full=True, recv=full)
    assert np.array_equal(full[:12 * 80].reshape(2, 6, 80), out['H'])
    assert np.array_equal(full[12 * 80:], recv)
    assert ctx.allreduce([3.0, -1.5], 'max').tolist() == [3.0, -1.5]
    assert ctx.allreduce([3.0, -1.5], 'sum').tolist() == [3.0, -1.5]
    ctx.comm_set_loopback(False)
    again = np.empty(ctx.compact_count())
    ctx.gather(0, [ctx.compact_count()], recv=again)
    assert np.array_equal(again, recv)
    ctx.comm_destroy()
    ctx.close()


def test_chi2_factor_reaches_the_gathered_Q():
    """with several devices Q came from the raw pack, which holds Q / chi2_factor"""
    def run(**kw):
        ew = job(**kw)
        for tm in (ew.maxent_diagonal, ew.maxent_offdiagonal):
            tm.cost_function.chi2_factor = 2.5
        return ew.run()
    one, two = run(), run(device_ids=(0, 0))
    for name in ('chi2', 'S', 'Q'):
        a, b = np.asarray(getattr(one, name)), np.asarray(getattr(two, name))
        assert np.max(np.abs(a - b)) <= 1e-7 * np.max(np.abs(a)), name
    Q, al = np.asarray(two.Q), np.asarray(two.alpha)
    assert np.allclose(Q, 0.5 * 2.5 * np.asarray(two.chi2) - np.broadcast_to(al, Q.shape) * np.asarray(two.S), rtol=1e-9)


def test_devices_of_one_process_are_driven_from_threads():
    """stage / launch / finish / fetch of the ranks ran one after the other on one Python thread.  Four
    contexts on the one device: same results as one context, wall time of the solve below 1.3 x the single context's
    plus what four times the staging costs on ONE device (on distinct devices the launches overlap as well)."""
    import time
    tau, omega, K, Gmat, _ = synthetic.matrix_G(8, 200, 500)
    K.reduce_singular_space(1e-14)
    D = synthetic.flat_D(omega)
    from maxent_amd import hostprep
    alphas = np.array(mx.LogAlphaMesh(alpha_min=1e-2, alpha_max=1e4, n_points=100)) * 200
    specs = []
    for i in range(8):
        for j in range(8):
            kind = device.ENTROPY_NORMAL if i == j else device.ENTROPY_PLUSMINUS
            specs.append(dict(G=Gmat[i, j], err=synthetic.SIGMA * np.ones(200), U_rot=None, D=D, kind=kind,
                              v0=hostprep.initial_v(K.V, D, omega.delta, kind), alpha=alphas))
    opts = mx.LevenbergMinimizer().to_opts()
    solo, quad = BatchSolver(K, (0,)), BatchSolver(K, (0, 0, 0, 0))
    walls = {}
    for name, s in (('solo', solo), ('quad', quad)):
        s.solve(K, specs, opts)
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            res, info = s.solve(K, specs, opts)
            t.append(time.perf_counter() - t0)
        walls[name] = (min(t), res)
    for a, b in zip(walls['solo'][1], walls['quad'][1]):
        assert np.max(np.abs(a['chi2'] - b['chi2'])) <= 1e-7 * np.max(np.abs(a['chi2']))
        assert a['converged'].all() and b['converged'].all()
    print('solve wall: one context %.2f ms, four contexts on threads %.2f ms' % (1e3 * walls['solo'][0], 1e3 * walls['quad'][0]))
    # (a guard against the ranks running one after the other again, with room for a busy box: measured 4.4 against 2.3 ms)
    assert walls['quad'][0] <= 1.5 * walls['solo'][0] + 4e-3
    solo.close()
    quad.close()


GOLDEN = __import__('os').path.join(__import__('os').path.dirname(__import__('os').path.abspath(__file__)), 'golden')


@pytest.mark.parametrize('name', ['cfg1_normal', 'cfg1_bryan', 'cfg1_plusminus', 'cfg1_tauerr', 'cfg2_normal', 'cfg5_preblur_pm',
                                  'kat_tau_maxent', 'cov'])
def test_device_analyzers_pick_the_alphas_the_host_analyzers_pick_on_the_reference_curves(name):
    """mxe_select3_launch (line fit, chi2 curvature, entropy) on chi2 / S curves of the REFERENCE's own runs, written
    into the result buffers of a launch of the same shape: the indices equal those of the host analyzers (which
    equal the reference's: tests/test_cabi_and_host.py) on every golden that holds a whole scan."""
    from maxent_amd.analyzers import fit_piecewise, curv
    z = np.load(__import__('os').path.join(GOLDEN, name + '.npz'))
    alpha, chi2, S = np.asarray(z['alpha'], float), np.asarray(z['chi2_ref'], float), np.asarray(z['S_ref'], float)
    n = len(alpha)
    rng = np.random.RandomState(5)
    # three scans: the reference curve, one with a NaN in it, one perturbed
    C = np.stack([chi2, chi2 * (1 + 0.05 * rng.rand(n)), chi2])
    Sm = np.stack([S, S * (1 + 0.05 * rng.rand(n)), S])
    C[2, n // 2] = np.nan
    import ctypes
    n_tau, n_w = 30, 40
    tau, omega, K, G = synthetic.single_G(n_tau, n_w)
    K.reduce_singular_space(1e-14)
    ctx = device.DeviceContext(K.U, K.S, K.V)
    ds = ctx.add_dataset(synthetic.SIGMA * np.ones(n_tau))
    D = synthetic.flat_D(omega)
    from maxent_amd import hostprep
    ctx.set_elements([ds] * 3, [G] * 3, np.tile(D, (3, 1)), [device.ENTROPY_NORMAL] * 3)
    v0 = hostprep.initial_v(K.V, D, omega.delta, device.ENTROPY_NORMAL)
    ctx.upload_chains([0, 1, 2], alpha, np.tile(v0, (3, 1)))
    ctx.launch()
    ctx.sync()
    # overwrite chi2 and S of the launch with the curves under test (device pointers of the result pack)
    lib = device.load_library()
    ptrs = [ctypes.c_void_p() for _ in range(7)]
    assert lib.mxe_result_device_ptrs(ctx._h, *[ctypes.byref(p) for p in ptrs]) == 0
    hip = ctypes.CDLL('libamdhip64.so')
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert hip.hipMemcpy(ptrs[1], C.ctypes.data_as(ctypes.c_void_p), C.nbytes, 1) == 0
    assert hip.hipMemcpy(ptrs[2], Sm.ctypes.data_as(ctypes.c_void_p), Sm.nbytes, 1) == 0
    out = ctx.fetch()
    for deg, gamma in ((0, 0.2), (1, 0.35)):
        ctx.select3_launch(deg, gamma)
        idx, rows = ctx.select3_fetch()
        for c in range(3):
            with np.errstate(all='ignore'):
                try:
                    want_fit = fit_piecewise(np.log(alpha), np.log(C[c]), deg)[0]
                except ValueError:
                    want_fit = -1
                cv = curv(gamma * np.log10(alpha), np.log10(C[c]))[0]
                d = np.full(n, np.nan)
                d[1:-1] = (Sm[c, 2:] - Sm[c, :-2]) / (np.log(alpha[2:]) - np.log(alpha[:-2]))
            want_curv = -1 if np.all(np.isnan(cv)) else int(np.nanargmax(cv))
            want_ent = -1 if np.all(np.isnan(d)) else int(np.nanargmin(d ** 2))
            assert (idx[0, c], idx[1, c], idx[2, c]) == (want_fit, want_curv, want_ent), (name, c, deg)
            for a in range(3):
                if idx[a, c] >= 0:
                    assert np.array_equal(rows[a, c], out['H'][c, idx[a, c]])
        # mxe_select3_fetch_rows: any part of the rows, with or without the indices, equals the whole
        for first, count in ((0, 1), (1, 2), (2, 1), (0, 3)):
            i2, r2 = ctx.select3_fetch_rows(first=first, count=count)
            assert np.array_equal(i2, idx) and np.array_equal(r2, rows[first:first + count], equal_nan=True)     # (a scan without a choice: NaN row)
            none, r3 = ctx.select3_fetch_rows(first=first, count=count, want_index=False)
            assert none is None and np.array_equal(r3, r2, equal_nan=True)
        i4, r4 = ctx.select3_fetch_rows(first=0, count=0)
        assert np.array_equal(i4, idx) and r4 is None
    # arguments and state: a part outside the three analyzers, neither indices nor rows, rows of another launch
    for first, count in ((-1, 1), (2, 2), (0, 4)):
        with pytest.raises(device.MaxEntDeviceError):
            ctx.select3_fetch_rows(first=first, count=count)
    with pytest.raises(device.MaxEntDeviceError):
        ctx.select3_fetch_rows(first=0, count=0, want_index=False)
    ctx.upload_chains([0, 1], alpha, np.tile(v0, (2, 1)))       # new chains: what the last selection chose is gone
    ctx.launch()
    ctx.sync()
    with pytest.raises(device.MaxEntDeviceError):
        ctx.select3_fetch_rows(first=1, count=1, want_index=False)
    ctx.select3_launch(0, 0.2)
    assert ctx.select3_fetch_rows(first=1, count=1)[1].shape == (1, 2, n_w)
    ctx.close()


def test_elementwise_result_from_device_picks_equals_host_analyzers():
    """ElementwiseMaxEnt with the alphas picked on the device: A_out and every analyzer's index / A_out equal what
    the host analyzers give on the same solved scans, bit for bit; the lazy extras are there when asked for"""
    ew = job(n_orb=3, n_alpha=20)
    res = ew.run()
    from maxent_amd.analyzers import LineFitAnalyzer, Chi2CurvatureAnalyzer, EntropyAnalyzer, _device_picks
    keys = [(i, j) for i in range(3) for j in range(3)]
    assert _device_picks(res, keys, 0, lambda p: True) is not None
    for an in (LineFitAnalyzer(), Chi2CurvatureAnalyzer(), EntropyAnalyzer()):
        for (i, j) in keys:
            dev = res.analyzer_results[i][j][an.name]
            host = an.analyze(res, (i, j))
            assert dev['alpha_index'] == host['alpha_index']
            assert np.array_equal(np.asarray(dev['A_out']), np.asarray(host['A_out']))
            assert dev['info'] == host['info'] and set(dev.keys()) == set(host.keys())
            for k in host.keys():
                if k in ('curvature', 'dS_dalpha'):
                    np.testing.assert_array_equal(np.asarray(dev[k]), np.asarray(host[k]))
    # another gamma than the device used: the host analyzers take over
    ew2 = job(n_orb=2, n_alpha=20)
    ew2.maxent_diagonal.analyzers = [LineFitAnalyzer(), Chi2CurvatureAnalyzer(gamma=0.5)]
    ew2.maxent_offdiagonal.analyzers = [LineFitAnalyzer(), Chi2CurvatureAnalyzer(gamma=0.5)]
    r2 = ew2.run()
    assert r2.analyzer_results[0][0]['Chi2CurvatureAnalyzer']['gamma'] == 0.5


def test_rows_of_the_other_analyzers_stay_on_the_device_until_somebody_looks():
    """the rows of the result's default analyzer come with the solve, those of the other two device analyzers by
    ``mxe_select3_fetch_rows`` when their A_out is read -- also after the same solver has run another job (they are brought
    to the host before its buffers are overwritten); the default is the first of the three in the analyzer list"""
    from maxent_amd.batch_solver import LazyRows
    from maxent_amd.analyzers import LineFitAnalyzer, Chi2CurvatureAnalyzer, EntropyAnalyzer
    ew = job(n_orb=3, n_alpha=20)
    res = ew.run()
    rows = res._records[(0, 0)]['device_select']['batch'][1]
    assert all(isinstance(r, LazyRows) for r in rows) and [r.on_host for r in rows] == [True, False, False]
    res.A_out                                                    # (the line fit's rows: nothing else moves)
    assert [r.on_host for r in rows] == [True, False, False]
    got = res.analyzer_results[0][1]['Chi2CurvatureAnalyzer']
    assert [r.on_host for r in rows] == [True, True, False]
    # the same object again, on other data: everything the first result still had on the device is brought over first
    tau, omega, K, Gmat, _ = synthetic.matrix_G(3, 60, 120, noise_seed=77)
    ew.set_G_tau_data(tau, 1.3 * Gmat)
    res2 = ew.run()
    assert rows[2].on_host
    A = np.asarray(res.A)
    assert np.array_equal(np.asarray(got['A_out']), A[0, 1, got['alpha_index']])
    for (i, j) in ((i, j) for i in range(3) for j in range(3)):
        e = res.analyzer_results[i][j]['EntropyAnalyzer']
        assert np.array_equal(np.asarray(e['A_out']), A[i, j, e['alpha_index']])
    A2 = np.asarray(res2.A)
    assert all(r.on_host for r in res2._records[(0, 0)]['device_select']['batch'][1])       # (they came with H)
    e2 = res2.analyzer_results[1][1]['EntropyAnalyzer']
    assert np.array_equal(np.asarray(e2['A_out']), A2[1, 1, e2['alpha_index']]) and not np.array_equal(A2, A)
    # another default analyzer: its rows are the ones that come with the solve
    ew3 = job(n_orb=2, n_alpha=20)
    ew3.maxent_diagonal.analyzers = [Chi2CurvatureAnalyzer(), LineFitAnalyzer(), EntropyAnalyzer()]
    ew3.maxent_offdiagonal.analyzers = [Chi2CurvatureAnalyzer(), LineFitAnalyzer(), EntropyAnalyzer()]
    r3 = ew3.run()
    rows3 = r3._records[(0, 0)]['device_select']['batch'][1]
    assert [r.on_host for r in rows3] == [False, True, False]
    c3 = r3.analyzer_results[0][1]['Chi2CurvatureAnalyzer']
    assert np.array_equal(r3.A_out[0, 1], np.asarray(c3['A_out']))
    assert np.array_equal(np.asarray(c3['A_out']), np.asarray(r3.A)[0, 1, c3['alpha_index']])
    l3 = r3.analyzer_results[1][0]['LineFitAnalyzer']
    assert np.array_equal(np.asarray(l3['A_out']), np.asarray(r3.A)[1, 0, l3['alpha_index']]) and rows3[0].on_host


def test_result_arrays_of_a_full_matrix_are_views_of_what_came_off_the_device():
    """ElementwiseMaxEnt launches its scans in the order of the result's matrix and MaxEntResult assembles H as a view of
    the ONE fetched array (A = H / delta in one division); the values are those of the element-by-element assembly, and a
    result with mirrored elements (use_hermiticity) goes the general way"""
    from maxent_amd.maxent_result import MaxEntResult
    res = job().run()
    H = res.H
    rec = res._records[(1, 2)]
    assert np.shares_memory(H, np.asarray(rec['H'])) and np.array_equal(H[1, 2], np.asarray(rec['H']))
    got = {name: np.array(getattr(res, name)) for name in ('H', 'A', 'chi2', 'S', 'v', 'A_out')}
    res2 = job().run()
    orig = MaxEntResult._assemble_whole
    MaxEntResult._assemble_whole = lambda self, *a: None
    try:
        for name in ('H', 'A', 'chi2', 'S', 'v', 'A_out'):
            assert np.array_equal(got[name], np.asarray(getattr(res2, name))), name
    finally:
        MaxEntResult._assemble_whole = orig
    herm = job(use_hermiticity=True).run()
    assert herm.H.shape == H.shape and np.array_equal(herm.H[2, 0], herm.H[0, 2])
    assert np.max(np.abs(herm.H[0, 2] - H[0, 2])) <= 1e-7 * np.max(np.abs(H[0, 2]))


def test_page_locked_result_blocks_come_from_a_pool_and_go_back_with_the_last_view():
    """device.pinned_empty (mxe_host_alloc): an ordinary writable array; the block returns to the library's pool when the last
    view of it is gone and the next request of that size takes it again; small requests are plain numpy arrays"""
    import gc
    a = device.pinned_empty((300, 1000))
    a[:] = 3.0
    addr = a.__array_interface__['data'][0]
    view = a[5]
    del a
    gc.collect()
    assert view[7] == 3.0                                      # the view keeps the block
    b = device.pinned_empty((300, 1000))
    assert b.__array_interface__['data'][0] != addr            # ... so another block was pinned
    del view, b
    gc.collect()
    c = device.pinned_empty((300, 1000))
    assert c.__array_interface__['data'][0] in (addr,) or c.nbytes == 2400000      # taken from the pool (either of the two)
    small = device.pinned_empty((10, 10))
    assert small.shape == (10, 10) and small.flags.owndata
    # a fetch into such a block and into pageable memory give the same bytes
    ew = job()
    res = ew.run()
    ctx = ew.maxent_diagonal.K._batch_solvers[(0,)].ctxs[0]
    H1 = ctx.fetch(want_v=False, want_H=True)['H']
    lib = device.load_library()
    H2 = np.empty(H1.shape)
    assert lib.mxe_chains_fetch(ctx._h, None, device._p(H2), None, None, None, None, None, None) == 0
    assert np.array_equal(H1, H2)


@pytest.mark.parametrize('herm,cplx,ids', [(False, False, None), (True, False, None), (False, True, None), (True, True, None),
                                           (False, False, (0, 0)), (True, True, (0, 0))])
def test_elementwise_variants_assemble_the_same_arrays_every_way(herm, cplx, ids):
    """hermiticity x complex elements x two contexts: the result arrays through the whole-array assembly (views of the
    fetched block where the launch order allows), through the element-by-element assembly and from a run with contexts
    of its own are the same bits; every record equals its slice"""
    from maxent_amd.maxent_result import MaxEntResult
    n_orb = 3
    tau, omega, K, Gmat, _ = synthetic.matrix_G(n_orb, 40, 60, seed=11)
    if cplx:
        G2 = synthetic.matrix_G(n_orb, 40, 60, seed=12)[3]
        sgn = np.sign(np.arange(n_orb)[None, :] - np.arange(n_orb)[:, None]).astype(float)
        Gmat = Gmat + 0.3j * sgn[:, :, None] * G2                # hermitian in the orbital indices

    def run():
        ew = mx.ElementwiseMaxEnt(use_hermiticity=herm, use_complex=cplx, device_ids=ids)
        ew.set_verbosity(mx.VerbosityFlags.Quiet)
        ew.set_G_tau_data(tau, Gmat)
        ew.omega = omega
        ew.alpha_mesh = mx.LogAlphaMesh(alpha_min=1e-1, alpha_max=1e3, n_points=9)
        ew.set_error(synthetic.SIGMA)
        return ew.run()
    res = run()
    names = ('H', 'A', 'chi2', 'S', 'Q', 'A_out')
    got = {name: np.array(getattr(res, name)) for name in names}
    assert np.all(np.isfinite(got['A_out'])) and got['A_out'].shape == (n_orb, n_orb, 60)
    assert np.iscomplexobj(got['A_out']) == cplx
    for key, rec in res._records.items():
        assert np.array_equal(np.asarray(rec['H']), got['H'][key]) and np.array_equal(np.asarray(rec['chi2']), got['chi2'][key])
    orig = MaxEntResult._assemble_whole
    MaxEntResult._assemble_whole = lambda self, *a: None
    try:
        res2 = run()
        for name in names:
            assert np.array_equal(np.asarray(getattr(res2, name)), got[name], equal_nan=True), name
    finally:
        MaxEntResult._assemble_whole = orig
    keep, BatchSolver.POOL_SIZE = BatchSolver.POOL_SIZE, 0
    try:
        res3 = run()
        for name in names:
            assert np.array_equal(np.asarray(getattr(res3, name)), got[name], equal_nan=True), name
    finally:
        BatchSolver.POOL_SIZE = keep


def test_bench_main_with_the_communicator_path_in_loop_back():
    """``python bench.py --force-comm``: main()'s multi-rank path -- communicator through the id file, the steps with a gather behind
    every one, barriers and the maximum over the ranks through ncclAllReduce, rank 0's self-check of what it gathered -- as a process of
    its own with the one rank this box has (the packs go to the rank itself).  The first run between two GPUs starts from here."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_PORT='29437')
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--full', '--force-comm', '--no-cpu-baseline', '--no-extras',
                        '--steps', '6', '--warmup', '2', '--n-orb', '4', '--n-tau', '100', '--n-omega', '200', '--n-alpha', '20'],
                       capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    assert line['value'] > 0 and line['n_gpus'] == 1 and line['steps'] == 6 and line['watchdog_fired'] is False
    assert line['config']['gather_checked'] is True
    assert line['config']['converged_on_rank0'] == line['config']['problems_on_rank0'] == 16 * 20
