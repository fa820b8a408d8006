"""The queue counter of the lock-step launches has no reset node: launch k draws from word k & 1 of a pair and stores the start
value of launch k + 1 into the other word (MCExtra::counter).  A launch that found its word unarmed would take no
piece and leave the result buffers as they were, so every launch here is preceded, on the context's stream, by a fill of the
scalar results with 0xFF bytes (NaN, negative counts)."""
import ctypes

import numpy as np
import pytest

from maxent_amd import device, hostprep, synthetic

pytestmark = pytest.mark.gpu

FIELDS = ('v', 'H', 'chi2', 'S', 'Q', 'n_iter', 'n_evals', 'converged')
N_TAU, N_OMEGA, N_ALPHA = 120, 96, 12


@pytest.fixture(scope='module')
def job():
    tau, omega, K, Gmat, _ = synthetic.matrix_G(3, N_TAU, N_OMEGA)
    K.reduce_singular_space(1e-14)
    D = synthetic.flat_D(omega)
    elems = [(i, j) for i in range(3) for j in range(3)]
    kinds = [device.ENTROPY_NORMAL if i == j else device.ENTROPY_PLUSMINUS for i, j in elems]
    v0 = np.stack([hostprep.initial_v(K.V, D, omega.delta, k) for k in kinds])
    alphas = np.array(synthetic.alpha_mesh(N_ALPHA)) * N_TAU
    hip = ctypes.CDLL('libamdhip64.so')
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]

    def context():
        ctx = device.DeviceContext(K.U, K.S, K.V)
        ds = ctx.add_dataset(synthetic.SIGMA * np.ones(N_TAU))
        ctx.set_elements([ds] * 9, [Gmat[i, j] for i, j in elems], np.tile(D, (9, 1)), kinds)
        return ctx

    def upload(ctx, scans):
        # the lock-step kernel itself, not the binary32 first pass of a launch that does not fill the GPU (its two words keep
        # their reset node)
        ctx.upload_chains(np.asarray(scans, dtype=np.int32), alphas, v0[list(scans)],
                          device.default_opts(chains_per_wg=4, alpha_split=4, lds_basis=2))

    def wipe(ctx, n_scan):
        p = ctx.result_device_ptrs()
        P = n_scan * N_ALPHA
        assert hip.hipMemsetAsync(p['chi2'], 0xFF, 3 * P * 8, ctx.stream_handle()) == 0
        assert hip.hipMemsetAsync(p['n_iter'], 0xFF, P * 4, ctx.stream_handle()) == 0

    def takes_the_queue(ctx, n_scan):
        info, sched, depth = ctx.last_launch_info(), ctx.schedule_info(), ctx.launch_depth()
        assert 'chain_kernel_mc<32, ' in info['kernel'] and 'chain_kernel_lv' not in info['kernel'], info
        # one data set: a persistent grid whose slots draw their pieces, the first ones too, from the queue (no solo workgroups,
        # which take their first pieces by position)
        assert sched['n_solo'] == 0 and info['n_workgroups'] < n_scan * N_ALPHA, (info, sched)
        assert depth['max_rounds'][0] > 0, depth           # (written by the workgroups of a launch with a queue only: mxe_launch_depth)

    def fresh(scans):
        ctx = context()
        upload(ctx, scans)
        wipe(ctx, len(scans))
        ctx.launch()
        out = ctx.fetch()
        takes_the_queue(ctx, len(scans))
        ctx.close()
        ok = out['converged'] != 0
        assert ok.mean() > 0.9 and np.all(np.isfinite(out['chi2'][ok])) and out['n_iter'][ok].min() > 0
        return out

    return dict(context=context, upload=upload, wipe=wipe, fresh=fresh, takes_the_queue=takes_the_queue)


def same(out, ref):
    for k in FIELDS:
        assert np.array_equal(out[k], ref[k], equal_nan=True), k


def test_three_launches_back_to_back_then_another_upload_equal_a_fresh_context(job):
    """three launches enqueued without a sync, then a fetch: every field bit for bit what a fresh context gives after one launch;
    the same after re-uploading a different number of scans on the same context"""
    all9, five = list(range(9)), [0, 4, 8, 1, 5]
    ref9, ref5 = job['fresh'](all9), job['fresh'](five)
    ctx = job['context']()
    job['upload'](ctx, all9)
    for _ in range(3):
        job['wipe'](ctx, 9)
        ctx.launch()
    same(ctx.fetch(), ref9)
    job['takes_the_queue'](ctx, 9)
    job['upload'](ctx, five)
    for _ in range(2):
        job['wipe'](ctx, 5)
        ctx.launch()
    same(ctx.fetch(), ref5)
    job['takes_the_queue'](ctx, 5)
    job['upload'](ctx, all9)
    job['wipe'](ctx, 9)
    ctx.launch()
    same(ctx.fetch(), ref9)
    ctx.close()


def test_a_launch_behind_one_that_counted_its_rounds_equals_a_fresh_context(job, monkeypatch):
    """MXE_COUNT_ROUNDS selects another build of the kernel for one launch: it re-arms the next launch like any other"""
    scans = list(range(9))
    ref = job['fresh'](scans)
    ctx = job['context']()
    job['upload'](ctx, scans)
    monkeypatch.setenv('MXE_COUNT_ROUNDS', '1')
    job['wipe'](ctx, 9)
    ctx.launch()
    ctx.sync()
    monkeypatch.delenv('MXE_COUNT_ROUNDS')
    same(ctx.fetch(), ref)
    for _ in range(2):
        job['wipe'](ctx, 9)
        ctx.launch()
    same(ctx.fetch(), ref)
    job['takes_the_queue'](ctx, 9)
    ctx.close()
