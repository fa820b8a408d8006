"""Element-wise MaxEnt for matrix-valued G(tau): the batching boundary.

``ElementwiseMaxEnt`` / ``DiagonalMaxEnt`` / ``PoormanMaxEnt`` keep the
reference's surface and semantics (reference python/elementwise_maxent.py:
58-653): two workers -- diagonal elements with the normal entropy,
off-diagonal ones with the plus-minus entropy --, attribute shadowing onto
both, hermiticity shortcut (i > j skipped), real and imaginary parts as
separate real problems, per-element errors or covariances, and Poorman's
default model D_ij = sqrt(A_ii A_jj) + eps from the analyzed diagonals.

What is different is the execution: the reference runs the elements one after
the other, each with a fresh kernel fill and SVD.  Here
``run_diagonal`` and ``run_offdiagonal`` each collect the alpha scans of all
their elements and hand them to the device as ONE launch of the chain kernel
(one chain per element, :func:`maxent_amd.maxent_loop.solve_elements`); the
kernel matrix is filled and decomposed once.  Poorman's method keeps its
ordering constraint: diagonals (including their analyzers) finish before the
off-diagonal launch is assembled.
"""

from datetime import datetime

import numpy as np

from . import kernels
from .default_models import DataDefaultModel
from .logtaker import VerbosityFlags
from .maxent_loop import solve_elements, select_params
from .maxent_result import MaxEntResult
from .tau_maxent import TauMaxEnt


class CallableMethodCheck(object):
    """call the same method on both workers; the results must agree."""

    def __init__(self, name, fun1, fun2):
        self.name, self.fun1, self.fun2 = name, fun1, fun2

    def __call__(self, *args, **kwargs):
        r1 = self.fun1(*args, **kwargs)
        r2 = self.fun2(*args, **kwargs)
        if np.all(r1 == r2):
            return r1
        raise Exception('Element {n} not uniquely defined. Use '
                        'self.maxent_diagonal.{n} or '
                        'self.maxent_offdiagonal.{n}!'.format(n=self.name))


class _LazySpecs(object):
    """the specs of the elements of a batch cut from ONE data array (``_prepare_batch``, direct input): the first element's
    spec as the worker made it, then copies of one template that differ in their data rows -- each made when it is asked for
    (a launch that is staged from the arrays and whose records nobody looks at never asks)"""

    def __init__(self, first_spec, template, g_rows, rest):
        self._first, self._template, self._g, self._rest = first_spec, template, g_rows, rest
        self._lead = 0 if first_spec is None else 1
        self._made = {}

    def __len__(self):
        return self._lead + len(self._rest)

    def __bool__(self):
        return len(self) > 0

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        i = int(i)
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        if i < self._lead:
            return self._first
        k = i - self._lead
        if k == 0:
            return self._template
        d = self._made.get(k)
        if d is None:
            g = self._g[self._rest[k]]
            d = self._made[k] = {**self._template, 'G': g, 'G_orig': g}
        return d


class _Picked(object):
    """``seq[i] for i in positions`` without making them"""

    def __init__(self, seq, positions):
        self._seq, self._pos = seq, positions

    def __len__(self):
        return len(self._pos)

    def __iter__(self):
        return (self._seq[i] for i in self._pos)

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self._seq[i] for i in self._pos[k]]
        return self._seq[self._pos[k]]


class _Chain(object):
    """seqs[n][k] as chain[(n, k)]"""

    def __init__(self, seqs):
        self._seqs = seqs

    def __getitem__(self, nk):
        return self._seqs[nk[0]][nk[1]]


class DeferredLaunch(object):
    """One launch of ``ElementwiseMaxEnt.run()`` on array input as the :class:`MaxEntResult` holds it until somebody looks at
    something per element (``MaxEntResult.add_deferred``): the launch's arrays as they came off the device, and ``settle``,
    which builds the records and analyses of its scans the way ``run()`` always did.  ``field`` / ``A_out`` serve the whole-matrix
    fields from the arrays (the same views and the same arithmetic as the assembly from records: the same bits)."""
    covers = None

    def __init__(self, keys, sols, alpha, omega, maps, which_of, settle):
        self.keys, self.sols, self.alpha, self.omega = keys, sols, alpha, omega
        self._maps, self._which_of, self._settle = maps, which_of, settle

    def settle(self, result):
        fn, self._settle = self._settle, None
        if fn is not None:
            fn(result)

    def _identity_delta(self):
        """delta of the output map when every scan's A is H / delta with the same delta, else None"""
        first = self._maps[0]
        if type(first).__name__ != 'IdentityA_of_H':
            return None
        d0 = getattr(getattr(first, '_omega', None), 'delta', None)
        for m in self._maps[1:]:
            if m is first:
                continue
            d = getattr(getattr(m, '_omega', None), 'delta', None)
            if type(m) is not type(first) or d is None or d0 is None or np.shape(d) != np.shape(d0) or not np.array_equal(d, d0):
                return None
        return d0

    def field(self, name, ems):
        sols = self.sols
        n, na = sols.n, sols.n_alpha
        if name in ('chi2', 'S', 'Q'):
            v = sols.arrays[name].reshape(tuple(ems) + (na,))
            v.setflags(write=False)
            return v
        if name == 'n_iter':
            return sols.arrays['n_iter'].astype(float).reshape(tuple(ems) + (na,))
        if name == 'converged':
            return sols.conv.astype(float).reshape(tuple(ems) + (na,))
        if name == 'H':
            whole = sols.claim_H.materialize()
            v = whole.reshape(tuple(ems) + (na, sols.n_omega))
            v.setflags(write=False)
            return v
        if name == 'A':
            delta = self._identity_delta()
            if delta is None:
                return None
            from . import device
            from .maxent_result import _by_rows
            H = self.field('H', ems)
            out = device.pinned_empty(H.shape)
            _by_rows(lambda a, b: np.divide(a, delta, out=b), H, out)
            return out
        return None

    def A_out(self, analyzer_name, ems):
        which = self._which_of.get(analyzer_name)
        picks = self.sols.picks
        if which is None or picks is None:
            return None
        idx = picks[0][which]
        delta = self._identity_delta()
        if delta is None or np.any(idx < 0):
            return None
        rows = np.asarray(picks[1][which])
        return (rows / delta).reshape(tuple(ems) + (rows.shape[-1],))


class PendingRun(object):
    """what :meth:`ElementwiseMaxEnt.run_async` returns: ``result()`` waits for the device and completes the run"""

    def __init__(self, owner, finish):
        self._owner, self._finish = owner, finish
        self._result = owner.maxent_result if finish is None else None
        self.done = finish is None

    def result(self):
        if not self.done:
            finish, self._finish = self._finish, None
            try:
                self._result = finish()
            finally:
                self.done = True
                if self._owner.__dict__.get('_pending_run') is self:
                    object.__setattr__(self._owner, '_pending_run', None)     # (the object does not hold on to its last result)
                self._owner = None
        return self._result


def run_many(objects, in_flight=None, same_cut=True):
    """``[ew.run() for ew in objects]`` with the jobs IN FLIGHT together: every object is prepared, staged and launched before
    the first is waited for (one thread, no wait between the launches), then each is completed in turn while the kernels of
    the others run.  ``in_flight``: jobs on the GPU at a time (default: all of them, at most eight).  Every job is cut into
    pieces as ``run()`` cuts it, so every field of every result is, bit for bit, what the sequential calls return.
    ``same_cut=False`` cuts a job for the company it has (``mxe_opts.in_flight``: fewer cold-started pieces, 0.65 instead of
    0.74 ms of GPU time per 16 x 16 x 100-alpha job with four in flight): other iterates, the same minimisers within the
    stopping tolerance (A_out to ~1e-10) -- through this API the host's work per job hides the difference (four jobs: 3.8 ms
    either way); a caller of the C interface with its own pipeline sees it (bench.py, value_in_flight)."""
    objects = list(objects)
    n = max(1, min(8, len(objects) if in_flight is None else int(in_flight)))
    cut = 1 if same_cut else n
    results, window = [None] * len(objects), []
    for k, ew in enumerate(objects):
        if len(window) >= n:
            j, h = window.pop(0)
            results[j] = h.result()
        window.append((k, ew.run_async(in_flight=cut) if hasattr(ew, 'run_async') else _Ran(ew.run())))
    for j, h in window:
        results[j] = h.result()
    return results


class _Ran(object):
    def __init__(self, result):
        self._r = result

    def result(self):
        return self._r


class ElementwiseMaxEnt(object):
    maxent_diagonal = None
    maxent_offdiagonal = None

    def __init__(self, use_hermiticity=True, use_complex=False, n_gpus=None, device_ids=None, **kwargs):
        """``n_gpus`` / ``device_ids``: shard the matrix elements over several GPUs of this process
        (element e of a phase on device e mod N, one gather).  Default: device 0."""
        if device_ids is None and n_gpus is not None:
            device_ids = tuple(range(int(n_gpus)))
        object.__setattr__(self, 'device_ids', None if device_ids is None else tuple(device_ids))
        self.maxent_diagonal = TauMaxEnt(**kwargs)
        self.maxent_offdiagonal = TauMaxEnt(cost_function='plusminus',
                                            **kwargs)
        self.set_G_element = None
        self.determine_shape = None
        self.G_mat = None
        self.maxent_result = None
        self.use_hermiticity = use_hermiticity
        self.use_complex = use_complex
        self.last_launches = []

    # ---- attribute shadowing onto both workers -------------------------
    def __getattr__(self, name):
        d = getattr(object.__getattribute__(self, 'maxent_diagonal'), name)
        o = getattr(object.__getattribute__(self, 'maxent_offdiagonal'), name)
        if callable(d) and callable(o):
            return CallableMethodCheck(name, d, o)
        if np.all(d == o):
            return d
        raise Exception('Element {n} not uniquely defined. Use '
                        'self.maxent_diagonal.{n} or '
                        'self.maxent_offdiagonal.{n}!'.format(n=name))

    def __setattr__(self, name, value):
        if hasattr(self.maxent_diagonal, name) and \
                hasattr(self.maxent_offdiagonal, name):
            setattr(self.maxent_offdiagonal, name, value)
            setattr(self.maxent_diagonal, name, value)
        else:
            object.__setattr__(self, name, value)

    # ---- result object ---------------------------------------------------
    def prepare_maxent_result(self, overwrite=False):
        if self.maxent_result is None or overwrite:
            self.maxent_result = MaxEntResult(
                matrix_structure=self.determine_shape(self.G_mat),
                element_wise=True,
                use_hermiticity=self.use_hermiticity,
                complex_elements=self.use_complex)

    # ---- single element (one chain) ---------------------------------------
    def _worker_for(self, element):
        return self.maxent_diagonal if element[0] == element[1] \
            else self.maxent_offdiagonal

    def _load_element(self, worker, element, re):
        i, j = element
        self.set_G_element(worker, self.G_mat, (i, j),
                           True if i == j else re)
        err = self.get_error((i, j))
        if self.__dict__.get('_errors_from_bins'):
            err = err[0 if (re or i == j) else 1]       # (real and imaginary part have eigenbases of their own)
        self.put_error(worker, err)

    def run_element(self, element, re=True):
        """one matrix element, like the reference's ``run_element``
        (elementwise_maxent.py:170-221)."""
        self.prepare_maxent_result(overwrite=False)
        i, j = element
        worker = self._worker_for(element)
        if i != j and self.use_hermiticity and i > j:
            worker.logtaker.message(
                VerbosityFlags.ElementInfo,
                'Element {} {} not calculated, can be determined from '
                'hermiticity'.format(i, j))
            return self.maxent_result
        worker.logtaker.message(VerbosityFlags.ElementInfo,
                                'Calling MaxEnt for element {} {}'.format(i, j))
        self._load_element(worker, element, re)
        worker.run(result=self.maxent_result, matrix_element=(i, j),
                   complex_index=0 if re else 1)
        return self.maxent_result

    # ---- batched phases --------------------------------------------------
    def _run_batch(self, worker, jobs, per_job_D=None):
        """``jobs``: list of (element, re).  All scans in one launch."""
        batch = self._prepare_batch(worker, jobs, per_job_D)
        self._solve_batches([batch])
        return self._finish_batch(batch)

    def _prepare_batch(self, worker, jobs, per_job_D=None, defer_last_load=None):
        """the specs of the elements of ``jobs`` that are to be solved (the others go to the result's zero
        elements); leaves ``worker`` loaded with the last element, as the reference does"""
        self.prepare_maxent_result(overwrite=False)
        res = self.maxent_result
        loop = worker.maxent_loop
        specs, live = [], []
        self._share_decomposition()
        direct = self._direct_input(worker) and per_job_D is None
        template = None
        below = err_same = g_rows = first_spec = g_mat = arrays = None
        if direct and len(jobs) > 1:
            # (all elements at once: the data vectors as the rows of ONE array -- real part, or imaginary part of an off-diagonal
            #  element's second scan --, which of them are below the threshold; one error array when it is the same for all)
            Gm = self.G_mat[1]
            plan = self.__dict__.get('_plans', {}).get(id(jobs))
            if plan is not None and plan['jobs'] is jobs:
                ii, jj, real_part, all_real = plan['ii'], plan['jj'], plan['real_part'], plan['all_real']
            else:
                ii = np.fromiter((e[0] for e, _ in jobs), dtype=np.intp, count=len(jobs))
                jj = np.fromiter((e[1] for e, _ in jobs), dtype=np.intp, count=len(jobs))
                real_part = np.fromiter((bool(re) for _, re in jobs), dtype=bool, count=len(jobs)) | (ii == jj)
                all_real = bool(real_part.all())
            Gsel = Gm[ii, jj]
            if np.iscomplexobj(Gsel):
                g_rows = np.where(real_part[:, None], Gsel.real, Gsel.imag).astype(float, copy=False)
            else:
                g_rows = np.array(Gsel, dtype=float)
                if not all_real:
                    g_rows[~real_part] = 0.0         # (the imaginary part of real data)
            with np.errstate(all='ignore'):
                below = (np.max(np.abs(g_rows), axis=-1) < loop.G_threshold).tolist()
            g_mat = g_rows
            g_rows = list(g_rows)                    # (row views, made in one go)
            e0 = self.get_error(tuple(jobs[0][0]))
            if isinstance(self.error, float) or len(np.shape(self.error)) == self.error_dimension:
                err_same = np.asarray(e0, dtype=float) * np.ones(np.shape(Gm)[-1])
            # a worker that already holds this tau grid (an object that has run before) is not sent through its setters for the FIRST
            # element either: nothing of a spec but the data depends on the element that is loaded, and the state the phase leaves
            # behind is that of the last element, loaded below (two loads per run instead of four: 0.1 ms)
            try:
                skip_first = (err_same is not None and loop.G is not None and loop.err is not None and
                              np.array_equal(np.asarray(worker.tau), np.asarray(self.G_mat[0])))
            except Exception:
                skip_first = False
        else:
            skip_first = False
        for n, (element, re) in enumerate(jobs):
            cidx = 0 if re else 1
            if direct and (n > 0 or skip_first):
                break               # (array input, plain errors, unrotated kernel: every further element below, straight from the arrays)
            if per_job_D is not None:
                worker.set_D(per_job_D[n])
            self._load_element(worker, element, re)
            if n == 0:
                self._share_decomposition()      # (the worker has its tau grid now)
            if loop.below_threshold():
                key = tuple(element) + ((cidx,) if self.use_complex else ())
                res._zero_elements.append(key)
                worker.logtaker.error_message(
                    'G below threshold, not performing the calculation.')
                continue
            spec = loop.make_spec()
            spec['A_map'] = loop.A_of_H
            if n == 0:
                first_spec = spec
            specs.append(spec)
            live.append((element, cidx))
        if direct and len(jobs) > 1:
            # the specs of the further elements: copies of ONE template with their rows of the data array (the worker keeps the
            # first element's state until the last is loaded, the state the reference leaves behind)
            rest = []
            for n in range(0 if skip_first else 1, len(jobs)):
                if below[n]:
                    element, re = jobs[n]
                    res._zero_elements.append(tuple(element) + (((0 if re else 1),) if self.use_complex else ()))
                    worker.logtaker.error_message('G below threshold, not performing the calculation.')
                else:
                    rest.append(n)
            if rest:
                n0 = rest[0]
                g, e0 = g_rows[n0], self.get_error(tuple(jobs[n0][0]))
                # (everything but the data is what the first element's spec holds, when that was made a moment ago)
                template = loop.make_spec(G=g, err=e0) if first_spec is None else loop.spec_like(first_spec, g, e0)
                template['A_map'] = loop.A_of_H
                template['G'] = template['G_orig'] = g
                if err_same is not None:
                    # (ONE error array for every spec of the batch: BatchSolver._stage then stages one row instead of stacking
                    #  256 -- it was 1 ms of the 4.7 ms of a run on an object that has run before)
                    template['err'] = err_same
                    # the job of this batch as ARRAYS, and its specs made when somebody asks (round 5: 256 dict copies per run
                    # that a launch staged from the arrays never reads)
                    specs = _LazySpecs(first_spec, template, g_rows, rest)
                    lead = first_spec if first_spec is not None else template
                    arrays = dict(G=(g_mat if (first_spec is None and len(rest) == len(jobs)) else
                                     g_mat[([0] if first_spec is not None else []) + rest]), err=err_same, D=lead['D'],
                                  alpha=lead['alpha'], v0=lead['v0'], kind=lead['kind'])
                else:
                    specs.append(template)
                    specs.extend([loop.spec_like(template, g_rows[n], self.get_error(tuple(jobs[n][0]))) for n in rest[1:]])
                whole = len(live) + len(rest) == len(jobs) and plan is not None and plan['jobs'] is jobs
                if whole and 'live' in plan:
                    live = plan['live']              # (every element of the phase is solved: one list for every run)
                else:
                    live.extend([(jobs[n][0], 0 if jobs[n][1] else 1) for n in rest])
                    if whole:
                        plan['live'] = live
                if rest[-1] == len(jobs) - 1:
                    if defer_last_load is not None and arrays is not None:
                        # (the state the phase leaves behind -- the worker loaded with its last element, as in the reference -- does
                        #  not enter the launch: the caller makes it up behind the launch, beside the kernel)
                        defer_last_load.append((worker, jobs[-1][0], jobs[-1][1]))
                    else:
                        self._load_element(worker, jobs[-1][0], jobs[-1][1])
        # (the keys of the result's records, made once: they were made three times per element -- 0.2 ms of a 16 x 16 run)
        keys = None
        if direct and len(jobs) > 1:
            plan = self.__dict__.get('_plans', {}).get(id(jobs))
            if plan is not None and plan.get('live') is live:
                flags = (res.matrix_structure is None, bool(res.element_wise), bool(res.complex_elements))
                if plan.get('keys_flags') != flags:
                    plan['keys'], plan['keys_flags'] = res._keys(live), flags
                keys = plan['keys']
        if keys is None:
            keys = res._keys(live)
        return dict(worker=worker, specs=specs, live=live, keys=keys, arrays=arrays)

    def _solve_batches(self, batches, defer=False, in_flight=0):
        """(``defer``: launch only and return the function that waits for the device and completes the batches -- the caller
        launches other objects meanwhile, :meth:`run_async`)
        one launch for all batches whose workers share the decomposition of the kernel, the minimiser settings
        and the alpha count (plain ElementwiseMaxEnt: diagonal and off-diagonal elements together, as bench.py
        times them); otherwise one launch per batch"""
        batches = [b for b in batches if b['specs']]
        groups = []
        for b in batches:
            for g in groups:
                if self._same_launch(g[0], b):
                    g.append(b)
                    break
            else:
                groups.append([b])
        res = self.maxent_result
        ends = []
        for g in groups:
            loop = g[0]['worker'].maxent_loop
            # the scans of the launch in the order of the result's matrix (row major): what comes off the device in one
            # copy then IS the (M, N, n_alpha, n_omega) array of the result -- MaxEntResult._assemble takes it as a view
            # (the order of a launch and the index arrays that go with it depend on the key lists of its batches alone; the lists of
            #  the full phases are one object per object and phase -- _jobs --: their launch plan is made once)
            lplans = self.__dict__.setdefault('_launch_plans', {})
            lkey = tuple(id(b['keys']) for b in g)
            lp = lplans.get(lkey)
            if lp is None or not all(k0 is b['keys'] for k0, b in zip(lp['keys_of'], g)):
                where = [(key, n, k) for n, b in enumerate(g) for k, key in enumerate(b['keys'])]
                try:
                    where.sort(key=lambda t: t[0])
                except TypeError:
                    pass
                offs = np.cumsum([0] + [len(b['keys']) for b in g])
                src = np.fromiter((offs[n] + k for (_, n, k) in where), dtype=np.intp, count=len(where))
                inv = np.empty(len(where), dtype=np.intp)
                inv[src] = np.arange(len(where))            # position in the launch of scan k of batch n: inv[offs[n] + k]
                lp = dict(keys_of=[b['keys'] for b in g], where=where, offs=offs, src=src, inv=inv,
                          sel=np.fromiter((n for (_, n, k) in where), dtype=np.intp, count=len(where)),
                          nk=[(n, k) for (_, n, k) in where], launch_keys=[key for (key, _, _) in where])
                plans_held = self.__dict__.get('_plans', {})
                if all(any(p.get('keys') is b['keys'] for p in plans_held.values()) for b in g):
                    if len(lplans) > 8:
                        lplans.clear()
                    lplans[lkey] = lp                       # (only for key lists that live as long as this object does)
            where = lp['where']
            all_arrays = all(b.get('arrays') is not None for b in g)
            specs = _Picked(_Chain([b['specs'] for b in g]), lp['nk']) if all_arrays else \
                [g[n]['specs'][k] for (_, n, k) in where]
            t0 = datetime.now()
            for b in g:
                b['t_start'] = t0              # (into the result's table of start times with the records: _finish_batch)
            for b in g:
                b['sols'] = [None] * len(b['specs']) if not all_arrays else None

            def hand_out(sols, g=g, where=where):
                for b in g:
                    if b['sols'] is None:
                        b['sols'] = [None] * len(b['specs'])
                for sol, (_, n, k) in zip(sols, where):
                    g[n]['sols'][k] = sol

            def records_while_the_kernel_runs(sols, g=g):
                # (the result dicts hold their arrays already, the device fills them behind this: the records of the scans --
                #  0.3 ms of dictionaries for 256 elements -- cost nothing next to a kernel of 0.8 ms)
                hand_out(sols)
                for b in g:
                    b['records'] = b['worker'].maxent_loop.make_records(b['specs'], b['sols'])
            plain = all(b['worker'].maxent_loop.probability is None for b in g)
            select = select_params(loop.analyzers)
            lazy = (defer and plain and select is not None and all(b.get('arrays') is not None for b in g) and
                    (self.device_ids is None or len(self.device_ids) == 1) and hasattr(loop.minimizer, 'to_opts') and
                    not any(bool(b['worker'].logtaker.verbose & (VerbosityFlags.ElementInfo | VerbosityFlags.AlphaLoop)) for b in g))
            if lazy:
                # the launch from ARRAYS: the data rows of the batches in the order of the launch, one row of D / alpha / v0 /
                # kind per batch; nothing per scan is built here -- records and analyses when somebody looks (DeferredLaunch)
                offs, src, sel, inv = lp['offs'], lp['src'], lp['sel'], lp['inv']
                arrays = dict(n=len(where), G=np.concatenate([b['arrays']['G'] for b in g])[src],
                              err=np.asarray(g[0]['arrays']['err'], dtype=float).reshape(1, -1), sel=sel,
                              D=np.stack([b['arrays']['D'] for b in g]), alpha=np.stack([b['arrays']['alpha'] for b in g]),
                              v0=np.stack([b['arrays']['v0'] for b in g]), kinds=np.array([b['arrays']['kind'] for b in g]))
                if not all(np.array_equal(g[0]['arrays']['err'], b['arrays']['err']) for b in g[1:]):
                    arrays['err'] = np.stack([b['arrays']['err'] for b in g])[sel]
                wait = solve_elements(loop.K, None, loop.minimizer, device_id=loop.device_id, device_ids=self.device_ids,
                                      chi2_factor=loop.cost_function.chi2_factor, select=select, defer=True, in_flight=in_flight,
                                      arrays=arrays)
                for n, b in enumerate(g):
                    b['positions'] = inv[offs[n]:offs[n + 1]]
                    b['launch_keys'] = lp['launch_keys']
                    b['launch_select'] = select
                    b['launch_batches'] = len(g)          # (not g itself: a batch that holds the list it is in is a cycle, and its
                    #  claim on the device buffers would live until the collector runs)
            else:
                for b in g:
                    b['arrays'] = None
                wait = solve_elements(loop.K, specs, loop.minimizer,
                                      device_id=loop.device_id, device_ids=self.device_ids,
                                      want_logdet=loop.probability is not None,
                                      chi2_factor=loop.cost_function.chi2_factor,
                                      select=select,
                                      while_waiting=records_while_the_kernel_runs if plain else None,
                                      defer=True, in_flight=in_flight)

            def end(g=g, wait=wait, t0=t0, specs=specs, hand_out=hand_out, lazy=lazy):
                sols, info = wait()
                t1 = datetime.now()
                self.last_launches.append(info)
                for b in g:
                    b.update(info=info, t0=t0, t1=t1, per_alpha=(t1 - t0) / max(1, len(specs) * len(specs[0]['alpha'])))
                if lazy:
                    for b in g:
                        b['sols'] = _Picked(sols, b['positions'])
                        b['launch'] = sols
                elif not all('records' in b for b in g):
                    hand_out(sols)
            if defer:
                ends.append(end)
            else:
                end()

        def end_all():
            for e in ends:
                e()
        return end_all if defer else None

    def _same_launch(self, a, b):
        la, lb = a['worker'].maxent_loop, b['worker'].maxent_loop
        if la is lb:
            return True
        Ka, Kb = la.K, lb.K
        try:
            same = (Ka._U is not None and Ka._U is Kb._U and Ka._S is Kb._S and Ka._V is Kb._V and
                    Ka.rotation is None and Kb.rotation is None and
                    len(a['specs'][0]['alpha']) == len(b['specs'][0]['alpha']) and
                    (la.probability is None) == (lb.probability is None) and
                    la.device_id == lb.device_id and
                    la.cost_function.chi2_factor == lb.cost_function.chi2_factor and
                    bytes(la.minimizer.to_opts()) == bytes(lb.minimizer.to_opts()))
        except Exception:
            return False
        return bool(same)

    def _finish_batch(self, batch):
        """records and analyzers of a solved batch"""
        res = self.maxent_result
        if not batch['specs']:
            return res
        self._finish_now(batch)
        self._finish_records(batch, res)
        return res

    def _finish_now(self, batch):
        """what of the end of a batch is not a record: the log lines, the state the minimiser is left in, the timing line"""
        res = self.maxent_result
        worker, specs, live = batch['worker'], batch['specs'], batch['live']
        loop = worker.maxent_loop
        if res._default_analyzer_name is None and loop.analyzers:
            res._default_analyzer_name = loop.analyzers[0].name
        sols, info = batch['sols'], batch['info']
        talk = bool(worker.logtaker.verbose & (VerbosityFlags.ElementInfo | VerbosityFlags.AlphaLoop))
        if talk:
            for sol, (element, cidx) in zip(sols, live):
                worker.logtaker.message(
                    VerbosityFlags.ElementInfo,
                    'Element {} {}{}'.format(element[0], element[1],
                                             '' if cidx == 0 else ' (imaginary part)'))
                loop.log_alpha_lines(sol)
        elif len(sols):
            # (one reduction over the rows of the launch's count array, not one numpy call per element: 1.2 ms for 256 elements)
            if batch.get('launch') is not None:
                total = int(batch['launch'].arrays['n_iter'][batch['positions']].sum())
            else:
                total = int(np.asarray([x['n_iter'] for x in sols]).sum())
            loop.note_minimizer_state(sols[-1], total)
        worker.logtaker.message(
            VerbosityFlags.Timing,
            '{} alpha scans x {} alpha in one launch: kernel {:.3f} ms',
            len(specs), len(specs[0]['alpha']), info['kernel_ms'])

    def _finish_records(self, batch, res):
        """the records of a solved batch into ``res``, and its analyzers (for a launch that was handed to the result as ONE
        object -- DeferredLaunch -- this runs when somebody looks at something per element)"""
        worker, specs, live = batch['worker'], batch['specs'], batch['live']
        loop = worker.maxent_loop
        sols, t1, per_alpha = batch['sols'], batch['t1'], batch['per_alpha']
        records = batch.pop('records', None)
        if records is None:
            records = loop.make_records(specs, sols)
        times = {}
        for rec in records:
            X = len(rec['alpha'])
            if X not in times:
                times[X] = (per_alpha,) * X        # (one immutable tuple for the records of a launch; MaxEntResult.run_times hands out lists)
            rec['run_times'] = times[X]
        keys = res.add_batch_results(records, live, t_start=batch.get('t_start'), t_end=t1, keys=batch.get('keys'))
        # analyzers after every record of the batch is in (adding a record drops the assembled-array cache
        # of the result); the rows of A they select come off the device in one go
        res.analyze_batch(loop.analyzers, keys)

    def _finish_deferred(self, batches):
        """the end of ``run()`` for batches that were ONE launch from arrays: the result gets the launch as one object, the records
        of its scans when somebody looks.  False when that does not apply (then: :meth:`_finish_batch`)."""
        res = self.maxent_result
        live = [b for b in batches if b['specs']]
        if not live or any(b.get('launch') is None for b in live) or any(b['launch'] is not live[0]['launch'] for b in live) or \
                live[0]['launch_batches'] != len(live) or res.__dict__.get('_records_store') or res.__dict__.get('_deferred'):
            return False
        from .analyzers import LineFitAnalyzer, Chi2CurvatureAnalyzer, EntropyAnalyzer
        select = live[0]['launch_select']
        which_of = None
        for b in live:
            cur = {}
            for a in b['worker'].maxent_loop.analyzers:
                w = (0 if (type(a) is LineFitAnalyzer and a.linefit_deg == select[0]) else
                     1 if (type(a) is Chi2CurvatureAnalyzer and a.gamma == select[1]) else
                     2 if type(a) is EntropyAnalyzer else None)
                cur[a.name] = None if a.name in cur else w          # (two analyzers of one name: the general way)
            which_of = cur if which_of is None else {k: v for k, v in which_of.items() if cur.get(k, -1) == v}
        which_of = {k: v for k, v in (which_of or {}).items() if v is not None}
        for b in live:
            self._finish_now(b)
        lead = live[0]['worker'].maxent_loop
        first = live[0]['launch_keys'][0]
        first_batch = next(b for b in live if b['keys'] and b['keys'][0] == first)

        def settle(result, live=live):
            for b in live:
                self._finish_records(b, result)
        res.add_deferred(DeferredLaunch(live[0]['launch_keys'], live[0]['launch'], first_batch['arrays']['alpha'], lead.omega,
                                        [b['worker'].maxent_loop.A_of_H for b in live], which_of, settle))
        return True

    # ---- error bars ------------------------------------------------------------
    def _posterior_models(self, jobs, result):
        """default models of the off-diagonal jobs when they are not the worker's own (PoormanMaxEnt), else None"""
        return None

    def _posterior_elements(self, res, run, extra, flip_names, what, with_stream=False, skip=('info',), timing=None,
                            fields=(), ragged=()):
        """What :meth:`posterior_errors` and :meth:`posterior_samples` share.  The items (see ``posterior.element_errors``;
        ``with_stream``: with their ``stream``) of every computed element of ``res``, per worker phase, go to
        ``run(K, omega, items, default_name=, chi2_factor=, device_ids=, bryan=, timing=)``, which returns one dict per item.
        These are assembled into a dict (with ``extra``): arrays shaped like the result's fields, NaN (-1 for integers) where nothing was
        computed, the hermitian partners filled in -- the imaginary part's ``flip_names`` with the other sign; ``info``
        per element, the names ``skip`` left out.  ``fields``: further fields of the result that an item carries under
        their names; ``ragged``: names whose last axis (the data rows) may differ between elements and is padded with NaN
        to the longest."""
        from . import posterior
        zero = set(tuple(z) for z in res.zero_elements)
        phases = [(self.maxent_diagonal, self._diag_jobs(), None)]
        if not isinstance(self, DiagonalMaxEnt):
            off = self._offdiag_jobs()
            phases.append((self.maxent_offdiagonal, off, self._posterior_models(off, res)))
        ids = self.device_ids if self.device_ids else (self.maxent_diagonal.maxent_loop.device_id,)
        collected, ms, counts = [], 0.0, {}
        for worker, jobs, models in phases:
            loop = worker.maxent_loop
            items, keys = [], []
            for n, (element, re) in enumerate(jobs):
                cidx = 0 if re else 1
                key = tuple(element) + ((cidx,) if self.use_complex else ())
                if key in zero:
                    continue
                try:
                    H = np.asarray(res.element_array('H', key), dtype=float)
                except (KeyError, IndexError, AttributeError, AssertionError):
                    continue
                if H.ndim != 2 or H.shape[0] == 0:
                    continue
                if models is not None:
                    worker.set_D(models[n])
                self._load_element(worker, element, re)
                spec = loop.make_spec()
                posterior.check_alpha(spec, res.alpha)
                logp = np.asarray(res.element_array('probability', key), dtype=float)
                ana = res.analyzer_results
                for i in key:
                    ana = ana[i]
                item = dict(spec=spec, H=H, alpha=np.asarray(res.alpha, dtype=float), analysis=ana,
                            probability=None if np.all(np.isnan(logp)) else logp, B=loop.A_of_H.matrix())
                for name in fields:
                    item[name] = np.asarray(res.element_array(name, key))
                if with_stream:
                    item['stream'] = int(np.ravel_multi_index(tuple(element), tuple(self.shape))) * 2 + cidx
                items.append(item)
                keys.append(key)
            if not items:
                continue
            t = {}
            outs = run(worker.K, worker.omega, items, default_name=res.default_analyzer_name,
                       chi2_factor=loop.cost_function.chi2_factor, device_ids=ids,
                       bryan=posterior.find_bryan(loop.analyzers), timing=t)
            ms += t.get('ms', 0.0)
            for name in ('reused_contexts', 'launches'):             # (what the drivers of a phase report beside the time)
                if name in t:
                    counts[name] = counts.get(name, 0) + t[name]
            collected.extend(zip(keys, outs))
        if timing is not None:
            timing['ms'] = ms
            timing.update(counts)
        if not collected:
            raise ValueError('the result holds no element to {}'.format(what))
        struct = tuple(self.shape) + ((2,) if self.use_complex else ())
        out = dict(info={}, **extra)
        for name in ragged:
            longest = max(np.shape(o[name])[-1] for _, o in collected)
            for _, o in collected:
                val = np.asarray(o[name], dtype=float)
                pad = [(0, 0)] * (val.ndim - 1) + [(0, longest - val.shape[-1])]
                o[name] = np.pad(val, pad, constant_values=np.nan)
        for key, o in collected:
            out['info'][key] = o['info']
            for name, val in o.items():
                if name in skip:
                    continue
                val = np.asarray(val)
                if name not in out:
                    out[name] = np.full(struct + val.shape, np.nan) if val.dtype.kind == 'f' else \
                        np.full(struct + val.shape, -1, dtype=val.dtype)
                if out[name].shape[len(struct):] != val.shape:
                    raise ValueError('{}: the elements chose different numbers of alphas; use alpha= indices'.format(name))
                out[name][key] = val
                if self.use_hermiticity and key[0] != key[1]:
                    # G_ji = conj(G_ij): the same errors and spectra; the imaginary part's values change sign
                    flip = -1.0 if (len(key) == 3 and key[2] == 1 and name in flip_names) else 1.0
                    out[name][(key[1], key[0]) + key[2:]] = val * flip if val.dtype.kind == 'f' else val
        return out

    def posterior_errors(self, result=None, alpha=None, windows=None, functionals=None, pointwise=False, timing=None):
        """:meth:`TauMaxEnt.posterior_errors` for every matrix element of ``result`` (default: the last result of this
        object): all elements of a worker -- the diagonal ones, the off-diagonal ones with their plus-minus entropy -- in
        ONE call of ``mxe_posterior_var`` per device, each with its own error bars or covariance.  Returns a dict of arrays
        shaped like the result's fields (matrix indices, then the complex index with ``use_complex``, then what
        :meth:`TauMaxEnt.posterior_errors` returns); elements that were not computed (below the threshold) hold NaN,
        those that follow from hermiticity are filled from their partners.  ``info``: per computed element its
        ``nan_rows``."""
        from . import posterior
        res = self.maxent_result if result is None else result
        if res is None:
            raise ValueError('no result: run() first or hand one in')

        def run(K, omega, items, **common):
            return posterior.element_errors(K, omega, items, alpha=alpha, windows=windows, functionals=functionals,
                                            pointwise=pointwise, **common)
        return self._posterior_elements(res, run, {}, ('window_weight', 'functional_value', 'A'), 'compute errors for',
                                        timing=timing)

    def posterior_samples(self, result=None, n_samples=100, seed=0, alpha=None, transform='linear', z=None, timing=None):
        """:meth:`TauMaxEnt.posterior_samples` for every matrix element of ``result`` (default: the last result of this
        object): all elements of a worker in ONE call of ``mxe_posterior_sample`` per device.  The stream of an element is
        ((flat matrix index) * 2 + complex index) * n_alpha + alpha index, so an element draws the same spectra alone and
        inside a matrix, and different elements draw independently.  ``z`` is used for every element alike.  Returns a dict of arrays laid out like
        :meth:`posterior_errors`' (elements that were not computed hold NaN; those that follow from hermiticity are
        filled from their partners, the imaginary part's spectra with the other sign).  ``transform='log'`` raises
        ``ValueError`` when plus-minus (off-diagonal) elements are among them."""
        from . import posterior
        res = self.maxent_result if result is None else result
        if res is None:
            raise ValueError('no result: run() first or hand one in')
        if int(n_samples) < 1:
            raise ValueError('n_samples must be at least 1, got {}'.format(n_samples))
        if transform not in posterior.TRANSFORMS:
            raise ValueError('transform={!r}: one of {} is needed'.format(transform, posterior.TRANSFORMS))

        def run(K, omega, items, **common):
            return posterior.element_samples(K, omega, items, n_samples=n_samples, seed=seed, alpha=alpha, transform=transform,
                                             z=z, **common)
        return self._posterior_elements(res, run, dict(seed=int(seed)), ('H', 'H_samples', 'A_samples'), 'draw samples for',
                                        with_stream=True, skip=('info', 'seed'), timing=timing)

    def fit_diagnostics(self, result=None, alpha='all', timing=None):
        """:meth:`TauMaxEnt.fit_diagnostics` for every matrix element of ``result`` (default: the last result of this
        object): all elements of a worker -- the diagonal ones, the off-diagonal ones with their plus-minus entropy -- in
        ONE call of ``mxe_fit_diagnostics`` per device, each with its own data, error bars or covariance.  Returns a dict of
        arrays laid out like :meth:`posterior_errors`' (matrix indices, then the complex index with ``use_complex``, then
        what :meth:`TauMaxEnt.fit_diagnostics` returns; elements that were not computed hold NaN, -1 for indices; those
        that follow from hermiticity are filled from their partners, the imaginary part's residuals and spectra with the
        other sign).  The data rows of ``residual``, ``leverage`` and ``studentized`` are padded with NaN to the longest
        element.  ``info``: per computed element its ``nan_rows``."""
        from . import diagnostics
        res = self.maxent_result if result is None else result
        if res is None:
            raise ValueError('no result: run() first or hand one in')

        def run(K, omega, items, bryan=None, **common):
            return diagnostics.element_diagnostics(K, items, alpha=alpha, **common)
        return self._posterior_elements(res, run, {}, ('residual', 'studentized', 'A_gcv', 'A_classic'), 'compute diagnostics for',
                                        timing=timing, fields=('S', 'A'), ragged=('residual', 'leverage', 'studentized'))

    def resolution(self, result=None, omega0=None, alpha=None, test=None, timing=None):
        """:meth:`TauMaxEnt.resolution` for every matrix element of ``result`` (default: the last result of this object):
        all elements of a worker -- the diagonal ones, the off-diagonal ones with their plus-minus entropy -- in the same
        ``mxe_response`` calls.  Returns a dict of arrays laid out like :meth:`posterior_errors`' (matrix indices, then the
        complex index with ``use_complex``, then what :meth:`TauMaxEnt.resolution` returns); ``index`` and ``omega0`` are
        shared by all elements.  Elements that were not computed (below the threshold) hold NaN; those that follow from
        hermiticity are filled from their partners UNCHANGED, the imaginary part too: a point-spread function, an averaging
        kernel and an ``image`` per unit of the element's own true spectrum are ratios of two quantities that change sign
        together.  ``test`` is applied to every element alike.  ``timing``: ``ms``, ``launches``, ``reused_contexts``."""
        from . import response
        res = self.maxent_result if result is None else result
        if res is None:
            raise ValueError('no result: run() first or hand one in')
        shared, noted = {}, []

        def note(msg, *args):
            if not noted:
                noted.append(msg)
                self.maxent_diagonal.logtaker.error_message(msg, *args)

        def run(K, omega, items, bryan=None, **common):
            outs = response.element_resolution(K, omega, items, omega0=omega0, alpha=alpha, test=test, note=note, **common)
            for o in outs:
                shared['index'], shared['omega0'] = o.pop('index'), o.pop('omega0')
                if o['averaging_kernel'] is None:
                    del o['averaging_kernel']
            return outs
        out = self._posterior_elements(res, run, {}, (), 'compute the resolution of', timing=timing)
        out.update(shared)
        out.setdefault('averaging_kernel', None)
        return out

    def default_model_response(self, result=None, dlogD=None, alpha=None, timing=None):
        """:meth:`TauMaxEnt.default_model_response` for every matrix element of ``result`` (default: the last result of
        this object), every element with its own default model (``PoormanMaxEnt``: the off-diagonal models built from the
        diagonal results) and the same relative changes ``dlogD`` (n_dir, n_omega).  Returns a dict of arrays laid out like
        :meth:`posterior_errors`'.  Elements that follow from hermiticity are filled from their partners; ``dA`` and ``dH``
        of a mirrored imaginary part take the other sign (the spectrum itself changes sign, ln D does not)."""
        from . import response
        res = self.maxent_result if result is None else result
        if res is None:
            raise ValueError('no result: run() first or hand one in')
        if dlogD is None:
            raise ValueError('dlogD: shape (n_dir, n_omega) is needed')

        def run(K, omega, items, bryan=None, **common):
            return response.element_default_model_response(K, omega, items, dlogD, alpha=alpha, **common)
        return self._posterior_elements(res, run, {}, ('dA', 'dH'), 'compute the default-model response of', timing=timing)

    def resample_errors(self, bins, method='jackknife', block=1, n_resamples=None, seed=None, alpha=None,
                        alpha_mode='per_resample', windows=None, functionals=None, pointwise=True, keep_samples=False,
                        timing=None, quantiles=None):
        """:meth:`TauMaxEnt.resample_errors` for every matrix element: ``bins`` are those the last ``set_G_tau_bins`` /
        ``set_G_iw_bins`` call received; all elements see the same resamples (bins are joint measurements).  The rotated
        data of all sets come from one ``mxe_bins_resample`` call on the first device, every phase is one launch per
        device for all elements and resamples, each element with ONE data set.  Returns a dict of arrays laid out like
        :meth:`posterior_errors`' (matrix indices, then the complex index with ``use_complex``; elements that were not
        computed hold NaN, those that follow from hermiticity are filled from their partners); ``info['n_datasets']``
        and ``info['n_elements']`` per phase.  ``quantiles`` (bootstrap only): the ``*_quantiles`` of
        :meth:`TauMaxEnt.resample_errors` per element; a mirrored imaginary part holds minus its partner's quantile at
        1 - q."""
        from . import resampling
        return resampling.elementwise_resample_errors(self, bins, method=method, block=block, n_resamples=n_resamples,
                                                      seed=seed, alpha=alpha, alpha_mode=alpha_mode, windows=windows,
                                                      functionals=functionals, pointwise=pointwise,
                                                      keep_samples=keep_samples, timing=timing, quantiles=quantiles)

    def parametric_bootstrap(self, result=None, n_mock=200, seed=None, alpha=None, alpha_mode='per_mock',
                             quantiles=(0.16, 0.5, 0.84), windows=None, functionals=None, pointwise=True, keep_samples=False,
                             keep_data=False, timing=None):
        """:meth:`TauMaxEnt.parametric_bootstrap` for every matrix element of ``result`` (default: ``run()``): the mocks of
        all sets of the job come from one ``mxe_mock_data`` call on the first device -- every element with its own error
        bars or covariance --, every phase is one launch per device for all elements and mocks.  The stream of an element
        is ``posterior.stream_id(flat matrix index, complex index, 1, 0)``: it draws the same mocks alone and inside a
        matrix, and different elements draw independently.  Returns a dict of arrays laid out like
        :meth:`resample_errors`' (elements that were not computed hold NaN, -1 for indices; those that follow from
        hermiticity are filled from their partners, the imaginary part's values with the other sign and its quantiles
        minus the partner's at 1 - q, which is what the sign does to the order); ``G_mock`` is padded with NaN to the
        longest element."""
        from . import mock
        return mock.elementwise_parametric_bootstrap(self, result=result, n_mock=n_mock, seed=seed, alpha=alpha,
                                                     alpha_mode=alpha_mode, quantiles=quantiles, windows=windows,
                                                     functionals=functionals, pointwise=pointwise,
                                                     keep_samples=keep_samples, keep_data=keep_data, timing=timing)

    def cross_validate(self, bins, n_folds=5, rule='min', result=None, keep_rows=False, timing=None):
        """:meth:`TauMaxEnt.cross_validate` for every matrix element: ``bins`` are those the last ``set_G_tau_bins`` /
        ``set_G_iw_bins`` call received; all elements see the same folds (bins are joint measurements).  The rotated data
        of the folds of all sets come from one ``mxe_bins_resample`` call on the first device, every phase is one launch
        per device for the 1 + K scans of all elements and one ``mxe_cv_score`` call per device behind it.  Returns a dict
        of arrays laid out like :meth:`resample_errors`' (matrix indices, then the complex index with ``use_complex``;
        elements that were not computed hold NaN, -1 for indices; those that follow from hermiticity are filled from
        their partners, ``A_cv`` and ``A_one_se`` of an imaginary part with the other sign); ``z`` is padded with NaN to
        the largest rank; ``left_out`` is a dict keyed by element.  With ``result``, every computed element gets its
        ``'CrossValidationAnalyzer'`` entry."""
        from . import cross_validation
        return cross_validation.elementwise_cross_validate(self, bins, n_folds=n_folds, rule=rule, result=result,
                                                           keep_rows=keep_rows, timing=timing)

    def default_model_scan(self, models, prior=None, alpha='bryan', windows=None, functionals=None, pointwise=True,
                           keep_models=True, timing=None):
        """:meth:`TauMaxEnt.default_model_scan` for every matrix element: the same ``models`` go to every computed element
        (the off-diagonal ones with their plus-minus entropy), all models of all elements of a phase in one launch per
        device, reduced there by ``mxe_evidence_reduce``.  Returns a dict of arrays laid out like
        :meth:`resample_errors`' (matrix indices, then the complex index with ``use_complex``; elements that were not
        computed hold NaN, -1 for indices; those that follow from hermiticity are filled from their partners, the
        imaginary part's spectra and weights with the other sign).  The object's default models and its last result are
        not changed."""
        from . import model_scan
        return model_scan.elementwise_default_model_scan(self, models, prior=prior, alpha=alpha, windows=windows,
                                                         functionals=functionals, pointwise=pointwise,
                                                         keep_models=keep_models, timing=timing)

    def check_bins(self, bins, basis='eigen'):
        """:meth:`TauMaxEnt.check_bins` for every set of the last ``set_G_*_bins`` call (``bins`` are the ones it
        received), all sets in one ``mxe_bins_check`` call on the first device.  Returns a dict keyed like
        ``bin_statistics``, each entry the dict of :func:`maxent_amd.bin_checks.summarize`, and a top-level
        ``recommended_block``: the largest over the elements, None if any element gives None."""
        from . import bin_checks
        return bin_checks.elementwise_check_bins(self, bins, basis=basis)

    def positivity(self, result=None, alpha=None, floor=0.0, keep_vectors=False, back_continue=True):
        """Is the continued A(omega), taken as a matrix, positive semi-definite -- and what is the nearest spectrum that
        is?  Element-wise continuation usually does not give a positive matrix (:class:`PoormanMaxEnt` usually improves
        it).  The matrix is assembled from ``result`` (default: ``run()``): ``A_out`` / ``A`` of the elements with their
        hermitian mirror, ``zero_elements`` as zeros; an element that was never continued (NaN) raises ValueError, and
        the message names it.  ``alpha``: None -- ``A_out`` of the default analyzer --, an analyzer name, an integer
        index into the alpha mesh, or ``'all'``: every alpha of the mesh, the outputs then carry a leading ``n_alpha``
        axis (at which alpha does positivity break?).  All eigenproblems -- one per frequency and alpha -- are one
        ``mxe_hermitian_eig`` launch; with several GPUs it runs on the first device (the matrices are assembled from host
        arrays).  Returns the dict of :func:`maxent_amd.positivity.matrix_positivity` (weights: the ``delta`` of the omega
        mesh) and ``alpha``, what was taken.  Clipping adds weight: the sum rule of ``A_psd`` is off by exactly
        ``negative_weight``.

        With ``back_continue`` and a single alpha, per element (laid out like the matrix, then the complex index with
        ``use_complex``; NaN for elements that were not computed, mirrored ones filled from their partners):
        ``G_rec_psd`` = K_delta A_psd, the data the repaired spectrum stands for (a host product with the un-blurred
        ``K_delta``), and ``chi2`` / ``chi2_psd``: the misfit of A and of A_psd in that element's own data space (its
        ``err``, its rotation after ``set_cov``) -- what the repair costs.  The result must have been made from the data
        the object holds now."""
        from . import positivity
        return positivity.elementwise_positivity(self, result=result, alpha=alpha, floor=floor, keep_vectors=keep_vectors,
                                                 back_continue=back_continue)

    def _direct_input(self, worker):
        """G(tau) came as one array and the errors are plain (no covariance): specs can be cut from the
        arrays without sending every element through the worker's setters"""
        return (getattr(self, '_array_input', False) and self.error_dimension == 1 and
                worker.K.rotation is None and not isinstance(self.error, str))

    def _share_decomposition(self):
        """the two workers have kernels of their own; where these are the same matrix (same class, tau,
        omega, beta, no preblur on one side only) the second takes the SVD of the first instead of
        repeating it"""
        a, b = self.maxent_diagonal.K, self.maxent_offdiagonal.K
        if a is b or type(a) is not type(b) or getattr(a, 'kind', None) is None or \
                a.rotation is not None or b.rotation is not None or \
                getattr(a, 'symmetric', None) != getattr(b, 'symmetric', None):
            return
        try:
            same = (np.array_equal(np.asarray(a.data_variable), np.asarray(b.data_variable)) and
                    np.array_equal(np.asarray(a.omega), np.asarray(b.omega)) and a.beta == b.beta and
                    a.svd_backend == b.svd_backend)
        except Exception:
            return
        if not same:
            return
        src, dst = (a, b) if b._U is None else ((b, a) if a._U is None else (None, None))
        if src is None:
            return
        src.S
        dst._U, dst._S, dst._V = src._U, src._S, src._V
        dst._last_threshold = src._last_threshold

    def _jobs(self, which):
        """the (element, re) list of a phase -- ONE list object per (phase, shape, hermiticity, complex) of this object, with the
        index arrays cut from it (``_plans``): the lists and arrays of a 16 x 16 matrix cost 0.15 ms per run to make again"""
        key = (which, tuple(self.shape), bool(self.use_hermiticity), bool(self.use_complex))
        plans = self.__dict__.setdefault('_plans', {})
        plan = plans.get(key)
        if plan is None:
            if which == 'diag':
                jobs = [((i, i), True) for i in range(self.shape[0])]
            else:
                jobs = []
                for i in range(self.shape[0]):
                    for j in range(self.shape[1]):
                        if i == j or (self.use_hermiticity and i > j):
                            continue
                        for re in ([True, False] if self.use_complex else [True]):
                            jobs.append(((i, j), re))
            ii = np.fromiter((e[0] for e, _ in jobs), dtype=np.intp, count=len(jobs))
            jj = np.fromiter((e[1] for e, _ in jobs), dtype=np.intp, count=len(jobs))
            real_part = np.fromiter((bool(re) for _, re in jobs), dtype=bool, count=len(jobs)) | (ii == jj)
            plan = plans[key] = dict(jobs=jobs, ii=ii, jj=jj, real_part=real_part, all_real=bool(real_part.all()))
            plans[id(jobs)] = plan
        return plan['jobs']

    def _diag_jobs(self):
        return self._jobs('diag')

    def _offdiag_jobs(self):
        return self._jobs('off')

    def run_diagonal(self):
        """all diagonal elements (reference elementwise_maxent.py:223-242)."""
        self.maxent_diagonal.logtaker.message(
            VerbosityFlags.ElementInfo, 'Calculating diagonal elements.')
        res = self._run_batch(self.maxent_diagonal, self._diag_jobs())
        self._mark_imaginary_diagonal(res)
        return res

    def run_offdiagonal(self):
        """all off-diagonal elements (reference elementwise_maxent.py:244-268)."""
        self.maxent_offdiagonal.logtaker.message(
            VerbosityFlags.ElementInfo, 'Calculating off-diagonal elements.')
        return self._run_batch(self.maxent_offdiagonal, self._offdiag_jobs())

    def run(self):
        """all elements (reference elementwise_maxent.py:270-285)"""
        return self.run_async().result()

    def run_async(self, in_flight=1):
        """Start :meth:`run` and return at once: the data are staged and the kernel is LAUNCHED, nothing is waited for.
        ``handle.result()`` waits, builds records and analyzers and returns the :class:`MaxEntResult` -- the one ``run()``
        returns, field for field.  In between the caller is free: a self-consistency loop that continues several Green
        functions per iteration (reference: ``ElementwiseMaxEnt.run()`` once per job, elementwise_maxent.py:270-285) starts
        them all and collects them afterwards,

            handles = [ew.run_async(in_flight=len(jobs)) for ew in jobs]
            results = [h.result() for h in handles]          # = maxent_amd.run_many(jobs)

        and the GPU works on all of them side by side (every object gets device contexts -- a stream -- of its own) while
        the host prepares the next and finishes the previous one.  ``in_flight``: how many jobs the caller keeps in flight
        (``mxe_opts.in_flight``): each is then cut into fewer cold-started pieces, n of them fill the GPU together (four 16 x 16
        x 100-alpha jobs: 0.65 instead of 0.83 ms of GPU time each).  The answers do not depend on it beyond the stopping
        tolerance.  A subclass with phases of its own (PoormanMaxEnt: the off-diagonal elements need the finished diagonal
        ones) runs to the end in this call."""
        cls = type(self)
        if (cls.run_diagonal is not ElementwiseMaxEnt.run_diagonal or
                cls.run_offdiagonal is not ElementwiseMaxEnt.run_offdiagonal):
            self.run_diagonal()              # (a subclass with phases of its own: PoormanMaxEnt needs the
            self.run_offdiagonal()           #  diagonal results before the off-diagonal elements start)
            return PendingRun(self, None)
        pending = self.__dict__.get('_pending_run')
        if pending is not None and not pending.done:
            raise RuntimeError('this object has a run in flight: take its result() first')
        # both phases in ONE launch where the two workers share the kernel's decomposition
        self.maxent_diagonal.logtaker.message(VerbosityFlags.ElementInfo, 'Calculating diagonal elements.')
        later = []
        diag = self._prepare_batch(self.maxent_diagonal, self._diag_jobs(), defer_last_load=later)
        self.maxent_offdiagonal.logtaker.message(VerbosityFlags.ElementInfo, 'Calculating off-diagonal elements.')
        off = self._prepare_batch(self.maxent_offdiagonal, self._offdiag_jobs(), defer_last_load=later)
        def load_last():                              # (the workers as the reference leaves them: loaded with their last element)
            while later:
                worker, element, re = later.pop(0)
                self._load_element(worker, element, re)
        try:
            wait = self._solve_batches([diag, off], defer=True, in_flight=in_flight)
        except BaseException:
            load_last()
            raise

        def finish():
            # (before the wait, beside the kernel -- and not between this job's launch and the next job's: with four jobs in flight
            #  the 0.08 ms per job delayed every later launch)
            load_last()
            wait()
            if self._finish_deferred([diag, off]):
                self._mark_imaginary_diagonal(self.maxent_result)
                return self.maxent_result
            res = self._finish_batch(diag)
            self._mark_imaginary_diagonal(res)
            return self._finish_batch(off)
        handle = PendingRun(self, finish)
        object.__setattr__(self, '_pending_run', handle)
        return handle

    def _mark_imaginary_diagonal(self, res):
        if self.use_complex:
            for i in range(self.shape[0]):
                if (i, i, 1) not in res._zero_elements:
                    res._zero_elements.append((i, i, 1))

    # ---- input ----------------------------------------------------------------
    def set_G(self, G_mat, set_G_element, determine_shape):
        """generic entry: ``set_G_element(maxent, G_mat, elem, re)`` feeds one
        element to a worker (reference elementwise_maxent.py:287-315)."""
        self.G_mat = G_mat
        self.set_G_element = set_G_element
        self.determine_shape = determine_shape
        self.maxent_result = None
        object.__setattr__(self, '_array_input', False)
        object.__setattr__(self, '_n_iw', None)

    def set_G_tau(self, *args, **kwargs):
        raise NotImplementedError('set_G_tau needs TRIQS Green functions; '
                                  'use set_G_tau_data')

    set_G_iw = set_G_tau

    def _set_array(self, cls, grid, G, put, n_iw=None, direct=True, assign_grid=True, **params):
        """the common tail of the array setters: both workers get their kernel of class ``cls`` on ``grid`` (``params``:
        its further constructor arguments), and ``put(worker, grid, x)`` -- the worker's setter -- feeds an element: x is
        the real part of G[i, j], or its imaginary part for the second scan of an off-diagonal element.  ``n_iw``: the
        part holds the stacked ``[Re ; Im]`` of that many complex values, and travels to the worker folded.  ``direct``:
        whether ``_direct_input`` may cut the specs from the array."""
        def feed(maxent, G_mat, elem, re):
            x = G_mat[1][elem]
            x = np.real(x) if re else np.imag(x)
            put(maxent, G_mat[0], x if n_iw is None else x[:n_iw] + 1j * x[n_iw:])
        for worker in (self.maxent_diagonal, self.maxent_offdiagonal):
            worker._use_kernel(cls, grid, assign_grid=assign_grid, **params)
        self.set_G((grid, G), feed, lambda G_mat: G_mat[1].shape[:2])
        object.__setattr__(self, '_array_input', direct)
        object.__setattr__(self, '_n_iw', n_iw)

    @staticmethod
    def _hermitian_split(G, stacked=True):
        """complex (M, M, n) data of a hermitian A(omega) as the data of the real-part problems, (G_ij + G_ji) / 2 =
        K Re A_ij, in the real part and of the imaginary-part problems, (G_ij - G_ji) / (2i) = K Im A_ij, in the imaginary
        part -- the feed and the arrays of _prepare_batch pick them the way they pick the parts of G(tau); ``stacked``:
        each as ``[Re ; Im]`` (2 n values), otherwise their real parts (n values)"""
        Gt = G.transpose(1, 0, 2)
        re_part = 0.5 * (G + Gt)                    # K Re A_ij
        im_part = (G - Gt) / 2j                     # K Im A_ij
        if not stacked:
            return re_part.real + 1j * im_part.real
        return np.concatenate([re_part.real, re_part.imag], axis=-1) + \
            1j * np.concatenate([im_part.real, im_part.imag], axis=-1)

    def set_G_tau_data(self, tau, G_tau, *args, **kwargs):
        """``G_tau``: (M, N, T) array (reference elementwise_maxent.py:373-395)."""
        # (a worker's kernel that stays gets the grid with its first element, not here)
        self._set_array(kernels.TauKernel, tau, G_tau, lambda tm, t, x: tm.set_G_tau_data(t, x, *args, **kwargs),
                        direct=not args and not kwargs, assign_grid=False)

    def set_G_iw_data(self, iomega, G_iw, beta=None):
        """``G_iw``: complex (M, N, n_iw) array of G_ij(i omega_n) on the real Matsubara frequencies ``iomega``
        (:meth:`TauMaxEnt.set_G_iw_data`).  Element (i, j) is continued from the parts of G that belong to the real
        and the imaginary part of A_ij: for a hermitian A(omega), (G_ij + G_ji) / 2 = K Re A_ij and
        (G_ij - G_ji) / (2i) = K Im A_ij (the latter with ``use_complex``); a diagonal element is G_ii itself.
        Every problem is the stacked real one of an IOmegaKernel, and all elements share its decomposition."""
        iomega = np.asarray(iomega, dtype=float)
        G_iw = np.asarray(G_iw)
        if G_iw.ndim != 3 or G_iw.shape[0] != G_iw.shape[1] or G_iw.shape[2] != len(iomega):
            raise AssertionError('G_iw must be (M, M, n_iw) with n_iw = len(iomega)')
        self._set_G_iw_stacked(iomega, self._hermitian_split(G_iw), beta)

    def _set_G_iw_stacked(self, iomega, stacked, beta):
        """the tail of :meth:`set_G_iw_data`: ``stacked`` (M, M, 2 n_iw) as described there"""
        self._set_array(kernels.IOmegaKernel, iomega, stacked, lambda tm, iw, z: tm.set_G_iw_data(iw, z, beta),
                        n_iw=len(iomega), beta=beta)

    def set_chi_tau_data(self, tau, chi, beta=None, symmetric=False):
        """``chi``: (M, N, T) array of bosonic chi_ij(tau) (:meth:`TauMaxEnt.set_chi_tau_data`); the real part of an
        element is continued to Re A_ij, with ``use_complex`` the imaginary part to Im A_ij, as for G(tau)."""
        tau = np.asarray(tau, dtype=float)
        chi = np.asarray(chi)
        if chi.ndim != 3 or chi.shape[2] != len(tau):
            raise AssertionError('chi must be (M, N, n_tau) with n_tau = len(tau)')
        self._set_array(kernels.BosonicTauKernel, tau, chi, lambda tm, t, x: tm.set_chi_tau_data(t, x, beta, symmetric),
                        beta=beta, symmetric=bool(symmetric))

    def set_chi_iw_data(self, inu, chi_iw, beta=None, symmetric=False):
        """``chi_iw``: complex (M, M, n) array of bosonic chi_ij(i nu_n) (:meth:`TauMaxEnt.set_chi_iw_data`).  The
        hermitian split of :meth:`set_G_iw_data` applies: (chi_ij + chi_ji) / 2 = K Re A_ij and
        (chi_ij - chi_ji) / (2i) = K Im A_ij (the latter with ``use_complex``).  ``symmetric``: the real parts of
        these (n values per element) are the data of the real half-axis kernel."""
        inu = np.asarray(inu, dtype=float)
        chi_iw = np.asarray(chi_iw)
        if chi_iw.ndim != 3 or chi_iw.shape[0] != chi_iw.shape[1] or chi_iw.shape[2] != len(inu):
            raise AssertionError('chi_iw must be (M, M, n) with n = len(inu)')
        self._set_array(kernels.BosonicIOmegaKernel, inu, self._hermitian_split(chi_iw, stacked=not symmetric),
                        lambda tm, nu, z: tm.set_chi_iw_data(nu, z, beta, symmetric),
                        n_iw=None if symmetric else len(inu), beta=beta, symmetric=bool(symmetric))

    def set_G_l_data(self, G_l, beta, l=None):
        """``G_l``: (M, N, n_l) array of Legendre coefficients of G_ij (:meth:`TauMaxEnt.set_G_l_data`; ``l`` defaults to
        0..n_l-1); the real part of an element is continued to Re A_ij, with ``use_complex`` the imaginary part to
        Im A_ij, as for G(tau)."""
        G_l = np.asarray(G_l)
        if G_l.ndim != 3:
            raise AssertionError('G_l must be (M, N, n_l)')
        self._set_array(kernels.LegendreKernel, TauMaxEnt._legendre_orders(l, G_l.shape[2]), G_l,
                        lambda tm, orders, x: tm.set_G_l_data(x, beta, orders), beta=beta)

    def set_G_tau_filename_pattern(self, filename, dimension, tau_col=0,
                                   G_col_re=1, G_col_im=2, *args, **kwargs):
        """one file per element, name with ``{i}`` and ``{j}``
        (reference elementwise_maxent.py:397-436)."""
        def feed(maxent, G_mat, elem, re):
            maxent.set_G_tau_file(G_mat.format(i=elem[0], j=elem[1]), tau_col,
                                  G_col_re if re else G_col_im, *args, **kwargs)
        self.set_G(filename, feed, lambda G_mat: dimension)

    def set_G_tau_filenames(self, filenames, tau_col=0, G_col_re=1,
                            G_col_im=2, *args, **kwargs):
        """2-d array of file names (reference elementwise_maxent.py:438-470)."""
        def feed(maxent, G_mat, elem, re):
            maxent.set_G_tau_file(G_mat[elem[0]][elem[1]], tau_col,
                                  G_col_re if re else G_col_im, *args, **kwargs)
        self.set_G(filenames, feed, lambda G_mat: np.shape(G_mat))

    def set_error(self, error):
        """float, (T,) or (M, N, T) (reference elementwise_maxent.py:472-487)."""
        self.error = error
        self.error_dimension = 1
        object.__setattr__(self, '_errors_from_bins', False)
        self.put_error = lambda maxent, err: maxent.set_error(err)

    def get_error(self, elem):
        if isinstance(self.error, float):
            return self.error
        if len(np.shape(self.error)) == self.error_dimension:
            return self._stacked_error(self.error)
        return self._stacked_error(self.error[elem])

    def _stacked_error(self, err):
        """Matsubara data: one error bar per frequency serves the real and the imaginary parts of the stacked data"""
        n = self.__dict__.get('_n_iw')
        if n is not None and self.error_dimension == 1 and np.shape(err) == (n,):
            err = np.concatenate([err, err]).astype(float, copy=False)
        return err

    def set_cov(self, cov):
        """(T, T) or (M, N, T, T) (reference elementwise_maxent.py:502-515)."""
        self.error_dimension = 2
        self.error = cov
        object.__setattr__(self, '_errors_from_bins', False)
        self.put_error = lambda maxent, err: maxent.set_cov(err)

    # ---- bins: all sets of the run through ONE mxe_bins_eig call ----------------------------------------
    def _bins_eig(self, shape, sets_of, n_bins, shrinkage=None):
        """``sets_of(i, j)``: the real bins (n_bins, n_data) of the real-part problem of element (i, j) and of its
        imaginary-part problem (None: there is none).  Every set the run needs -- with ``use_hermiticity`` only
        i <= j, imaginary parts only with ``use_complex`` and off the diagonal -- goes down in one call, on the first
        of ``device_ids`` (the preparation is not sharded: the elements' solves are).  Returns
        {(i, j): [statistics of the real part, of the imaginary part or None]}.  ``shrinkage``: as for
        :meth:`TauMaxEnt.set_G_tau_bins`; with ``'auto'`` every set gets its own lambda."""
        from . import device
        lambda_in = device.shrinkage_argument(shrinkage, n_bins)     # (a ValueError before anything is touched)
        M, N = shape
        where, sets = [], []
        for i in range(M):
            for j in range(N):
                if self.use_hermiticity and i > j:
                    continue
                re_set, im_set = sets_of(i, j)
                where.append((i, j, 0))
                sets.append(re_set)
                if self.use_complex and i != j and im_set is not None:
                    where.append((i, j, 1))
                    sets.append(im_set)
        stack = np.ascontiguousarray(np.stack(sets), dtype=float)
        ids = self.device_ids if self.device_ids else (self.maxent_diagonal._device_for_bins(),)
        if lambda_in is None:
            self.maxent_diagonal._warn_few_bins(n_bins, stack.shape[-1])
            stats = device.bins_eig(stack, self.cov_threshold, device=ids[0])
        else:
            stats = device.bins_eig_shrunk(stack, self.cov_threshold, shrinkage, device=ids[0])
            self.maxent_diagonal._note_shrinkage(n_bins, stack.shape[-1], [st['shrinkage'] for st in stats])
        table, public = {}, {}
        for (i, j, c), st in zip(where, stats):
            st = dict(st, n_bins=n_bins)
            if st['rank'] == 0 and np.any(st['mean'] != 0.0):
                raise AssertionError('bins of element {} {}: no eigenvalue of the covariance of the mean is above '
                                     'cov_threshold = {}'.format(i, j, self.cov_threshold))
            table.setdefault((i, j), [None, None])[c] = st if st['rank'] > 0 else None
            public[(i, j, c) if self.use_complex else (i, j)] = st
        object.__setattr__(self, 'bin_statistics', public)
        return table

    def _means_of_bins(self, table, shape, n_data):
        """the (M, N, n_data) array of the means: real parts' + 1j imaginary parts' with ``use_complex``"""
        G = np.zeros(tuple(shape) + (n_data,), dtype=complex if self.use_complex else float)
        for (i, j), (st_re, st_im) in table.items():
            if st_re is not None:
                G[i, j] = G[i, j] + st_re['mean']
            if st_im is not None:
                G[i, j] = G[i, j] + 1j * st_im['mean']
        return G

    def _put_eigenbases(self, table):
        """errors from bins: ``get_error`` gives the element's pair of statistics, ``_load_element`` picks the part that
        is loaded and ``put_error`` hands the worker its precomputed (sigma, T), where ``set_cov`` would decompose a matrix"""
        def put(maxent, st):
            if st is None:
                maxent.set_error(1.0)        # (a part without data -- all bins zero --: below G_threshold, nothing is solved)
            else:
                maxent._set_eigenbasis(st['sigma'], st['T'])
        self.error_dimension = 2
        self.error = table                   # (get_error(elem) -> table[elem])
        self.put_error = put
        object.__setattr__(self, '_errors_from_bins', True)

    def set_G_tau_bins(self, tau, bins, shrinkage=None):
        """``bins``: (n_bins, M, N, n_tau) array of independent estimates of G_ij(tau) (:meth:`TauMaxEnt.set_G_tau_bins`),
        complex with ``use_complex``: real and imaginary parts are then sets of their own, each with the covariance of
        its own mean.  The eigenbases of all elements the run needs come from one ``mxe_bins_eig`` call;
        ``bin_statistics[(i, j)]`` (``[(i, j, c)]`` with ``use_complex``) holds ``mean``, ``sigma``, ``T``, ``rank`` and
        ``n_bins``.  ``shrinkage``: as for :meth:`TauMaxEnt.set_G_tau_bins`, all sets still in one call
        (``mxe_bins_eig_shrunk``), every set with its own lambda.  Not in the reference."""
        tau = np.asarray(tau, dtype=float)
        bins = TauMaxEnt._check_bins(tau, bins, 'G(tau) bins')
        if bins.ndim != 4:
            raise AssertionError('G(tau) bins must be (n_bins, M, N, n_tau); their shape is {}'.format(bins.shape))
        cplx = np.iscomplexobj(bins)
        if cplx and not self.use_complex:
            raise AssertionError('complex G(tau) bins need use_complex=True')

        def sets_of(i, j):
            b = bins[:, i, j, :]
            return b.real, (b.imag if cplx else None)
        table = self._bins_eig(bins.shape[1:3], sets_of, bins.shape[0], shrinkage)
        self.set_G_tau_data(tau, self._means_of_bins(table, bins.shape[1:3], len(tau)))
        self._put_eigenbases(table)

    def set_G_iw_bins(self, iomega, bins, beta=None, shrinkage=None):
        """``bins``: complex (n_bins, M, M, n_iw) array of independent estimates of G_ij(i omega_n).  Every bin is split
        as in :meth:`set_G_iw_data` -- (G_ij + G_ji) / 2 = K Re A_ij, (G_ij - G_ji) / (2i) = K Im A_ij (the latter with
        ``use_complex``) -- and unfolded to stacked real values, whose mean and covariance enter as in
        :meth:`set_G_tau_bins`."""
        iomega = np.asarray(iomega, dtype=float)
        bins = TauMaxEnt._check_bins(iomega, bins, 'G(i omega_n) bins', per_point=2)
        if bins.ndim != 4 or bins.shape[1] != bins.shape[2]:
            raise AssertionError('G(i omega_n) bins must be (n_bins, M, M, n_iw); their shape is {}'.format(bins.shape))

        def sets_of(i, j):
            a, b = bins[:, i, j, :], bins[:, j, i, :]
            re_part = 0.5 * (a + b)
            re_set = np.concatenate([re_part.real, re_part.imag], axis=-1)
            if not self.use_complex or i == j:
                return re_set, None
            im_part = (a - b) / 2j
            return re_set, np.concatenate([im_part.real, im_part.imag], axis=-1)
        table = self._bins_eig(bins.shape[1:3], sets_of, bins.shape[0], shrinkage)
        self._set_G_iw_stacked(iomega, self._means_of_bins(table, bins.shape[1:3], 2 * len(iomega)), beta)
        self._put_eigenbases(table)

    def set_G_l_bins(self, bins, beta, l=None, shrinkage=None):
        """``bins``: (n_bins, M, N, n_l) array of independent estimates of the Legendre coefficients of G_ij
        (:meth:`TauMaxEnt.set_G_l_bins`), complex with ``use_complex``; everything else as :meth:`set_G_tau_bins`."""
        bins = np.asarray(bins)
        if bins.ndim != 4:
            raise AssertionError('G_l bins must be (n_bins, M, N, n_l); their shape is {}'.format(bins.shape))
        l = TauMaxEnt._legendre_orders(l, bins.shape[-1])
        bins = TauMaxEnt._check_bins(l, bins, 'G_l bins')
        cplx = np.iscomplexobj(bins)
        if cplx and not self.use_complex:
            raise AssertionError('complex G_l bins need use_complex=True')

        def sets_of(i, j):
            b = bins[:, i, j, :]
            return b.real, (b.imag if cplx else None)
        table = self._bins_eig(bins.shape[1:3], sets_of, bins.shape[0], shrinkage)
        self.set_G_l_data(self._means_of_bins(table, bins.shape[1:3], len(l)), beta, l)
        self._put_eigenbases(table)

    def get_tau(self):
        d = self.maxent_diagonal.get_data_variable()
        o = self.maxent_offdiagonal.get_data_variable()
        if np.all(d == o):
            return d
        raise Exception('tau not uniquely defined. Use self.maxent_diagonal.tau '
                        'or self.maxent_offdiagonal.tau!')

    def set_tau(self, tau, **kwargs):
        self.maxent_diagonal.set_tau(tau, **kwargs)
        self.maxent_offdiagonal.set_tau(tau, **kwargs)

    tau = property(get_tau, set_tau)

    @property
    def shape(self):
        try:
            return self.determine_shape(self.G_mat)
        except Exception as e:
            raise Exception('Cannot determine shape. ({})'.format(e))


class DiagonalMaxEnt(ElementwiseMaxEnt):
    """diagonal elements only (reference elementwise_maxent.py:549-559)."""

    def run(self):
        self.run_diagonal()
        return self.maxent_result

    def run_offdiagonal(self):
        raise TypeError('DiagonalMaxEnt cannot run for off-diagonals.')

    def positivity(self, *args, **kwargs):
        raise NotImplementedError('DiagonalMaxEnt.positivity: a job without off-diagonal elements has no matrix to test -- a '
                                  'diagonal A(omega) is positive where its elements are; use ElementwiseMaxEnt or PoormanMaxEnt, '
                                  'or maxent_amd.matrix_positivity on a matrix of your own')


class PoormanMaxEnt(ElementwiseMaxEnt):
    r"""off-diagonals with :math:`D_{ij} = \sqrt{A_{ii}A_{jj}} + \epsilon`
    from the analyzed diagonals (reference elementwise_maxent.py:562-653)."""

    def __init__(self, analyzer_offdiag_D='LineFitAnalyzer',
                 D_add_constant=1.e-6, *args, **kwargs):
        super(PoormanMaxEnt, self).__init__(*args, **kwargs)
        self.analyzer_offdiag_D = analyzer_offdiag_D
        self.D_add_constant = D_add_constant

    def _posterior_models(self, jobs, result):
        ar = result.analyzer_results
        models = []
        for (i, j), re in jobs:
            A1 = (ar[i][i][0] if self.use_complex else ar[i][i])[self.analyzer_offdiag_D]['A_out']
            A2 = (ar[j][j][0] if self.use_complex else ar[j][j])[self.analyzer_offdiag_D]['A_out']
            models.append(DataDefaultModel(np.sqrt(A1 * A2) + self.D_add_constant, self.omega))
        return models

    def resample_errors(self, *args, **kwargs):
        raise NotImplementedError('PoormanMaxEnt.resample_errors: the default model of an off-diagonal element is built from '
                                  'the diagonal results, so every resample would need the diagonal results of that resample '
                                  'first -- two dependent launches per resample, which this driver does not do; use '
                                  'ElementwiseMaxEnt or DiagonalMaxEnt')

    def parametric_bootstrap(self, *args, **kwargs):
        raise NotImplementedError('PoormanMaxEnt.parametric_bootstrap: the default model of an off-diagonal element is built '
                                  'from the diagonal results, so every mock would need the diagonal results of that mock '
                                  'first -- two dependent launches per mock, which this driver does not do; use '
                                  'ElementwiseMaxEnt or DiagonalMaxEnt')

    def cross_validate(self, *args, **kwargs):
        raise NotImplementedError('PoormanMaxEnt.cross_validate: the default model of an off-diagonal element is built from '
                                  'the diagonal results, so every fold would need the diagonal results of that fold first '
                                  '-- two dependent launches per fold, which this driver does not do; use '
                                  'ElementwiseMaxEnt or DiagonalMaxEnt')

    def default_model_scan(self, *args, **kwargs):
        raise NotImplementedError('PoormanMaxEnt.default_model_scan: the default model of an off-diagonal element is built '
                                  'from the diagonal results, so it is not the caller\'s to choose; use ElementwiseMaxEnt or '
                                  'DiagonalMaxEnt')

    def run_offdiagonal(self):
        self.prepare_maxent_result(overwrite=False)
        self.maxent_offdiagonal.logtaker.message(
            VerbosityFlags.ElementInfo,
            'Calculating off-diagonal elements using default model from '
            'diagonal solution')
        ar = self.maxent_result.analyzer_results
        jobs = self._offdiag_jobs()
        models = []
        for (i, j), re in jobs:
            if self.use_complex:
                A1 = ar[i][i][0][self.analyzer_offdiag_D]['A_out']
                A2 = ar[j][j][0][self.analyzer_offdiag_D]['A_out']
            else:
                A1 = ar[i][i][self.analyzer_offdiag_D]['A_out']
                A2 = ar[j][j][self.analyzer_offdiag_D]['A_out']
            models.append(DataDefaultModel(
                np.sqrt(A1 * A2) + self.D_add_constant, self.omega))
        return self._run_batch(self.maxent_offdiagonal, jobs,
                               per_job_D=models)
