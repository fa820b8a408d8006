"""The planner of mxe_chains_finish (mxe::plan_finish, maxent_amd/csrc/mxe_plan.h) on the host: `plan_dump finish`, the
stand-alone program of tools/plan_dump.cpp (built with the address and undefined-behaviour sanitizers where the compiler
links them), is fed synthetic FinishInputs and its FinishPlan is checked against expectations derived by hand from the rules
(DESIGN.md section 4), and against the invariants of every plan on seeded random inputs.  Integers are compared exactly,
alphas to a relative 1e-14: a few roundings of pow and one product between libm and numpy."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from plan_dump_build import plan_dump_binary, run_plan_dump

RATIO, RUNG_ITERS, COARSE, RUNGS_MAX = 1.3, 10, 1.6, 40
MC_GAVE_UP = 32          # iterations after which the lock-step kernel gives an alpha up
RTOL = 1e-14


@pytest.fixture(scope='session')
def plan_dump(tmp_path_factory):
    return plan_dump_binary(tmp_path_factory)


def case(alpha, open_at=(), rows=200, chain_elem=None, maxiter=100, n_iter=None, n_evals=None, env=None):
    """alpha [n_alpha] or [n_chain][n_alpha].  Every problem converged after 5 iterations / 7 evaluations except those of
    open_at (flat indices): not converged after MC_GAVE_UP iterations.  n_iter / n_evals: {flat index: value} overrides"""
    a = np.atleast_2d(np.asarray(alpha, dtype=float))
    n_chain, n_alpha = a.shape
    P = n_chain * n_alpha
    conv, nit, nev = np.ones(P, dtype=int), np.full(P, 5), np.full(P, 7)
    for i in open_at:
        conv[i], nit[i], nev[i] = 0, MC_GAVE_UP, MC_GAVE_UP + 8
    for i, v in (n_iter or {}).items():
        nit[i] = v
    for i, v in (n_evals or {}).items():
        nev[i] = v
    rows = [rows] * n_chain if np.isscalar(rows) else list(rows)
    return dict(alpha=a, conv=conv, nit=nit, nev=nev, rows=rows, chain_elem=list(chain_elem) if chain_elem is not None else list(range(n_chain)),
                maxiter=maxiter, env=dict(env or {}))


def text_of(c):
    n_chain, n_alpha = c['alpha'].shape
    ints = lambda key, v: key + ' ' + ' '.join(str(int(x)) for x in v)
    w = ['n_chain %d n_alpha %d maxiter %d' % (n_chain, n_alpha, c['maxiter'])]
    w += ['env %s %r' % (k, float(v)) for k, v in sorted(c['env'].items())]
    w += [ints('rows', c['rows']), ints('chain_elem', c['chain_elem']), 'alpha ' + ' '.join(repr(float(x)) for x in c['alpha'].ravel()),
          ints('converged', c['conv']), ints('n_iter', c['nit']), ints('n_evals', c['nev'])]
    return '\n'.join(w) + '\n'


def parse(out):
    lines = out.split('\n')
    p, i = {}, 0
    while i < len(lines) and lines[i]:
        key, val = lines[i].split()
        i += 1
        if key in ('runs', 'entries', 'open'):
            rows = [r.split() for r in lines[i:i + int(val)]]
            i += int(val)
            if key == 'runs':
                p['runs'] = [dict(elem=int(r[0]), entry0=int(r[1]), len=int(r[2]), start=(bool(int(r[3])), int(r[4]))) for r in rows]
            elif key == 'entries':
                p['alpha'], p['out'], p['budget'] = [float(r[0]) for r in rows], [int(r[1]) for r in rows], [int(r[2]) for r in rows]
            else:
                p['open'] = [int(r[0]) for r in rows]
        else:
            p[key] = int(val)
    return p


def open_of(c):
    """what the pass solves again: not converged, iterations of maxiter left"""
    return [int(not cv and it < c['maxiter']) for cv, it in zip(c['conv'], c['nit'])]


def steps_of(c, p):
    """the entries of a plan as steps: (run, problem, the rungs that lead to it)"""
    steps = []
    for r, run in enumerate(p['runs']):
        rungs = []
        for e in range(run['entry0'], run['entry0'] + run['len']):
            if p['out'][e] < 0:
                rungs.append(p['alpha'][e])
            else:
                steps.append((r, p['out'][e], rungs))
                rungs = []
        assert not rungs                                              # a run ends with an alpha of the mesh
    return steps


def check_invariants(c, p):
    n_chain, n_alpha = c['alpha'].shape
    alpha = c['alpha'].ravel()
    env = c['env']
    ratio, no_ladder = max(1.05, env.get('ratio', RATIO)), bool(env.get('no_ladder', 0))
    expected_open = open_of(c)
    assert p['open'] == expected_open and p['n_open'] == sum(expected_open)
    # every open problem is the out of exactly one entry, and no other problem is
    assert sorted(x for x in p['out'] if x >= 0) == [i for i, o in enumerate(expected_open) if o]
    assert p['n_rungs'] == sum(x == -1 for x in p['out']) and all(x >= -1 for x in p['out'])
    assert len(p['alpha']) == len(p['out']) == len(p['budget']) and all(b >= 1 for b in p['budget'])
    if p['n_open'] == 0:
        assert not p['runs'] and not p['out']
    # the entries of a run are contiguous; entry0 and len tile the entry list
    at = 0
    for run in p['runs']:
        assert run['entry0'] == at and run['len'] >= 1
        at += run['len']
    assert at == len(p['out'])
    seen_head = set()
    for r, pk, rungs in steps_of(c, p):
        run = p['runs'][r]
        scan, k = divmod(pk, n_alpha)
        assert run['elem'] == c['chain_elem'][scan]
        assert not (no_ladder and rungs)
        first_of_run = r not in seen_head
        seen_head.add(r)
        if first_of_run:
            # the run starts at the alpha before its first, or at its own record, or at the scan's start vector
            from_v0, index = run['start']
            if k > 0:
                assert (from_v0, index) == (False, pk - 1) and not expected_open[pk - 1]
            elif c['nit'][pk] > 0 or c['nev'][pk] > 0:
                assert (from_v0, index) == (False, pk)
            else:
                assert (from_v0, index) == (True, scan)
        else:
            assert k > 0 and expected_open[pk - 1]
        if not rungs:
            continue
        if k == 0:
            # the head ladder: from N_data / 4 itself down to the first alpha
            assert first_of_run and run['start'] == (True, scan) and rungs[0] == 0.25 * c['rows'][scan]
            chain, capped = rungs + [alpha[pk]], len(rungs) == RUNGS_MAX + 1
        else:
            chain, capped = [alpha[pk - 1]] + rungs + [alpha[pk]], len(rungs) == RUNGS_MAX
        assert len(rungs) <= RUNGS_MAX + (k == 0)
        # rungs lie strictly between their neighbours, monotonically, in steps of at most the ratio
        up = chain[-1] > chain[0]
        assert all((y > x) == up and y != x for x, y in zip(chain, chain[1:]))
        if not capped:
            assert all(max(x / y, y / x) <= ratio * (1 + 1e-12) for x, y in zip(chain, chain[1:]))


def plan(binary, c):
    p = parse(run_plan_dump(binary, text_of(c), 'finish'))
    check_invariants(c, p)
    return p


def entries(p):
    return list(zip(p['alpha'], p['out'], p['budget']))


def assert_entries(p, expected):
    assert [(o, b) for _, o, b in entries(p)] == [(o, b) for _, o, b in expected]
    assert np.allclose(p['alpha'], [a for a, _, _ in expected], rtol=RTOL, atol=0.0)


def fine_mesh(n_alpha=8, top=100.0, ratio=1.2):
    return top / ratio ** np.arange(n_alpha)


def away_from_an_integer(x):
    return abs(x - round(x)) > 1e-6


# ---- empty plans and budgets

def test_all_converged_gives_an_empty_plan(plan_dump):
    p = plan(plan_dump, case(fine_mesh()))
    assert (p['n_open'], p['n_rungs'], p['runs'], entries(p)) == (0, 0, [], [])


def test_an_alpha_that_used_its_maxiter_stays_as_it_is(plan_dump):
    p = plan(plan_dump, case(fine_mesh(), open_at=[3, 4], n_iter={3: 100, 4: 117}))
    assert (p['n_open'], p['n_rungs'], p['runs'], entries(p)) == (0, 0, [], [])
    # ... and the one beside it that did not is a run of its own, from the record of the one before
    a = fine_mesh()
    p = plan(plan_dump, case(a, open_at=[3, 4], n_iter={3: 100}))
    assert p['runs'] == [dict(elem=0, entry0=0, len=1, start=(False, 3))]
    assert_entries(p, [(a[4], 4, 100 - MC_GAVE_UP)])


@pytest.mark.parametrize('n_iter, budget', [(MC_GAVE_UP, 68), (0, 100), (99, 1)])
def test_the_budget_is_what_the_first_pass_left_of_maxiter(plan_dump, n_iter, budget):
    a = fine_mesh()
    p = plan(plan_dump, case(a, open_at=[3], n_iter={3: n_iter}))
    assert_entries(p, [(a[3], 3, budget)])
    assert budget == max(1, 100 - n_iter)


# ---- runs on a fine mesh (ratio 1.2: no rungs)

def test_one_open_alpha_starts_from_the_record_before_it(plan_dump):
    a = fine_mesh()
    p = plan(plan_dump, case(a, open_at=[3]))
    assert (p['n_open'], p['n_rungs']) == (1, 0)
    assert p['runs'] == [dict(elem=0, entry0=0, len=1, start=(False, 2))]
    assert_entries(p, [(a[3], 3, 68)])


def test_consecutive_open_alphas_are_one_run(plan_dump):
    a = fine_mesh()
    p = plan(plan_dump, case(a, open_at=[2, 3, 4], n_iter={4: 0}, n_evals={4: 0}))
    assert p['runs'] == [dict(elem=0, entry0=0, len=3, start=(False, 1))]
    assert_entries(p, [(a[2], 2, 68), (a[3], 3, 68), (a[4], 4, 100)])


def test_two_open_stretches_are_two_runs(plan_dump):
    a = fine_mesh()
    p = plan(plan_dump, case(a, open_at=[1, 2, 5]))
    assert p['runs'] == [dict(elem=0, entry0=0, len=2, start=(False, 0)), dict(elem=0, entry0=2, len=1, start=(False, 4))]
    assert_entries(p, [(a[1], 1, 68), (a[2], 2, 68), (a[5], 5, 68)])


def test_runs_of_two_scans_carry_their_elements(plan_dump):
    a = np.stack([fine_mesh(), fine_mesh(top=70.0)])
    p = plan(plan_dump, case(a, open_at=[2, 8 + 4, 8 + 5], chain_elem=[3, 7]))
    assert p['runs'] == [dict(elem=3, entry0=0, len=1, start=(False, 1)), dict(elem=7, entry0=1, len=2, start=(False, 8 + 3))]
    assert_entries(p, [(a[0, 2], 2, 68), (a[1, 4], 12, 68), (a[1, 5], 13, 68)])
    # the last alpha of a scan and the first of the next are not neighbours
    p = plan(plan_dump, case(a, open_at=[7, 8], chain_elem=[3, 7]))
    assert p['runs'] == [dict(elem=3, entry0=0, len=1, start=(False, 6)), dict(elem=7, entry0=1, len=1, start=(False, 8))]


# ---- rungs between alphas

def between(step, n_rungs_expected, plan_dump, env=None, ratio=RATIO, rung_iters=RUNG_ITERS, top=10.0):
    """the mesh top, top / step, top / step^2 on 8 data points (N_data / 4 = 2: no head ladder); the middle alpha is open"""
    a = np.array([top, top / step, top / step ** 2])
    x = math.log(max(a[0] / a[1], a[1] / a[0])) / math.log(ratio)
    assert away_from_an_integer(x)
    m = n_rungs_expected + 1
    p = plan(plan_dump, case(a, open_at=[1], rows=8, env=env))
    q = (a[1] / a[0]) ** (1.0 / m)
    assert_entries(p, [(a[0] * q ** s, -1, rung_iters) for s in range(1, m)] + [(a[1], 1, 68)])
    assert p['n_rungs'] == n_rungs_expected and p['runs'] == [dict(elem=0, entry0=0, len=m, start=(False, 0))]
    return p, x


def test_the_default_mesh_of_the_reference_takes_two_rungs_per_step(plan_dump):
    """ln 1.9 / ln 1.3 = 2.45: three steps of 1.9^(1/3) = 1.239"""
    p, x = between(1.9, 2, plan_dump)
    assert math.ceil(x) == 3
    chain = [10.0] + p['alpha']
    assert np.allclose([u / v for u, v in zip(chain, chain[1:])], 1.9 ** (1 / 3), rtol=1e-13)


def test_just_above_the_threshold_takes_one_rung(plan_dump):
    """ln 1.61 / ln 1.3 = 1.82: two steps"""
    _, x = between(1.61, 1, plan_dump)
    assert math.ceil(x) == 2


@pytest.mark.parametrize('second', [6.25, 10.0 / 1.5, 10.0 / 1.2])
def test_a_step_of_at_most_the_threshold_takes_none(plan_dump, second):
    assert 10.0 / 6.25 == COARSE and 10.0 / second <= COARSE
    a = np.array([10.0, second, second / 1.2])
    p = plan(plan_dump, case(a, open_at=[1, 2], rows=8))
    assert p['n_rungs'] == 0
    assert_entries(p, [(a[1], 1, 68), (a[2], 2, 68)])


def test_the_rungs_of_one_step_are_capped(plan_dump):
    """ln 1e5 / ln 1.3 = 43.9: 44 steps, capped at 41: 40 rungs of 1e5^(1/41) = 1.324, above 1.3 by design of the cap"""
    p, x = between(1e5, RUNGS_MAX, plan_dump)
    assert math.ceil(x) == 44
    chain = [10.0] + p['alpha']
    assert np.allclose([u / v for u, v in zip(chain, chain[1:])], 1e5 ** (1 / 41), rtol=1e-12) and 1e5 ** (1 / 41) > RATIO


def test_an_ascending_mesh_lays_ascending_rungs(plan_dump):
    p, _ = between(1 / 1.9, 2, plan_dump, top=1.0)
    assert 1.0 < p['alpha'][0] < p['alpha'][1] < p['alpha'][2]
    assert np.allclose(p['alpha'], [1.9 ** (1 / 3), 1.9 ** (2 / 3), 1.9], rtol=RTOL, atol=0.0)


def test_every_coarse_step_of_a_run_gets_its_rungs(plan_dump):
    a = np.array([10.0, 10.0 / 1.9, 10.0 / 1.9 / 1.2, 10.0 / 1.9 / 1.2 / 1.61])
    p = plan(plan_dump, case(a, open_at=[1, 2, 3], rows=8))
    q1, q3 = (a[1] / a[0]) ** (1 / 3), (a[3] / a[2]) ** (1 / 2)
    assert_entries(p, [(a[0] * q1, -1, 10), (a[0] * q1 ** 2, -1, 10), (a[1], 1, 68), (a[2], 2, 68), (a[2] * q3, -1, 10), (a[3], 3, 68)])
    assert p['runs'] == [dict(elem=0, entry0=0, len=6, start=(False, 0))]


# ---- the head of a scan (200 data points: the ladder starts at 50)

def head_ladder(a_to, m, rung_iters=RUNG_ITERS):
    q = (a_to / 50.0) ** (1.0 / m)
    return [(50.0 * q ** s, -1, 3 * rung_iters if s == 0 else rung_iters) for s in range(m)]


def test_a_head_that_was_never_evaluated_walks_down_from_a_quarter_of_the_data_points(plan_dump):
    """first alpha 0.5, the next within 1.6: ln 100 / ln 1.3 = 17.55, 18 rungs from 50 down, budgets 30 and 17 x 10"""
    a = np.array([[60.0, 50.0, 40.0], [0.5, 0.45, 0.4]])
    assert away_from_an_integer(math.log(100) / math.log(RATIO)) and math.ceil(math.log(100) / math.log(RATIO)) == 18
    p = plan(plan_dump, case(a, open_at=[3, 4], n_iter={3: 0, 4: 0}, n_evals={3: 0, 4: 0}))
    assert p['runs'] == [dict(elem=1, entry0=0, len=20, start=(True, 1))]
    assert_entries(p, head_ladder(0.5, 18) + [(0.5, 3, 100), (0.45, 4, 100)])
    assert [b for _, _, b in entries(p)][:18] == [30] + [10] * 17 and p['n_rungs'] == 18


@pytest.mark.parametrize('a, why', [([40.0, 36.0, 30.0], '40 x 1.69 > 50'), ([0.5], 'one alpha'), ([0.5, 0.25, 0.2], 'the next alpha is a factor 2 away')])
def test_heads_without_a_ladder(plan_dump, a, why):
    p = plan(plan_dump, case(np.array(a), open_at=[0], n_iter={0: 0}, n_evals={0: 0}))
    assert p['runs'] == [dict(elem=0, entry0=0, len=1, start=(True, 0))]
    assert_entries(p, [(a[0], 0, 100)])


@pytest.mark.parametrize('n_iter, n_evals', [(MC_GAVE_UP, 40), (0, 3)])
def test_a_head_that_was_evaluated_starts_from_its_own_record(plan_dump, n_iter, n_evals):
    a = np.array([[60.0, 50.0, 40.0], [0.5, 0.45, 0.4]])
    p = plan(plan_dump, case(a, open_at=[3], n_iter={3: n_iter}, n_evals={3: n_evals}))
    assert p['runs'] == [dict(elem=1, entry0=0, len=1, start=(False, 3))]
    assert_entries(p, [(0.5, 3, 100 - n_iter)])


# ---- the environment overrides

def test_no_ladder_removes_every_rung_and_nothing_else(plan_dump):
    a = np.array([[0.5, 0.45, 0.2, 0.19], [20.0, 10.0, 9.0, 2.0]])
    c = case(a, open_at=[0, 1, 2, 5, 7], n_iter={0: 0}, n_evals={0: 0})
    p, off = plan(plan_dump, c), plan(plan_dump, dict(c, env=dict(no_ladder=1)))
    assert p['n_rungs'] > 18 and off['n_rungs'] == 0 and off['n_open'] == p['n_open'] == 5
    assert entries(off) == [e for e in entries(p) if e[1] >= 0]
    assert [(r['elem'], r['start']) for r in off['runs']] == [(r['elem'], r['start']) for r in p['runs']]
    assert [r['len'] for r in off['runs']] == [3, 1, 1]


def test_ratio_and_rung_budget_overrides(plan_dump):
    """ratio 1.2: ln 1.9 / ln 1.2 = 3.52, four steps; seven iterations per rung, 21 for the first of a head ladder"""
    env = dict(ratio=1.2, rung_iters=7)
    _, x = between(1.9, 3, plan_dump, env=env, ratio=1.2, rung_iters=7)
    assert math.ceil(x) == 4
    x = math.log(100) / math.log(1.2)
    assert away_from_an_integer(x) and math.ceil(x) == 26
    p = plan(plan_dump, case(np.array([0.5, 0.45]), open_at=[0], n_iter={0: 0}, n_evals={0: 0}, env=env))
    assert_entries(p, head_ladder(0.5, 26, rung_iters=7) + [(0.5, 0, 100)])


def test_overrides_arrive_clamped(plan_dump):
    """a ratio below 1.05 is 1.05 -- ln 1.9 / ln 1.05 = 13.16: 14 steps --, a rung budget below 1 is 1"""
    _, x = between(1.9, 13, plan_dump, env=dict(ratio=1.0, rung_iters=0), ratio=1.05, rung_iters=1)
    assert math.ceil(x) == 14


# ---- every plan

def expected_plan(c):
    """the rules of plan_finish, written down again"""
    n_chain, n_alpha = c['alpha'].shape
    env = c['env']
    ratio, rung_iters, ladder = max(1.05, env.get('ratio', RATIO)), max(1, int(env.get('rung_iters', RUNG_ITERS))), not env.get('no_ladder', 0)
    is_open = open_of(c)
    runs, ent = [], []

    def rungs(a_from, a_to, first):
        m = min(max(math.ceil(math.log(max(a_from / a_to, a_to / a_from)) / math.log(ratio) - 1e-9), 2), RUNGS_MAX + 1)
        q = (a_to / a_from) ** (1.0 / m)
        return [(a_from * q ** s, -1, 3 * rung_iters if s == 0 else rung_iters) for s in range(first, m)]

    for s in range(n_chain):
        a, i = c['alpha'][s], 0
        while i < n_alpha:
            if not is_open[s * n_alpha + i]:
                i += 1
                continue
            entry0, head = len(ent), s * n_alpha + i
            from_v0 = i == 0 and c['nit'][head] == 0 and c['nev'][head] == 0
            start = (True, s) if from_v0 else (False, head - 1 if i > 0 else head)
            quarter = 0.25 * c['rows'][s]
            if ladder and from_v0 and n_alpha > 1 and max(a[1] / a[0], a[0] / a[1]) <= COARSE and a[0] * ratio * ratio < quarter:
                ent += rungs(quarter, a[0], 0)
            while i < n_alpha and is_open[s * n_alpha + i]:
                if ladder and i > 0 and max(a[i - 1] / a[i], a[i] / a[i - 1]) > COARSE:
                    ent += rungs(a[i - 1], a[i], 1)
                ent.append((a[i], s * n_alpha + i, max(1, c['maxiter'] - c['nit'][s * n_alpha + i])))
                i += 1
            runs.append(dict(elem=c['chain_elem'][s], entry0=entry0, len=len(ent) - entry0, start=start))
    return runs, ent


def near_a_boundary(c):
    """a step whose count of rungs hangs on the last bits of a logarithm, or on those of the comparison with the threshold"""
    ratio = max(1.05, c['env'].get('ratio', RATIO))
    for s, a in enumerate(c['alpha']):
        steps = [max(x / y, y / x) for x, y in zip(a, a[1:])] + [0.25 * c['rows'][s] / a[0]]
        for r in steps:
            if r > 1 and not away_from_an_integer(math.log(r) / math.log(ratio)):
                return True
            if abs(r - COARSE) < 1e-9:
                return True
        if abs(a[0] * ratio * ratio - 0.25 * c['rows'][s]) < 1e-9:
            return True
    return False


def random_case(rng):
    n_chain, n_alpha = int(rng.integers(1, 6)), int(rng.integers(1, 13))
    maxiter = int(rng.choice([40, 100]))
    alpha = np.empty((n_chain, n_alpha))
    for s in range(n_chain):
        fine = rng.random(n_alpha) < 0.5
        step = np.where(fine, np.exp(rng.uniform(math.log(1.1), math.log(1.6), n_alpha)), np.exp(rng.uniform(math.log(1.6), math.log(1e3), n_alpha)))
        if rng.random() < 0.5:
            alpha[s] = math.exp(rng.uniform(math.log(0.01), math.log(1.0))) * np.cumprod(step)          # ascending
        else:
            alpha[s] = math.exp(rng.uniform(math.log(0.1), math.log(1e3))) / np.cumprod(step)
    P = n_chain * n_alpha
    conv = (rng.random(P) < rng.choice([0.2, 0.6, 0.9])).astype(int)
    nit = np.where(conv == 1, rng.integers(3, 30, P), rng.choice([0, 0, MC_GAVE_UP, maxiter - 1, maxiter, maxiter + 3], P))
    nev = np.where(nit == 0, rng.choice([0, 0, 0, 4], P), nit + rng.integers(0, 9, P))
    env = {}
    if rng.random() < 0.5:
        env['ratio'] = float(rng.choice([1.1, 1.5, 1.0]))
    if rng.random() < 0.3:
        env['rung_iters'] = int(rng.choice([1, 4, 25]))
    if rng.random() < 0.15:
        env['no_ladder'] = 1
    return dict(alpha=alpha, conv=conv, nit=nit, nev=nev, rows=[int(x) for x in rng.choice([8, 40, 200, 1000], n_chain)],
                chain_elem=[int(x) for x in rng.integers(0, 9, n_chain)], maxiter=maxiter, env=env)


def test_invariants_and_rules_on_random_inputs(plan_dump):
    rng = np.random.default_rng(20240611)
    n, n_rungs, n_head, n_capped, n_empty = 0, 0, 0, 0, 0
    while n < 300:
        c = random_case(rng)
        if near_a_boundary(c):
            continue
        n += 1
        p = plan(plan_dump, c)                  # (the invariants)
        runs, ent = expected_plan(c)
        assert p['runs'] == runs
        assert_entries(p, ent)
        n_rungs += p['n_rungs'] > 0
        n_empty += p['n_open'] == 0
        n_head += any(r['start'][0] and p['out'][r['entry0']] < 0 for r in p['runs'])
        n_capped += any(len(rungs) >= RUNGS_MAX for _, _, rungs in steps_of(c, p))
    # (the draw reaches what it is there for)
    assert n_rungs > 100 and n_head > 5 and n_capped > 5 and n_empty > 5


def test_the_plan_is_deterministic(plan_dump):
    c = random_case(np.random.default_rng(7))
    t = text_of(c)
    assert run_plan_dump(plan_dump, t, 'finish') == run_plan_dump(plan_dump, t, 'finish')
