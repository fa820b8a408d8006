"""The choosers of the kernel build (mxe::KernelBuild: lockstep_build, one_chain_build, lv_build, first_waves, build_name in
maxent_amd/csrc/mxe_plan.h, over the LDS formulas of mxe_shapes.h) on the host: `plan_dump build`, the stand-alone program of
tools/plan_dump.cpp (built with the address and undefined-behaviour sanitizers where the compiler links them).  Three checks:
cases derived by hand from the carve comments of the kernels, a sweep against a second statement of the rules below, and --
for every build a chooser returns -- that the list the library instantiates its kernels from has it.  All integers, compared
exactly."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from plan_dump_build import plan_dump_binary, run_plan_dump

OK, ERR_LIMIT = 0, -5
ONE_CHAIN, LOCKSTEP, LV = 0, 1, 2
LDS_CU = 160 * 1024
LDS_MC1, LDS_MC2 = LDS_CU - 6144, LDS_CU // 2 - 2048
FIELDS = ('rc', 'kind', 'NA', 'WGPC', 'NWV', 'lead', 'gst', 'NW', 'NAB', 'f32', 'lds', 'listed')


@pytest.fixture(scope='session')
def plan_dump(tmp_path_factory):
    return plan_dump_binary(tmp_path_factory)


def ask(binary, queries):
    """queries: tuples ('lockstep', NA, WGPC, lead, gst, n_omega_pad, waves_per_chain) and the like; one dict per answer"""
    out = run_plan_dump(binary, '\n'.join(' '.join(str(int(x)) if not isinstance(x, str) else x for x in q) for q in queries) + '\n', 'build')
    lines = out.split('\n')[:-1]
    assert len(lines) == len(queries)
    res = []
    for q, l in zip(queries, lines):
        if q[0] == 'first_waves':
            res.append(int(l))
        else:
            nums, name = l.split(' | ')
            res.append(dict(zip(FIELDS, map(int, nums.split())), name=name))
    return res


# ---- the second statement of the rules
def mc_lds(NA, nwp, wgpc, nwv=4, gst=False):
    """chain_kernel_mc (the carve at the top of the kernel), in doubles: eight vectors of four slots x 64, c and 1 / c, the step
    (64 x 4), the partial h of the waves (two buffers at two workgroups per CU), 32 sums per wave, two solve scales of four
    slots; u and H [n_omega_pad][4] (two workgroups per CU: u in registers); four slots x the tile pairs of the active block
    x 256.  Then sw [n_omega_pad][4] as floats.  Device-memory state: none of the three mesh arrays"""
    tiles = NA // 16
    pairs = tiles * (tiles + 1) // 2
    mesh = 0 if gst else nwp
    doubles = 8 * 256 + 2 * 64 + 256 + (2 if wgpc == 2 else nwv) * 256 + nwv * 32 + 2 * 256 + (1 if wgpc == 2 else 2) * mesh * 4 + 4 * pairs * 256
    return doubles * 8 + mesh * 4 * 4


def one_lds(NP, nwp, NW, f32, gst=False):
    """chain_kernel: the Newton matrix NP x (NP + 1), 13 (NP = 64) or 11 vectors of NP, NP + 8 doubles per wave and -- binary64 only --
    the Gram staging of each wave, 2 x 4 rows of NP / 4 blocks of 6 doubles: all binary64.  In the stream type: five mesh
    arrays (device-memory state: none) and one vector of NP"""
    fixed = NP * (NP + 1) + (13 if NP == 64 else 11) * NP + NW * (NP + 8)
    stage = 0 if f32 else NW * 2 * 4 * (NP // 4) * 6
    return (fixed + stage) * 8 + ((0 if gst else 5 * nwp) + NP) * (4 if f32 else 8)


def lv_lds(n_s, nwp):
    """chain_kernel_lv: max(32, n_s rounded up to eight) rows of V^T of n_omega_pad + 4 floats; 4 x 4 + 2 + 4 + 1 vectors of 64
    doubles; three of 4 x 64 floats; H or sw of the four slots, then the larger of a second such array and the solve's
    4 x 4 x 64 doubles; four slots x three tile pairs x 256 floats"""
    rows, s32 = max(32, (n_s + 7) // 8 * 8), nwp + 4
    stage, solve = 4 * s32 * 4, 4 * 4 * 64 * 8
    return rows * s32 * 4 + (16 + 2 + 4 + 1) * 64 * 8 + 3 * 4 * 64 * 4 + stage + max(stage, solve) + 4 * 3 * 256 * 4


def lockstep_model(NA, wgpc, lead, gst, nwp, wpc):
    nwv = 8 if (NA == 32 and wgpc == 1 and nwp % 256 == 0 and wpc != 4 and mc_lds(NA, nwp, 1, 8, gst) <= LDS_MC1) else 4
    lds = mc_lds(NA, nwp, wgpc, nwv, gst)
    name = 'mxe::chain_kernel_mc<%d, %d%s%s%s>' % (NA, wgpc, ', lead' if lead else '', ', 8 waves' if nwv == 8 else '', ', device-memory state' if gst else '')
    return dict(rc=OK if lds <= LDS_MC1 else ERR_LIMIT, kind=LOCKSTEP, NA=NA, WGPC=wgpc, NWV=nwv, lead=int(lead), gst=int(gst), lds=lds, name=name)


def one_chain_model(NP, nwp, NW, nw_min, f32):
    if f32 and NP != 64:
        return dict(rc=ERR_LIMIT)
    while one_lds(NP, nwp, NW, f32) > LDS_CU and NW > nw_min:
        NW //= 2
    gst = one_lds(NP, nwp, NW, f32) > LDS_CU
    if gst:
        NW = 4 if NP == 64 else 1
    lds = one_lds(NP, nwp, NW, f32, gst)
    name = 'mxe::chain_kernel<%d, %d, %s%s>' % (NW, NP // 32, 'float' if f32 else 'double', ', device-memory state' if gst else '')
    return dict(rc=OK if lds <= LDS_CU else ERR_LIMIT, kind=ONE_CHAIN, NW=NW, NAB=NP // 32, f32=int(f32), gst=int(gst), lds=lds, name=name)


def agrees(got, want):
    return all(got[k] == v for k, v in want.items())


# ---- hand-derived cases
def test_lockstep_lds_at_the_baseline_mesh(plan_dump):
    """n_omega_pad = 512.  <32, 2>, four waves: (2048 + 128 + 256 + 512 + 128 + 512 + 2048 + 3072) x 8 + 8192 = 77 824 <= LDS_MC2;
    <32, 1>: (2048 + 128 + 256 + 1024 + 128 + 512 + 4096 + 3072) x 8 + 8192 = 98 304; eight waves: h 2048, sums 256: 107 520"""
    assert (LDS_MC1, LDS_MC2) == (157696, 79872)
    a, b, c = ask(plan_dump, [('lockstep', 32, 2, 0, 0, 512, 0), ('lockstep', 32, 1, 0, 0, 512, 4), ('lockstep', 32, 1, 0, 0, 512, 0)])
    assert (a['rc'], a['NWV'], a['lds']) == (OK, 4, 77824) and a['lds'] <= LDS_MC2
    assert (b['rc'], b['NWV'], b['lds']) == (OK, 4, 98304)
    assert (c['rc'], c['NWV'], c['lds']) == (OK, 8, 107520)
    assert mc_lds(32, 512, 2) == 77824 and mc_lds(32, 512, 1) == 98304 and mc_lds(32, 512, 1, 8) == 107520
    # what tests/test_launch_plan_host.py carried as literals: the 64-row build and chain_kernel_lv with its static arrays at n_s = 56
    (d, e) = ask(plan_dump, [('lockstep', 64, 1, 0, 0, 512, 0), ('lv', 56, 512)])
    assert (d['rc'], d['NWV'], d['lds']) == (OK, 4, 155648) and e['lds'] + 2304 == 161536 <= LDS_CU


def test_waves_of_a_lockstep_build(plan_dump):
    """eight waves need n_omega_pad in units of 256 and waves_per_chain != 4; <32, 1> is 57 344 + 80 n_omega_pad bytes at four
    waves and 66 560 + 80 n_omega_pad at eight, against 157 696: up to 1254 and 1139; with device-memory state the mesh drops
    out and eight waves fit whatever the mesh; <64, 1> and <32, 2> always have four"""
    q = [('lockstep', 32, 1, 1, 0, nwp, wpc) for nwp in (256, 384, 512, 1024, 1152) for wpc in (0, 1, 2, 4, 8)]
    for (_, _, _, _, _, nwp, wpc), r in zip(q, ask(plan_dump, q)):
        assert r['rc'] == OK and r['NWV'] == (8 if nwp % 256 == 0 and wpc != 4 else 4), (nwp, wpc, r)
    assert (157696 - 57344) // 80 == 1254 and (157696 - 66560) // 80 == 1139
    assert mc_lds(32, 1254, 1) <= LDS_MC1 < mc_lds(32, 1255, 1) and mc_lds(32, 1139, 1, 8) <= LDS_MC1 < mc_lds(32, 1140, 1, 8)
    fits4, over4, fits8, over8 = ask(plan_dump, [('lockstep', 32, 1, 1, 0, 1254, 0), ('lockstep', 32, 1, 1, 0, 1255, 0),
                                                 ('lockstep', 32, 1, 1, 0, 1024, 0), ('lockstep', 32, 1, 1, 0, 1280, 0)])
    assert (fits4['rc'], fits4['NWV']) == (OK, 4) and (over4['rc'], over4['NWV']) == (ERR_LIMIT, 4)
    assert (fits8['rc'], fits8['NWV']) == (OK, 8) and (over8['rc'], over8['NWV']) == (ERR_LIMIT, 4)       # (1280 % 256 == 0, but eight waves no longer fit)
    g8, g4, g4b = ask(plan_dump, [('lockstep', 32, 1, 1, 1, 1280, 0), ('lockstep', 32, 1, 1, 1, 1280, 4), ('lockstep', 32, 1, 1, 1, 1600, 0)])
    assert (g8['rc'], g8['NWV'], g8['lds']) == (OK, 8, 66560) and (g4['rc'], g4['NWV'], g4['lds']) == (OK, 4, 57344) and g4b['NWV'] == 4
    assert g8['name'] == 'mxe::chain_kernel_mc<32, 1, lead, 8 waves, device-memory state>'
    for r in ask(plan_dump, [('lockstep', NA, w, lead, 0, 256, wpc) for NA, w in ((64, 1), (32, 2)) for lead in (0, 1) for wpc in (0, 8)]):
        assert r['rc'] == OK and r['NWV'] == 4 and r['listed'] == 1


def test_one_chain_layout(plan_dump):
    """NP = 64, binary64: 40 448 + 6 720 NW + 40 n_omega_pad bytes against 163 840: four waves up to 2412, two up to 2748, one up
    to 2916.  The launch halves 4 -> 2 -> 1; the finishing pass (nw_min = 4) never did and moves its state to device memory
    instead -- inside 2413-2748 the two differ.  Device-memory state: four waves at NP = 64, one at NP = 128 (144 384 +
    13 376 NW: only one wave fits beside the 128 x 128 matrix, and only up to n_omega_pad = 152)"""
    assert [(163840 - 40448 - 6720 * nw) // 40 for nw in (4, 2, 1)] == [2412, 2748, 2916]
    for nwp, launch, finish in ((2412, (4, 0), (4, 0)), (2413, (2, 0), (4, 1)), (2748, (2, 0), (4, 1)), (2749, (1, 0), (4, 1)),
                                (2916, (1, 0), (4, 1)), (2917, (4, 1), (4, 1))):
        l, f = ask(plan_dump, [('one_chain', 64, nwp, 4, 1, 0), ('one_chain', 64, nwp, 4, 4, 0)])
        assert (l['rc'], l['NW'], l['gst']) == (OK,) + launch and (f['rc'], f['NW'], f['gst']) == (OK,) + finish, nwp
        assert l['listed'] == f['listed'] == 1 and l['NAB'] == 2
    assert (163840 - 144384 - 13376) // 40 == 152 and 144384 + 2 * 13376 > 163840
    a, b, c = ask(plan_dump, [('one_chain', 128, 128, 4, 1, 0), ('one_chain', 128, 192, 4, 1, 0), ('one_chain', 128, 192, 4, 4, 0)])
    assert (a['rc'], a['NW'], a['NAB'], a['gst'], a['name']) == (OK, 1, 4, 0, 'mxe::chain_kernel<1, 4, double>')
    for r in (b, c):
        assert (r['rc'], r['NW'], r['gst'], r['lds'], r['name']) == (OK, 1, 1, 157760, 'mxe::chain_kernel<1, 4, double, device-memory state>')
    # with its state in device memory a chain fits whatever the mesh (NP = 64: 67 328 bytes, NP = 128: 157 760); what does not
    # fit anything is binary32 at NP = 128 -- binary32 is built with the 64-row matrix only (NAB = 2): MXE_ERR_LIMIT
    big, f32_128, f32_64, f32_g = ask(plan_dump, [('one_chain', 64, 1 << 20, 4, 1, 0), ('one_chain', 128, 128, 1, 1, 1),
                                                  ('one_chain', 64, 512, 2, 1, 1), ('one_chain', 64, 8192, 1, 1, 1)])
    assert (big['rc'], big['NW'], big['gst'], big['lds']) == (OK, 4, 1, 67328)
    assert f32_128['rc'] == ERR_LIMIT
    assert (f32_64['rc'], f32_64['NAB'], f32_64['name']) == (OK, 2, 'mxe::chain_kernel<2, 2, float>')
    assert (f32_g['rc'], f32_g['name']) == (OK, 'mxe::chain_kernel<4, 2, float, device-memory state>')


def test_first_waves(plan_dump):
    """the caller's waves per chain, at most four (eight are not built); else few chains -> more waves"""
    q = [('first_waves', w, n) for w in (0, 1, 2, 4, 8) for n in (1, 1023, 1024, 2047, 2048, 100000)]
    for (_, w, n), r in zip(q, ask(plan_dump, q)):
        assert r == (min(w, 4) if w else 1 if n >= 2048 else 2 if n >= 1024 else 4)


def test_the_names_the_gpu_tests_assert(plan_dump):
    """every kernel string tests/test_gpu_*.py compare with or take a prefix of, and the examples of DESIGN.md"""
    r = ask(plan_dump, [('lv', 56, 512), ('lockstep', 32, 2, 0, 0, 512, 0), ('one_chain', 128, 3136, 4, 1, 0),
                        ('two_pass', 56, 512, 1), ('two_pass', 56, 512, 2), ('two_pass', 56, 448, 1),
                        ('lockstep', 32, 1, 1, 0, 512, 0), ('lockstep', 64, 1, 0, 0, 512, 0), ('lockstep', 64, 1, 1, 0, 512, 0),
                        ('lockstep', 32, 2, 1, 0, 512, 0), ('lockstep', 32, 1, 0, 0, 512, 4), ('one_chain', 64, 512, 4, 1, 1),
                        ('one_chain', 64, 512, 4, 1, 0), ('lockstep', 32, 1, 1, 1, 1536, 0)])
    assert [x['name'] for x in r] == [
        'mxe::chain_kernel_lv', 'mxe::chain_kernel_mc<32, 2>', 'mxe::chain_kernel<1, 4, double, device-memory state>',
        'mxe::chain_kernel_lv + mxe::chain_kernel_mc<32, 1, 8 waves> per alpha', 'mxe::chain_kernel_lv + mxe::chain_kernel_mc<32, 2> per alpha',
        'mxe::chain_kernel_lv + mxe::chain_kernel_mc<32, 1> per alpha',
        'mxe::chain_kernel_mc<32, 1, lead, 8 waves>', 'mxe::chain_kernel_mc<64, 1>', 'mxe::chain_kernel_mc<64, 1, lead>',
        'mxe::chain_kernel_mc<32, 2, lead>', 'mxe::chain_kernel_mc<32, 1>', 'mxe::chain_kernel<4, 2, float>',
        'mxe::chain_kernel<4, 2, double>', 'mxe::chain_kernel_mc<32, 1, lead, 8 waves, device-memory state>']
    assert all(x['rc'] == OK and x['listed'] == 1 for x in r)
    assert (r[0]['kind'], r[0]['NWV'], r[0]['lds']) == (LV, 8, lv_lds(56, 512))


def test_a_build_that_is_not_listed_has_no_kernel(plan_dump):
    """the list holds what is instantiated: device-memory state without led pieces, at two workgroups per CU or with the 64-row
    block, and an active block of 48, are builds the chooser can be asked for and the library has no kernel of"""
    for r in ask(plan_dump, [('lockstep', 32, 1, 0, 1, 1536, 0), ('lockstep', 32, 2, 1, 1, 512, 0), ('lockstep', 64, 1, 1, 1, 512, 0), ('lockstep', 48, 1, 0, 0, 512, 0)]):
        assert r['rc'] == OK and r['listed'] == 0, r


# ---- the sweep
MESHES = range(64, 8192 + 1, 64)


def test_sweep_against_the_second_statement(plan_dump):
    """every mesh from 64 to 8192 in steps of 64; every (NA, WGPC, lead, device-memory state) choose_layout can emit -- two
    workgroups per CU only up to n_omega_pad = 512, device-memory state only as <32, 1, lead> --, every waves_per_chain; the
    one-chain build for both NP, every wanted wave count, launch and finishing pass, both precisions; the lv rows.  Every
    build a chooser returns with MXE_OK is one the library has a kernel for"""
    q = []
    for nwp in MESHES:
        emit = [(32, 1, l, 0) for l in (0, 1)] + [(64, 1, l, 0) for l in (0, 1)] + [(32, 1, 1, 1)] + ([(32, 2, l, 0) for l in (0, 1)] if nwp <= 512 else [])
        q += [('lockstep',) + e + (nwp, wpc) for e in emit for wpc in (0, 1, 2, 4, 8)]
        q += [('one_chain', NP, nwp, NW, nw_min, f32) for NP in (64, 128) for NW in (1, 2, 4) for nw_min in (1, 4) for f32 in (0, 1)]
        q += [('lv', n_s, nwp) for n_s in (16, 33, 56, 64)]
    seen = set()
    for query, got in zip(q, ask(plan_dump, q)):
        if query[0] == 'lockstep':
            want = lockstep_model(*query[1:])
        elif query[0] == 'one_chain':
            want = one_chain_model(*query[1:])
        else:
            want = dict(rc=OK, kind=LV, NA=32, WGPC=1, NWV=8, lead=1, gst=0, lds=lv_lds(*query[1:]), name='mxe::chain_kernel_lv')
        assert agrees(got, want), (query, got, want)
        if got['rc'] == OK:
            assert got['listed'] == 1, (query, got)
            seen.add(got['name'])
    # ... and 21 of the 23 kernels are chosen somewhere in the sweep.  The other two are listed and instantiated but no mesh selects
    # them: beside the 128 x 128 Newton matrix two or four waves of the binary64 one-chain kernel need 171 136 / 197 888 bytes
    # before the first mesh array (144 384 + 13 376 NW), more than the 163 840 of a CU
    assert len(seen) == 21 and not seen & {'mxe::chain_kernel<2, 4, double>', 'mxe::chain_kernel<4, 4, double>'}, sorted(seen)
    assert (one_lds(128, 0, 2, False), one_lds(128, 0, 4, False)) == (171136, 197888) and 171136 > LDS_CU
