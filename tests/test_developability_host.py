"""CPU-only checks of the developability analysis (abx_developability_scores, abx_amd.developability): C layout of the descriptor, argument
checks without a GPU, the reference areas and the fixed-point weights, the float64 / int64 host twin against an independent float
formulation and against recorded numbers of the two shipped complexes, hand-made sequences for the motif and charge rules, the edge
cases of the radius, and the wiring of the design driver."""
import ctypes

import numpy as np
import pytest
import torch

import host_cases as HC
import relax_cases as RC

A, R, N, D, C, Q, E, G, H, I, L_, K, M, F, P, S, T, W, Y, V = range(20)
# the issue's table: side-chain area of the isolated residue at P = 128, probe 1.4 A, in square Angstrom
REF = [62.3, 192.3, 115.9, 116.2, 99.5, 147.0, 144.4, 0.0, 159.1, 138.7, 136.8, 163.8, 152.8, 169.8, 116.0, 79.4, 106.3, 211.4, 186.0, 118.9]
TWO30 = float(1 << 30)


@pytest.fixture(scope='module')
def lib():
    return HC.load_lib()


def col(name):
    from abx_amd import developability as dv
    return dv.DEVELOPABILITY_COLUMNS.index(name)


def test_developability_args_match_c_layout():
    from abx_amd import _lib, developability as dv
    c_layout = HC.assert_c_layout({'AbxDevelopabilityArgs': _lib.AbxDevelopabilityArgs}, ['ABX_DEV_COLS'])
    assert c_layout['ABX_DEV_COLS'] == _lib.DEV_COLS == len(dv.DEVELOPABILITY_COLUMNS) == 21
    assert [dv.DEVELOPABILITY_COLUMNS.index(c) for c in dv.DELTA_COLUMNS] == [0, 1, 2, 3, 6, 7, 17, 18]
    assert dv.COUNT_COLUMNS == dv.DEVELOPABILITY_COLUMNS[4:] and len(dv.ROW_COLUMNS) == 4
    assert 'abx_developability_scores' in _lib.EXPORTED and 'abx_developability_scores_workspace_bytes' in _lib.EXPORTED


def test_argument_checks_without_gpu(lib):
    """Every malformed descriptor comes back negative before any launch, with the entry's name in the error string."""
    from abx_amd._lib import AbxDevelopabilityArgs
    PTR = 0x1000                                    # any non-null "device pointer": nothing is dereferenced

    def good():
        a = AbxDevelopabilityArgs()
        a.pred_atom14 = a.pred_seq = a.gt_atom14 = a.gt_exists = a.gt_seq = a.radius = a.chain_id = a.cdr_def = a.q = a.a = a.ref = a.points = a.out = PTR
        a.B, a.L, a.Lab, a.Lpred, a.P = 4, 40, 30, 30, 128
        a.pred_sb, a.pred_seq_sb, a.out_stride = 30 * 42, 30, 21
        a.radius2, a.exposed, a.q_max = 100.0, 0.075, 4123229
        return a

    def bad(a, ws=PTR):
        rc = lib.abx_developability_scores(ctypes.byref(a) if a is not None else None, ws, None)
        msg = lib.abx_last_error_string()
        assert rc < 0 and b'abx_developability_scores' in msg, (rc, msg)
        return msg

    bad(None)
    bad(AbxDevelopabilityArgs())
    bad(good(), ws=None)
    for field in ('pred_atom14', 'pred_seq', 'gt_atom14', 'gt_exists', 'gt_seq', 'radius', 'chain_id', 'cdr_def', 'q', 'a', 'ref', 'points', 'out'):
        a = good()
        setattr(a, field, None)
        bad(a)
    nan = float('nan')
    for field, v in (('B', 0), ('B', 65536), ('L', 0), ('Lab', 41), ('Lab', 0), ('Lpred', 29), ('out_stride', 20), ('P', 0), ('P', 1025),
                     ('radius2', 0.0), ('radius2', -1.0), ('radius2', nan), ('exposed', -0.1), ('exposed', 1.1), ('exposed', nan),
                     ('j_chunk', -1), ('j_chunk', 2049), ('q_max', -1)):
        a = good()
        setattr(a, field, v)
        bad(a)
    a = good()                                      # more rows than the row tables of the last kernel hold
    a.L, a.Lab, a.Lpred = 3000, 2049, 2049
    assert b'Lab <= 2048' in bad(a)
    a = good()                                      # weights with which the sums could leave int64
    a.q_max = 1 << 44
    assert b'int64' in bad(a)
    assert lib.abx_developability_scores_workspace_bytes(100, 352) == 100 * (48 * 14 * 352 + 16)
    assert lib.abx_developability_scores_workspace_bytes(0, 352) == 0


def test_reference_areas_and_weights():
    """The isolated-residue side-chain areas match the recorded table to 0.05; q is 0 on the backbone, for Gly and for X, has the sign of
    the hydrophobicity elsewhere, and P q_max stays below 0.5 x 2^30 from the default P to 1024 (the header's bound)."""
    from abx_amd import developability as dv, residue_constants as rc
    ref = dv.reference_areas(128, 1.4)
    assert ref.shape == (21,) and ref[20] == 0.0 and ref[G] == 0.0
    print('reference areas', np.round(ref, 2).tolist())
    assert np.abs(ref[:20] - np.array(REF)).max() <= 0.05
    h = dv.hydrophobicity()
    assert h[G] == 0.0 and h[20] == 0.0 and abs(h[F] - 0.499) < 1e-12 and abs(h[R] + 0.501) < 1e-12 and list(rc.restypes) == list('ARNDCQEGHILKMFPSTWYV')
    typed = np.asarray(rc.restype_atom14_mask) != 0
    assert typed.shape == (21, 14) and not typed[20].any()
    for Pn in (16, 128, 1024):
        q, a, r = dv.weight_table(Pn, 1.4)
        assert q.dtype == np.int64 and q.shape == (21, 14) and a.shape == (21, 14) and r.shape == (21,)
        assert not q[:, :4].any() and not q[G].any() and not q[20].any()
        side = typed.copy()
        side[:, :4] = False
        side[G] = False
        assert np.array_equal(np.sign(q), np.where(side, np.sign(h)[:, None], 0).astype(np.int64))
        assert np.array_equal(a > 0, typed)
    for Pn in (128, 256, 512, 1024):                # the header's worst case: |w_j| <= P q_max < 0.5 x 2^30
        assert Pn * int(np.abs(dv.weight_table(Pn, 1.4)[0]).max()) < (1 << 29)
    # the ideal geometry: bonded neighbours at bond length, chi = 180 degrees puts Lys NZ far from its C-alpha
    x = dv.ideal_residue(K)
    d = lambda i, j: float(np.linalg.norm(x[i] - x[j]))
    assert abs(d(0, 1) - 1.46) < 0.03 and abs(d(1, 4) - 1.53) < 0.03 and abs(d(7, 8) - 1.49) < 0.03 and d(1, 8) > 6.0


@pytest.fixture(scope='module')
def shipped():
    """Host rows of the two shipped complexes (ground truth, P = 128, region = CDR-H3, R = 10 A), computed once."""
    from abx_amd import developability as dv, interface
    out = {}
    for code in ('6ct7', '6qd7'):
        c = RC.load_complex(code, 'h3')
        pts = interface.interface_host(c['x'], c['mask'], c['aa'], c['Lab'], region=c['mov'], n_points=128)[1]
        row, rows, d = dv.developability_host(c['x'], c['mask'], c['aa'], c['Lab'], c['chain'], c['residx'], c['cdr'], region=c['mov'], points=pts,
                                              details=True)
        out[code] = dict(c=c, pts=pts, row=row, rows=rows, d=d)
    return out


@pytest.mark.parametrize('code', ['6ct7', '6qd7'])
def test_fixed_point_against_a_float_formulation(shipped, code):
    """SAP_i / 2^30 against a brute-force float64 sum of acc_alone a h / ref over the atoms within 10 A: the difference stays within
    the quantisation of q, 2^-31 per accessible point of the neighbours."""
    from abx_amd import developability as dv
    from abx_amd.interface import _radius_table
    s = shipped[code]
    c, d = s['c'], s['d']
    aa, Lab = c['aa'].numpy(), c['Lab']
    counted = c['mask'].numpy() & (_radius_table()[aa] > 0) & (np.arange(aa.shape[0]) < Lab)[:, None]
    assert np.array_equal(counted, d['counted'])
    rows_i, slots_i = np.nonzero(counted)
    xyz = c['x'].numpy().astype(np.float32).astype(np.float64)[rows_i, slots_i]
    alone = s['pts'][..., 0].astype(np.float64)[rows_i, slots_i]
    _, a, ref = dv.weight_table(128, 1.4)
    h = dv.hydrophobicity()
    side = (slots_i >= 4) & (ref[aa[rows_i]] > 0)
    wf = np.where(side, alone * a[aa[rows_i], slots_i] * h[aa[rows_i]] / np.where(ref[aa[rows_i]] > 0, ref[aa[rows_i]], 1.0), 0.0)
    near = (((xyz[:, None] - xyz[None]) ** 2).sum(-1) <= 100.0)
    want = near.astype(np.float64) @ wf
    bound = (near.astype(np.float64) @ np.where(side, alone, 0.0)) * 2.0 ** -31
    got = d['sap'][rows_i, slots_i].astype(np.float64) / TWO30
    diff = np.abs(got - want)
    print(code, 'largest difference', diff.max(), 'bound', bound.max(), 'atoms', rows_i.shape[0])
    assert bool((diff <= bound + 1e-12).all()) and 1e-9 < diff.max() < 1e-6
    assert np.abs(d['sap']).max() < 2e10 and np.abs(d['sap']).sum() < 1e13


RECORDED = {                                         # the twin's own values; the first five as a prototype of the definitions printed them
    '6ct7': dict(sap_pos=55.07294, sap_pos_region=2.85017, sap_max_res=0.69433, hottest=108, n_res_sap_pos=40, sap_pos_cdr=4.39684,
                 n_res_sap_pos_region=3, charge_heavy=-2, charge_light=-4, charge_product=8, n_his=2, n_glyc=0, n_deamid=1, n_isomer=4, n_frag=0,
                 n_met_ox=2, n_trp_ox=1, n_cys_free=0, n_liab=8, n_liab_region=0, n_liab_cdr=5, n_atoms=1663),
    '6qd7': dict(sap_pos=80.00797, sap_pos_region=8.69628, sap_max_res=0.79923, hottest=115, n_res_sap_pos=47, sap_pos_cdr=13.35952,
                 n_res_sap_pos_region=5, charge_heavy=3, charge_light=0, charge_product=0, n_his=1, n_glyc=0, n_deamid=2, n_isomer=1, n_frag=0,
                 n_met_ox=0, n_trp_ox=1, n_cys_free=0, n_liab=4, n_liab_region=0, n_liab_cdr=1, n_atoms=1722),
}


@pytest.mark.parametrize('code', ['6ct7', '6qd7'])
def test_shipped_complexes_give_the_recorded_rows(shipped, code):
    from abx_amd import developability as dv
    s = shipped[code]
    row, rows, c = s['row'], s['rows'], s['c']
    got = dict(zip(dv.DEVELOPABILITY_COLUMNS, row.tolist()))
    print(code, got)
    want = dict(RECORDED[code])
    hottest = want.pop('hottest')
    for k, v in want.items():
        assert (got[k] == v) if k in dv.COUNT_COLUMNS else (abs(got[k] - v) <= 5e-6), (k, got[k], v)
    assert int(rows[:, 0].argmax()) == hottest and int(c['aa'][hottest]) == V and rows[hottest, 0] == row[3]
    # the per-residue table against the row
    Lab = c['Lab']
    assert rows.shape == (c['aa'].shape[0], 4) and not rows[Lab:].any()
    assert sum(bin(int(m)).count('1') for m in rows[:, 2]) == row[17] and [int((rows[:, 2].astype(np.int64) >> k & 1).sum()) for k in range(7)] == row[10:17].tolist()
    heavy = (c['chain'] == c['chain'][0]).numpy()
    assert rows[heavy, 3].sum() == row[6] and rows[~heavy, 3].sum() == row[7] and row[8] == row[6] * row[7]
    assert 0.0 <= rows[:, 1].min() and rows[:, 1].max() < 1.3 and not rows[(c['aa'] == G).numpy(), 1].any()
    # the points are computed by interface_host when none are given
    again = dv.developability_host(c['x'], c['mask'], c['aa'], Lab, c['chain'], c['residx'], c['cdr'], region=c['mov'])[0]
    assert again.tolist() == row.tolist()


def hand_made(seq_edits, chain=None, residx='given', points_edit=None, x_edit=None, Lab=None):
    """6ct7's coordinates under a hand-made sequence: every antibody row Ala except seq_edits {row: type}, the atoms of the types, 64 of
    128 points accessible on every slot (every non-Gly residue is exposed) except points_edit {row: count}."""
    from abx_amd import developability as dv, residue_constants as rc
    c = RC.load_complex('6ct7', 'h3')
    Lab = c['Lab'] if Lab is None else Lab
    aa = c['aa'].numpy().copy()
    aa[:Lab] = A
    for r, t in seq_edits.items():
        aa[r] = t
    mask = np.asarray(rc.restype_atom14_mask)[aa] != 0
    pts = np.full(aa.shape + (14, 2), 64, np.int32)
    for r, n in (points_edit or {}).items():
        pts[r] = n
    x = c['x'].numpy().copy()
    for (r, sl), v in (x_edit or {}).items():
        x[r, sl] = v
    ch = c['chain'].numpy() if chain is None else chain
    ri = c['residx'].numpy() if isinstance(residx, str) else residx
    row, rows = dv.developability_host(x, mask, aa, Lab, ch, ri, c['cdr'], region=c['mov'], points=pts)
    return dict(zip(dv.DEVELOPABILITY_COLUMNS, row.tolist())), rows, c


def test_motifs_on_hand_made_sequences():
    c = RC.load_complex('6ct7', 'h3')
    chain, residx = c['chain'].numpy(), c['residx'].numpy()
    Lab = c['Lab']
    last_heavy = int(np.nonzero(chain[:Lab] == chain[0])[0][-1])
    assert 40 < last_heavy < Lab - 3 and (np.diff(residx[20:30]) == 1).all() and chain[20] == chain[29]
    liab = lambda g: [int(g[k]) for k in ('n_glyc', 'n_deamid', 'n_isomer', 'n_frag', 'n_met_ox', 'n_trp_ox', 'n_cys_free', 'n_liab')]
    g, rows, _ = hand_made({})
    assert liab(g) == [0] * 8 and not rows[:, 2].any()
    g, rows, _ = hand_made({20: N, 21: G, 22: S})                              # NGS: a sequon and a deamidation site, both owned by the N
    assert liab(g) == [1, 1, 0, 0, 0, 0, 0, 2] and rows[20, 2] == 3 and rows[:, 2].sum() == 3
    assert liab(hand_made({20: N, 21: P, 22: S})[0]) == [0] * 8               # NPS is no sequon (and NP no deamidation site)
    assert liab(hand_made({20: N, 21: A, 22: T})[0]) == [1, 0, 0, 0, 0, 0, 0, 1]
    assert liab(hand_made({20: N, 21: S, 22: A})[0]) == [0, 1, 0, 0, 0, 0, 0, 1]
    assert liab(hand_made({20: N, 21: G, 22: S}, points_edit={20: 0})[0]) == [0] * 8      # a buried N
    assert liab(hand_made({20: N, 21: G, 22: S}, points_edit={21: 0, 22: 0})[0]) == [1, 1, 0, 0, 0, 0, 0, 2]      # only the N's exposure counts
    # across the chain boundary, and across a gap of the residue numbers
    at = {last_heavy: N, last_heavy + 1: G, last_heavy + 2: S}
    assert liab(hand_made(at)[0]) == [0] * 8
    assert liab(hand_made(at, chain=np.zeros_like(chain), residx=None)[0]) == [1, 1, 0, 0, 0, 0, 0, 2]
    gap = residx.copy()
    gap[21:] += 1
    assert liab(hand_made({20: N, 21: G, 22: S}, residx=gap)[0]) == [0] * 8
    gap = residx.copy()
    gap[22:] += 1
    assert liab(hand_made({20: N, 21: G, 22: S}, residx=gap)[0]) == [0, 1, 0, 0, 0, 0, 0, 1]
    assert liab(hand_made({20: N, 21: G, 22: S}, residx=None)[0]) == [1, 1, 0, 0, 0, 0, 0, 2]       # without numbers the chain id links
    # D-G, D-S, D-P, Met, Trp; the region and CDR columns follow the first row
    g, rows, c = hand_made({20: D, 21: G, 24: D, 25: P, 27: D, 28: S, 30: M, 31: W})
    assert liab(g) == [0, 0, 2, 1, 1, 1, 0, 5] and rows[[20, 24, 27, 30, 31], 2].tolist() == [4, 8, 4, 16, 32]
    h3 = int(np.nonzero(c['mov'].numpy())[0][0])
    g, rows, c = hand_made({h3: M, 30: W})
    assert (g['n_liab'], g['n_liab_region'], g['n_liab_cdr']) == (2, 1, 1 + int(int(c['cdr'][30]) in RC.CDR_CODES))
    # Gly is never exposed, and an unexposed Met is no liability
    assert liab(hand_made({30: M}, points_edit={30: 0})[0]) == [0] * 8
    # the threshold itself: rel >= exposed x ref
    from abx_amd import developability as dv
    q, a, ref = dv.weight_table(128, 1.4)
    n_min = int(np.ceil(0.075 * ref[M] / a[M, 4:8].sum()))
    assert liab(hand_made({30: M}, points_edit={30: n_min})[0])[4] == 1 and liab(hand_made({30: M}, points_edit={30: n_min - 1})[0])[4] == 0


def test_free_cysteines_and_charges():
    c = RC.load_complex('6ct7', 'h3')
    sg = c['x'].numpy()[40, 4]
    near = {(40, 5): sg + np.array([1.0, 0.0, 0.0]), (60, 5): sg + np.array([3.05, 0.0, 0.0])}
    g, rows, _ = hand_made({40: C, 60: C}, x_edit=near)                        # two SG 2.05 A apart: a disulfide
    assert g['n_cys_free'] == 0 and g['n_liab'] == 0
    far = {(40, 5): sg + np.array([1.0, 0.0, 0.0]), (60, 5): sg + np.array([4.0, 0.0, 0.0])}
    g, rows, _ = hand_made({40: C, 60: C}, x_edit=far)                         # 3 A: two free cysteines
    assert g['n_cys_free'] == 2 and g['n_liab'] == 2 and rows[[40, 60], 2].tolist() == [64, 64]
    g, _, _ = hand_made({40: C, 60: C}, x_edit=far, points_edit={40: 0, 60: 0})      # no exposure condition
    assert g['n_cys_free'] == 2
    g, _, _ = hand_made({40: C, 60: C, 80: C}, x_edit={**near, (80, 5): sg + np.array([0.0, 9.0, 0.0])})
    assert g['n_cys_free'] == 1
    # charges per chain: heavy K K R D H -> +2, light E E D K -> -2
    chain, Lab = c['chain'].numpy(), c['Lab']
    first_light = int(np.nonzero(chain[:Lab] != chain[0])[0][0])
    edits = {3: K, 9: K, 50: R, 70: D, 71: H, first_light + 2: E, first_light + 9: E, first_light + 30: D, first_light + 31: K, first_light + 40: H}
    g, rows, _ = hand_made(edits)
    assert (g['charge_heavy'], g['charge_light'], g['charge_product'], g['n_his']) == (2, -2, -4, 2)
    assert rows[[3, 70, 71, first_light + 2], 3].tolist() == [1, -1, 0, -1]
    g, _, _ = hand_made(edits, chain=np.zeros_like(chain))                      # a single-chain antibody: no light chain
    assert (g['charge_heavy'], g['charge_light'], g['charge_product']) == (0, 0, 0)
    g, _, _ = hand_made(edits, Lab=first_light)                                 # the heavy chain alone
    assert (g['charge_heavy'], g['charge_light'], g['charge_product'], g['n_his']) == (2, 0, 0, 1)


def test_radius_and_weight_edge_cases(shipped):
    from abx_amd import developability as dv, residue_constants as rc
    s = shipped['6ct7']
    c = s['c']
    args = (c['x'], c['mask'], c['aa'], c['Lab'], c['chain'], c['residx'], c['cdr'])
    # a radius below every distance: only j = i remains
    row, _, d = dv.developability_host(*args, region=c['mov'], points=s['pts'], radius=1e-3, details=True)
    assert np.array_equal(d['sap'], d['w']) and d['w'].any() and row[0] == np.maximum(d['w'], 0).sum() / TWO30
    # a radius beyond every distance: every atom carries the sum of the structure
    row, rows, d = dv.developability_host(*args, region=c['mov'], points=s['pts'], radius=1e4, details=True)
    total = int(d['w'].sum())
    assert np.array_equal(d['sap'][d['counted']], np.full(int(row[20]), total)) and total != 0
    assert row[0] == max(total, 0) * row[20] / TWO30 and row[3] == total / TWO30
    assert np.array_equal(d['w'], s['d']['w'])
    # all-Gly tokens: no weighted atom, every sap column is 0
    aa = c['aa'].clone()
    aa[:c['Lab']] = G
    mask = torch.as_tensor(np.asarray(rc.restype_atom14_mask))[aa].bool()
    row, rows, d = dv.developability_host(c['x'], mask, aa, c['Lab'], c['chain'], c['residx'], c['cdr'], region=c['mov'], points=s['pts'], details=True)
    assert row[:6].tolist() == [0.0] * 6 and not d['w'].any() and row[20] == 4 * c['Lab'] and not rows[:, :3].any() and row[6:20].tolist() == [0.0] * 14


PARSER = None


def parser():
    global PARSER
    if PARSER is None:
        from abx_amd import design
        PARSER = design.build_parser()
    return PARSER


def test_driver_declares_an_extension():
    """ANALYSES keeps its order; --developability is walked after the first seven."""
    from abx_amd import analyses, developability as dv
    assert [an.flag for an in analyses.ANALYSES] == ['score', 'relax', 'interface', 'confidence', 'accuracy', 'polar', 'ensemble', 'developability', 'shape', 'patches', 'torsions', 'secondary']
    assert analyses.DEVELOPABILITY.kw == 'developability'
    a = parser().parse_args([])
    assert a.developability is False and a.developability_rows is False and (a.developability_radius, a.developability_exposed) == (10.0, 0.075)
    assert analyses.check_options(a, False) == []
    every = ['--' + an.flag for an in analyses.ANALYSES[:7]]
    a = parser().parse_args(['--developability'] + every)
    assert [an.flag for an in analyses.check_options(a, True)] == [an.flag for an in analyses.ANALYSES[:7]] + ['developability']
    a = parser().parse_args(['--developability', '--developability_rows', '--developability_radius', '8', '--developability_exposed', '0.1'])
    assert [an.flag for an in analyses.check_options(a, False)] == ['developability']
    ND = len(dv.DEVELOPABILITY_COLUMNS)
    shapes = lambda a: {f.name: (f.dtype, f.shape, f.rows) for f in analyses.fields_of(analyses.check_options(a, False), a)}
    assert shapes(a) == {'seq': (torch.int64, ('Lab',), True), 'pLDDT': (torch.float32, ('Lab',), False),
                         'developability': (torch.float64, (2 * ND,), True), 'developability_rows': (torch.float64, ('L', 4), False)}
    a = parser().parse_args(['--developability', '--relax'])
    assert shapes(a)['developability'] == (torch.float64, (3 * ND,), True) and 'developability_rows' not in shapes(a)


@pytest.mark.parametrize('argv, set_level, text', [
    (['--developability_rows'], False, '--developability_rows needs --developability'),
    (['--developability', '--developability_rows'], True,
     '--developability_rows needs the sample-sharded schedule (--shard_samples): a set-level run gathers one table only'),
    (['--developability', '--developability_radius', '0'], False, '--developability_radius must be > 0, --developability_exposed in [0, 1]'),
    (['--developability', '--developability_exposed', '1.5'], False, '--developability_radius must be > 0, --developability_exposed in [0, 1]'),
    (['--developability', '--interface_points', '0'], False, '--interface_points must be in 1..1024, --interface_probe >= 0'),
    (['--developability', '--interface_probe', '-1'], False, '--interface_points must be in 1..1024, --interface_probe >= 0'),
])
def test_option_checks_exit_by_name(argv, set_level, text):
    from abx_amd import analyses
    with pytest.raises(SystemExit) as e:
        analyses.check_options(parser().parse_args(argv), set_level)
    assert e.value.code == text


class Wild:
    """A scorer as analyses.collect sees one: a wild row per complex and the buffer of point counts."""

    def __init__(self, columns, seen):
        self.columns, self.seen = columns, seen

    def new_points(self, B):
        return torch.empty(B, 9, 14, 2, dtype=torch.int32)

    def wild(self, points=None):
        self.seen.append(points)
        return torch.full((1, len(self.columns)), 0.5, dtype=torch.float64)


@pytest.mark.parametrize('with_seven', [False, True])
def test_zero_row_block_matches_the_filled_block(with_seven):
    from abx_amd import accuracy, analyses, confidence, developability as dv, interface, metrics, polar, relax
    L, Lab, n = 9, 7, 2
    seven = [an.flag for an in analyses.ANALYSES[:7]] if with_seven else []
    flags = seven + ['developability', 'developability_rows'] + [an.extra for an in analyses.ANALYSES[:7] if an.extra and with_seven]
    a = parser().parse_args(['--' + f for f in flags])
    active = analyses.check_options(a, set_level=False)
    assert [an.flag for an in active] == seven + ['developability']
    g = torch.Generator().manual_seed(3)
    table = lambda cols: (torch.rand(n, len(cols), generator=g, dtype=torch.float64) * 50).round(decimals=3)
    rec = {'seq': torch.randint(0, 20, (n, Lab), generator=g), 'pLDDT': torch.full((n, Lab), 70.0), 'atom14_results': torch.randn(n, Lab, 14, 3, generator=g),
           'time': 0.01, 'scores': table(metrics.SCORE_COLUMNS), 'relax': table(relax.RELAX_COLUMNS), 'scores_relaxed': table(metrics.SCORE_COLUMNS),
           'confidence_wild': table(confidence.CONFIDENCE_COLUMNS), 'confidence_planes': (torch.rand(n, L, L, generator=g), None),
           'accuracy_rows': torch.rand(n, L, 4, generator=g, dtype=torch.float64), 'polar_rows': torch.zeros(n, L, 4, dtype=torch.int32),
           'developability_rows': torch.rand(n, L, 4, generator=g, dtype=torch.float64)}
    for mod in (interface, confidence, accuracy, polar, dv):
        kind = mod.__name__.rsplit('.', 1)[1]
        rec[kind], rec[kind + '_relaxed'] = table(getattr(mod, kind.upper() + '_COLUMNS')), table(getattr(mod, kind.upper() + '_COLUMNS'))
    seen = []
    columns = {'interface': interface.INTERFACE_COLUMNS, 'accuracy': accuracy.ACCURACY_COLUMNS, 'polar': polar.POLAR_COLUMNS,
               'developability': dv.DEVELOPABILITY_COLUMNS}
    scorers = {f: Wild(c, seen) for f, c in columns.items() if f in flags}
    filled = analyses.collect(active, a, [rec], scorers)
    zero = analyses.zero_rows(active, a, L, Lab, 'cpu')
    assert list(filled) == list(zero) == [f.name for f in analyses.fields_of(active, a)] and list(zero)[-2:] == ['developability', 'developability_rows']
    for k in filled:
        assert filled[k].dtype == zero[k].dtype and filled[k].shape[1:] == zero[k].shape[1:] and filled[k].shape[0] == n and zero[k].shape[0] == 0, k
    ND = len(dv.DEVELOPABILITY_COLUMNS)
    assert filled['developability'].shape == (n, (3 if with_seven else 2) * ND) and bool((filled['developability'][:, -ND:] == 0.5).all())
    assert torch.equal(filled['developability'][:, :ND], rec['developability']) and torch.equal(filled['developability_rows'], rec['developability_rows'])
    if with_seven:                  # one buffer of point counts serves the three wild rows; accuracy's takes none
        assert len(seen) == 4 and seen[0] is seen[2] and seen[0] is seen[3] and seen[0].shape == (1, 9, 14, 2) and seen[1] is None
    else:
        assert seen == [None]


def test_table_format(tmp_path):
    from abx_amd import design, developability as dv
    ND = len(dv.DEVELOPABILITY_COLUMNS)
    wild = [55.0729, 4.3968, 2.8502, 0.6943, 40, 3, -2, -4, 8, 2, 0, 1, 4, 0, 2, 1, 0, 8, 0, 5, 1663]
    d0 = [60.5, 5.0, 3.0, 0.75, 42, 4, -1, -4, 4, 2, 1, 1, 4, 0, 2, 1, 0, 9, 1, 6, 1670]
    assert dv.format_developability(wild) == ['55.073', '4.397', '2.850', '0.694', '40', '3', '-2', '-4', '8', '2', '0', '1', '4', '0', '2', '1', '0', '8',
                                              '0', '5', '1663']
    assert dv.format_delta(d0, wild) == ['+5.427', '+0.603', '+0.150', '+0.056', '+1', '+0', '+1', '+1']
    path = design._write_developability(str(tmp_path), '6ct7_H_L_S', wild, [(0, d0 + wild), (1, wild + wild)], False)
    lines = [ln.split('\t') for ln in open(path).read().splitlines()]
    assert path.endswith('6ct7_H_L_S_developability.tsv') and len(lines) == 4
    assert lines[0] == ['sample'] + list(dv.DEVELOPABILITY_COLUMNS) + ['delta_' + c for c in dv.DELTA_COLUMNS]
    assert lines[1] == ['wild'] + dv.format_developability(wild) + ['+0.000'] * 4 + ['+0'] * 4
    assert lines[2] == ['0'] + dv.format_developability(d0) + dv.format_delta(d0, wild) and lines[3][1 + ND:] == lines[1][1 + ND:]
    path = design._write_developability(str(tmp_path), 'x_H_L_A', wild, [(5, d0 + wild + wild)], True)
    lines = [ln.split('\t') for ln in open(path).read().splitlines()]
    assert lines[0][1 + ND + 8:] == [c + '_relaxed' for c in dv.DEVELOPABILITY_COLUMNS] and lines[1][1 + ND + 8:] == ['nan'] * ND
    assert lines[2] == ['5'] + dv.format_developability(d0) + dv.format_delta(d0, wild) + dv.format_developability(wild)


def test_sampler_signature_defaults_to_no_developability():
    import inspect
    from abx_amd import sampler
    assert inspect.signature(sampler.sample_fn).parameters['developability'].default is None
