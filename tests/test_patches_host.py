"""CPU-only checks of the patch analysis (abx_patch_scores, abx_amd.patches): C layout of the descriptor, argument checks without a GPU,
the hydrophobicity and charge tables, the float64 / int64 host twin against the numbers a prototype of the definition printed for the two
shipped complexes, hand-built structures of a few residues whose answer is written down, the antigen moved away, and the wiring of the
design driver."""
import ctypes

import numpy as np
import pytest
import torch

import host_cases as HC
import patches_cases as PC
import relax_cases as RC
import shape_cases as SC
from patches_cases import A, D, G, K, R, E, H, TWO30, X


@pytest.fixture(scope='module')
def lib():
    return HC.load_lib()


def col(name):
    from abx_amd import patches
    return patches.PATCHES_COLUMNS.index(name)


def test_patch_args_match_c_layout():
    from abx_amd import _lib, patches
    c_layout = HC.assert_c_layout({'AbxPatchArgs': _lib.AbxPatchArgs}, ['ABX_PATCH_COLS'])
    assert c_layout['ABX_PATCH_COLS'] == _lib.PATCH_COLS == len(patches.PATCHES_COLUMNS) == 18
    assert [patches.PATCHES_COLUMNS.index(c) for c in patches.DELTA_COLUMNS] == [0, 1, 2, 3, 4, 7, 8, 9, 10]
    assert patches.COUNT_COLUMNS == patches.PATCHES_COLUMNS[11:] and patches.ROW_COLUMNS == ('psh', 'charge_patch', 'cross_charge', 'flags')
    assert 'abx_patch_scores' in _lib.EXPORTED and 'abx_patch_scores_workspace_bytes' in _lib.EXPORTED


def test_argument_checks_without_gpu(lib):
    """Every malformed descriptor comes back negative before any launch, with the entry's name in the error string."""
    from abx_amd._lib import AbxPatchArgs
    PTR = 0x1000                                    # any non-null "device pointer": nothing is dereferenced
    operands = ('pred_atom14', 'pred_seq', 'gt_atom14', 'gt_exists', 'gt_seq', 'radius', 'points', 'chain_id', 'cdr_def', 'h', 'q10', 'table', 'a',
                'ref', 'out')

    def good():
        a = AbxPatchArgs()
        for f in operands:
            setattr(a, f, PTR)
        a.B, a.L, a.Lab, a.Lpred = 4, 40, 30, 30
        a.pred_sb, a.pred_seq_sb, a.out_stride = 30 * 42, 30, 18
        a.cutoff2, a.vicinity2, a.salt2, a.exposed, a.h_max, a.q_max, a.gly = 56.25, 16.0, 10.24, 0.075, 2.0, 10, 7
        return a

    def bad(a, ws=PTR):
        rc = lib.abx_patch_scores(ctypes.byref(a) if a is not None else None, ws, None)
        msg = lib.abx_last_error_string()
        assert rc < 0 and b'abx_patch_scores' in msg, (rc, msg)
        return msg

    bad(None)
    bad(AbxPatchArgs())
    bad(good(), ws=None)
    for field in operands:
        a = good()
        setattr(a, field, None)
        bad(a)
    nan = float('nan')
    for field, v in (('B', 0), ('B', 65536), ('L', 0), ('Lab', 41), ('Lab', 0), ('Lpred', 29), ('out_stride', 17), ('cutoff2', 0.0),
                     ('cutoff2', nan), ('vicinity2', -1.0), ('vicinity2', nan), ('salt2', 0.0), ('salt2', nan), ('exposed', -0.1),
                     ('exposed', 1.1), ('exposed', nan), ('gly', -1), ('gly', 21), ('h_max', -1.0), ('h_max', nan), ('q_max', -1)):
        a = good()
        setattr(a, field, v)
        bad(a)
    a = good()                                      # more rows than the row tables of the last kernel hold
    a.L, a.Lab, a.Lpred = 2049, 300, 300
    assert b'L <= 2048' in bad(a)
    a = good()                                      # tables with which the sums could leave int64
    a.h_max = 1e5
    assert b'int64' in bad(a)
    a = good()
    a.q_max = 1 << 20
    assert b'int64' in bad(a)
    tiles = (228 + 15) // 16
    assert lib.abx_patch_scores_workspace_bytes(100, 352, 228) == 100 * ((224 * 352 + 8 * 228 * 352 + 4 * 352 + tiles * 228 + 15) // 16 * 16)
    assert lib.abx_patch_scores_workspace_bytes(0, 352, 228) == 0 and lib.abx_patch_scores_workspace_bytes(1, 10, 11) == 0


def test_tables():
    """H = 1 + (KD + 4.5) / 9 lies in [1, 2] with Arg at 1, Ile at 2 and Gly at 1.4555...; X is 0; the charges in tenths."""
    from abx_amd import patches, residue_constants as rc
    h, q = patches.kyte_doolittle(), patches.charge_table()
    assert list(rc.restypes) == list('ARNDCQEGHILKMFPSTWYV') and patches.gly_type() == G
    assert h.dtype == np.float64 and h.shape == (21,) and q.dtype == np.int64 and q.shape == (21,)
    assert h[X] == 0.0 and h[R] == 1.0 and h[PC.I] == 2.0 and 1.0 <= h[:20].min() and h[:20].max() <= 2.0
    assert abs(h[G] - 1.4555555555555555) < 1e-15 and h[G] == 1.0 + (-0.4 + 4.5) / 9.0
    assert q.tolist() == [10 if t in (K, R) else -10 if t in (D, E) else 1 if t == H else 0 for t in range(21)]


@pytest.fixture(scope='module')
def shipped():
    """Host rows of the two shipped complexes (ground truth, P = 128, region = CDR-H3, the default thresholds), computed once."""
    from abx_amd import interface
    out = {}
    for code in ('6ct7', '6qd7'):
        c = RC.load_complex(code, 'h3')
        pts = interface.interface_host(c['x'], c['mask'], c['aa'], c['Lab'], region=c['mov'], n_points=128)[1]
        row, rows, d = PC.twin(c, c['x'], c['mask'], pts, details=True)
        out[code] = dict(c=c, pts=pts, row=row, rows=rows, d=d)
    return out


@pytest.mark.parametrize('code', ['6ct7', '6qd7'])
def test_twin_reproduces_the_prototype(shipped, code):
    """The integers exactly, the floats to the digits the prototype printed; and the invariants of the definition: D2 and S2 symmetric
    bit for bit, the per-row shares add up to twice the columns, the flags nest."""
    from abx_amd import patches
    s, want = shipped[code], PC.PROTOTYPE[code]
    row, rows, d, c = s['row'], s['rows'], s['d'], s['c']
    Lab = c['Lab']
    print(code, dict(zip(patches.PATCHES_COLUMNS, row.tolist())))
    for name in ('psh', 'ppc', 'pnc', 'sfvcsp', 'psh_region', 'cross_attract', 'cross_repel'):
        digits = len(want[name].split('.')[1])
        assert f'{row[col(name)]:.{digits}f}' == want[name], (name, row[col(name)])
    assert tuple(int(v) for v in row[11:]) == want['counts']
    D2, S2 = d['D2'], d['S2']
    assert D2.shape == (Lab, c['aa'].shape[0]) and np.array_equal(D2[:, :Lab], D2[:, :Lab].T) and np.array_equal(S2[:, :Lab], S2[:, :Lab].T)
    assert np.isinf(np.diag(D2[:, :Lab])).all() and (S2 >= D2).all()
    assert d['vicinity'].sum() == row[13] and (d['seed'] <= d['vicinity']).all() and (d['vicinity'] <= d['exposed']).all()
    assert not d['exposed'][c['aa'][:Lab].numpy() == G].any()           # Gly has no reference area
    two30 = lambda v: np.rint(v * TWO30).astype(np.int64)
    assert two30(rows[:, 0]).sum() == 2 * two30(row[0]) and two30(rows[:, 1]).sum() == 2 * (two30(row[1]) + two30(row[2]))
    assert two30(rows[:, 2]).sum() == 2 * (two30(row[7]) - two30(row[8])) and not rows[Lab:, :2].any()
    flags = rows[:, 3].astype(np.int64)
    assert ((flags & 8) != 0).sum() == row[13] and ((flags[:Lab] & 2) != 0).sum() == row[12] and not (flags[Lab:] & 30).any()
    assert np.array_equal((flags & 32) != 0, c['mov'].numpy() & d['present'])
    if code in PC.PSH_WITHOUT_OVERRIDE:             # the salt-bridge override is visible
        plain = PC.twin(c, c['x'], c['mask'], s['pts'], salt_override=False)[0]
        assert f'{plain[0]:.3f}' == PC.PSH_WITHOUT_OVERRIDE[code] and plain[5:].tolist() == row[5:].tolist() and \
            plain[1:4].tolist() == row[1:4].tolist()


def test_perturbations_move_the_vicinity_and_reach_the_floor():
    """The seeded perturbations of 6ct7 change n_vicinity and n_pairs as the prototype printed, and put atoms of two residues within
    1 Angstrom of each other: every term stays bounded by its product."""
    c = RC.load_complex('6ct7', 'h3')
    below = 0
    for seed, (n_vic, n_pairs) in PC.PERTURBED.items():
        row, rows, d = PC.twin(c, RC.perturb(c, seed), c['mask'], None, details=True)
        assert (int(row[13]), int(row[14])) == (n_vic, n_pairs), (seed, row[13], row[14])
        below += int(d['D2'].min() < 1.0)
        assert rows[:, 0].max() <= 4.0 * row[14] and np.isfinite(row).all()
    assert below >= 2
    # 6qd7, seed 5: two rows of the vicinity come within 0.3 Angstrom (D2 = 0.087), so the floor acts on a term that is counted
    q = RC.load_complex('6qd7', 'h3')
    row, rows, d = PC.twin(q, RC.perturb(q, 5), q['mask'], None, details=True)
    v = d['vicinity']
    assert f"{d['D2'][:, :q['Lab']][np.ix_(v, v)].min():.3f}" == '0.087' and np.isfinite(row).all()


def host(s, **kw):
    from abx_amd import patches
    return patches.patches_host(s['x'], s['mask'], s['aa'], s['Lab'], s['chain_id'], s['residx'], s['cdr_def'], region=s['region'],
                                points=s['points'], details=True, **kw)


def test_two_lysines_inside_and_outside_the_cutoff():
    from abx_amd import patches
    h = patches.kyte_doolittle()
    row, rows, d = host(PC.hand_built([K, K], [(0, 0, 0), (5, 0, 0)], cdr=[5, 5]))
    assert d['D2'][0, 1] == 25.0 and d['exposed'].all() and d['seed'].all()
    assert row[col('ppc')] == PC.term(1.0, 25.0) and row[col('psh')] == PC.term(h[K] * h[K], 25.0) and row[col('pnc')] == 0.0
    assert row[11:].tolist() == [2, 2, 2, 1, 0, 0, 0] and row[col('sfvcsp')] == 0.0        # one chain: the other sum is 0
    assert rows[:, 0].tolist() == [row[0], row[0]] and rows[:, 1].tolist() == [row[1], row[1]] and rows[:, 3].tolist() == [15.0, 15.0]
    far = host(PC.hand_built([K, K], [(0, 0, 0), (8, 0, 0)], cdr=[5, 5]))[0]
    assert far[:11].tolist() == [0.0] * 11 and far[11:].tolist() == [2, 2, 2, 0, 0, 0, 0]
    at = host(PC.hand_built([K, K], [(0, 0, 0), (7.5, 0, 0)], cdr=[5, 5]))[0]               # the cutoff is inclusive
    assert at[col('n_pairs')] == 1 and at[col('ppc')] == PC.term(1.0, 56.25)
    two = host(PC.hand_built([K, R], [(0, 0, 0), (5, 0, 0)], cdr=[5, 5], chain=[0, 1]))[0]  # heavy +1.0, light +1.0
    assert two[col('sfvcsp')] == 1.0 and two[col('ppc')] == PC.term(1.0, 25.0)
    neg = host(PC.hand_built([D, E, H], [(0, 0, 0), (5, 0, 0), (0, 5, 0)], cdr=[5, 5, 5], chain=[0, 1, 1]))[0]
    assert neg[col('pnc')] == PC.term(1.0, 25.0) and neg[col('ppc')] == 0.0 and neg[col('sfvcsp')] == (-10 * -9) / 100.0
    gly = host(PC.hand_built([G, X, K], [(0, 0, 0), (3, 0, 0), (0, 3, 0)], cdr=[5, 5, 5]))  # Gly and X are never exposed
    assert gly[2]['exposed'].tolist() == [False, False, True] and gly[0][11:].tolist() == [2, 1, 1, 0, 0, 0, 0]


def test_salt_bridge_override_toggles_between_3_0_and_3_4():
    from abx_amd import patches
    h = patches.kyte_doolittle()
    row, rows, d = host(PC.hand_built([K, D], [(0, 0, 0), (3, 0, 0)], cdr=[5, 5]))
    assert d['S2'][0, 1] == 9.0 and d['salt'].all() and row[col('n_salt')] == 2
    assert row[col('psh')] == PC.term(h[G] * h[G], 9.0) and row[col('ppc')] == row[col('pnc')] == 0.0 and rows[:, 3].tolist() == [31.0, 31.0]
    row, rows, d = host(PC.hand_built([K, D], [(0, 0, 0), (3.4, 0, 0)], cdr=[5, 5]))
    r2 = float(np.float32(3.4)) ** 2
    assert d['S2'][0, 1] == r2 > 3.2 * 3.2 and not d['salt'].any() and row[col('n_salt')] == 0
    assert row[col('psh')] == PC.term(h[K] * h[D], r2) and rows[:, 3].tolist() == [15.0, 15.0]
    # two like charges are no salt bridge, and an antigen row does not bridge an antibody row
    assert not host(PC.hand_built([K, R], [(0, 0, 0), (3, 0, 0)], cdr=[5, 5]))[2]['salt'].any()
    assert not host(PC.hand_built([K, D], [(0, 0, 0), (3, 0, 0)], cdr=[5, 0], Lab=1))[2]['salt'].any()


def test_vicinity_between_3_9_and_4_1():
    near = host(PC.hand_built([A, A], [(0, 0, 0), (3.9, 0, 0)], cdr=[5, 0]))
    assert near[2]['seed'].tolist() == [True, False] and near[2]['vicinity'].tolist() == [True, True] and near[0][11:].tolist() == [1, 2, 2, 1, 0, 0, 0]
    assert near[1][:, 3].tolist() == [15.0, 11.0]
    far = host(PC.hand_built([A, A], [(0, 0, 0), (4.1, 0, 0)], cdr=[5, 0]))
    assert far[2]['vicinity'].tolist() == [True, False] and far[0][11:].tolist() == [1, 2, 1, 0, 0, 0, 0] and far[0][0] == 0.0
    # a framework residue next to a framework residue in the vicinity is not in the vicinity itself
    chain = host(PC.hand_built([A, A, A], [(0, 0, 0), (3.9, 0, 0), (7.8, 0, 0)], cdr=[5, 0, 0]))
    assert chain[2]['vicinity'].tolist() == [True, True, False]


def test_coincident_atoms_keep_the_term_bounded():
    from abx_amd import patches
    h = patches.kyte_doolittle()
    row, rows, d = host(PC.hand_built([K, K], [(1, 2, 3), (1, 2, 3)], cdr=[5, 5]))
    assert d['D2'][0, 1] == 0.0 and row[col('ppc')] == 1.0 and row[col('psh')] == PC.term(h[K] * h[K], 1.0) and np.isfinite(row).all()
    cross = host(PC.hand_built([K, D, E], [(1, 2, 3), (1, 2, 3), (1, 2, 3)], cdr=[5, 0, 0], Lab=2, region=np.array([True, False, False])))
    row, rows = cross[0], cross[1]
    # K - E attract (region row), D - E repel; K and D are salt-bridged within the antibody
    assert row[7:11].tolist() == [1.0, 1.0, 1.0, 0.0] and row[16:].tolist() == [2, 1] and rows[:, 2].tolist() == [1.0, -1.0, 0.0]


@pytest.mark.parametrize('code', ['6ct7', '6qd7'])
def test_antigen_moved_away(shipped, code):
    """The antigen 100 Angstrom away: every cross column is 0; with the point counts held fixed the columns of the free antibody keep
    their bits."""
    s = shipped[code]
    c = s['c']
    row, rows = PC.twin(c, SC.antigen_moved(c), c['mask'], s['pts'])
    assert row[list(PC.CROSS_COLUMNS)].tolist() == [0.0] * 6 and not rows[:, 2].any()
    assert row[list(PC.FREE_COLUMNS)].tolist() == s['row'][list(PC.FREE_COLUMNS)].tolist()
    assert np.array_equal(rows[:, [0, 1, 3]], s['rows'][:, [0, 1, 3]])


# ---------------------------------------------------------------------------------------------------------------------
# the design driver
# ---------------------------------------------------------------------------------------------------------------------
PARSER = None


def parser():
    global PARSER
    if PARSER is None:
        from abx_amd import design
        PARSER = design.build_parser()
    return PARSER


def test_driver_declares_a_further_analysis():
    """ANALYSES keeps its order; --patches is walked after the first nine."""
    from abx_amd import analyses, patches
    before = analyses.ANALYSES[:9]
    assert [an.flag for an in analyses.ANALYSES] == ['score', 'relax', 'interface', 'confidence', 'accuracy', 'polar', 'ensemble', 'developability', 'shape', 'patches', 'torsions', 'secondary']
    assert analyses.PATCHES.kw == 'patches' and analyses.PATCHES.extra == 'patches_rows'
    assert 'patches' not in [an.flag for an in before]
    a = parser().parse_args([])
    assert a.patches is False and a.patches_rows is False
    assert (a.patches_cutoff, a.patches_vicinity, a.patches_salt, a.patches_exposed) == (7.5, 4.0, 3.2, 0.075)
    assert analyses.check_options(a, False) == []
    a = parser().parse_args(['--patches'] + ['--' + an.flag for an in before])
    active = [an.flag for an in analyses.check_options(a, True)]
    assert active[:len(before)] == [an.flag for an in before] and 'patches' in active[len(before):]
    a = parser().parse_args(['--patches', '--patches_rows', '--patches_cutoff', '6', '--patches_vicinity', '3', '--patches_salt', '4', '--patches_exposed', '0'])
    assert [an.flag for an in analyses.check_options(a, False)] == ['patches']
    NP = len(patches.PATCHES_COLUMNS)
    shapes = lambda a: {f.name: (f.dtype, f.shape, f.rows) for f in analyses.fields_of(analyses.check_options(a, False), a)}
    assert shapes(a) == {'seq': (torch.int64, ('Lab',), True), 'pLDDT': (torch.float32, ('Lab',), False),
                         'patches': (torch.float64, (2 * NP,), True), 'patches_rows': (torch.float64, ('L', 4), False)}
    a = parser().parse_args(['--patches', '--relax'])
    assert shapes(a)['patches'] == (torch.float64, (3 * NP,), True) and 'patches_rows' not in shapes(a)


THRESHOLDS = '--patches_cutoff, --patches_vicinity and --patches_salt must be > 0, --patches_exposed in [0, 1]'


@pytest.mark.parametrize('argv, set_level, text', [
    (['--patches_rows'], False, '--patches_rows needs --patches'),
    (['--patches', '--patches_rows'], True, '--patches_rows needs the sample-sharded schedule (--shard_samples): a set-level run gathers one table only'),
    (['--patches', '--patches_cutoff', '0'], False, THRESHOLDS),
    (['--patches', '--patches_vicinity', '-1'], False, THRESHOLDS),
    (['--patches', '--patches_salt', '0'], False, THRESHOLDS),
    (['--patches', '--patches_exposed', '1.5'], False, THRESHOLDS),
    (['--patches', '--patches_exposed', '-0.1'], False, THRESHOLDS),
    (['--patches', '--interface_points', '0'], False, '--interface_points must be in 1..1024, --interface_probe >= 0'),
    (['--patches', '--interface_probe', '-1'], False, '--interface_points must be in 1..1024, --interface_probe >= 0'),
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


@pytest.mark.parametrize('with_all', [False, True])
def test_zero_row_block_matches_the_filled_block(with_all):
    from abx_amd import accuracy, analyses, confidence, developability as dv, interface, metrics, patches, polar, relax, shape
    L, Lab, n = 9, 7, 2
    before = analyses.ANALYSES[:9]
    others = [an.flag for an in before] if with_all else []
    flags = others + ['patches', 'patches_rows'] + [an.extra for an in before if an.extra and with_all]
    a = parser().parse_args(['--' + f for f in flags])
    active = analyses.check_options(a, set_level=False)
    assert [an.flag for an in active] == others + ['patches']
    g = torch.Generator().manual_seed(3)
    table = lambda cols: (torch.rand(n, len(cols), generator=g, dtype=torch.float64) * 50).round(decimals=3)
    rec = {'seq': torch.randint(0, 20, (n, Lab), generator=g), 'pLDDT': torch.full((n, Lab), 70.0), 'atom14_results': torch.randn(n, Lab, 14, 3, generator=g),
           'time': 0.01, 'scores': table(metrics.SCORE_COLUMNS), 'relax': table(relax.RELAX_COLUMNS), 'scores_relaxed': table(metrics.SCORE_COLUMNS),
           'confidence_wild': table(confidence.CONFIDENCE_COLUMNS), 'confidence_planes': (torch.rand(n, L, L, generator=g), None),
           'accuracy_rows': torch.rand(n, L, 4, generator=g, dtype=torch.float64), 'polar_rows': torch.zeros(n, L, 4, dtype=torch.int32),
           'developability_rows': torch.rand(n, L, 4, generator=g, dtype=torch.float64), 'patches_rows': torch.rand(n, L, 4, generator=g, dtype=torch.float64)}
    for mod in (interface, confidence, accuracy, polar, dv, shape, patches):
        kind = mod.__name__.rsplit('.', 1)[1]
        rec[kind], rec[kind + '_relaxed'] = table(getattr(mod, kind.upper() + '_COLUMNS')), table(getattr(mod, kind.upper() + '_COLUMNS'))
    seen = []
    columns = {'interface': interface.INTERFACE_COLUMNS, 'accuracy': accuracy.ACCURACY_COLUMNS, 'polar': polar.POLAR_COLUMNS,
               'developability': dv.DEVELOPABILITY_COLUMNS, 'shape': shape.SHAPE_COLUMNS, 'patches': patches.PATCHES_COLUMNS}
    scorers = {f: Wild(c, seen) for f, c in columns.items() if f in flags}
    filled = analyses.collect(active, a, [rec], scorers)
    zero = analyses.zero_rows(active, a, L, Lab, 'cpu')
    assert list(filled) == list(zero) == [f.name for f in analyses.fields_of(active, a)] and list(zero)[-2:] == ['patches', 'patches_rows']
    for k in filled:
        assert filled[k].dtype == zero[k].dtype and filled[k].shape[1:] == zero[k].shape[1:] and filled[k].shape[0] == n and zero[k].shape[0] == 0, k
    NP = len(patches.PATCHES_COLUMNS)
    assert filled['patches'].shape == (n, (3 if with_all else 2) * NP) and bool((filled['patches'][:, -NP:] == 0.5).all())
    assert torch.equal(filled['patches'][:, :NP], rec['patches']) and torch.equal(filled['patches_rows'], rec['patches_rows'])
    if with_all:                    # one buffer of point counts serves the five wild rows; accuracy's takes none
        assert len(seen) == 6 and all(seen[k] is seen[0] for k in (2, 3, 4, 5)) and seen[0].shape == (1, 9, 14, 2) and seen[1] is None
    else:
        assert seen == [None]


def test_table_format(tmp_path):
    """A table written from fixed rows has the expected header and `wild` line: three decimals for PSH, two for SFvCSP, four for the
    charge columns, integers for the counts."""
    from abx_amd import design, patches
    NP, ND = len(patches.PATCHES_COLUMNS), len(patches.DELTA_COLUMNS)
    wild = [46.97167, 0.052723, 0.298360, 5.51, 4.356865, 0.0, 0.0, 0.239864, 0.175209, 0.002791, 0.0, 42, 135, 46, 220, 4, 12, 1]
    d0 = [50.5, 0.1, 0.25, 4.4, 6.0, 0.05, 0.0, 0.3, 0.1, 0.01, 0.0, 42, 136, 48, 238, 3, 13, 2]
    assert patches.format_patches(wild) == ['46.972', '0.0527', '0.2984', '5.51', '4.357', '0.0000', '0.0000', '0.2399', '0.1752', '0.0028', '0.0000',
                                            '42', '135', '46', '220', '4', '12', '1']
    assert patches.format_delta(d0, wild) == ['+3.528', '+0.0473', '-0.0484', '-1.11', '+1.643', '+0.0601', '-0.0752', '+0.0072', '+0.0000']
    path = design._write_patches(str(tmp_path), '6ct7_H_L_S', wild, [(0, d0 + wild), (1, wild + wild)], False)
    lines = [ln.split('\t') for ln in open(path).read().splitlines()]
    assert path.endswith('6ct7_H_L_S_patches.tsv') and len(lines) == 4
    assert lines[0] == ['sample'] + list(patches.PATCHES_COLUMNS) + ['delta_' + c for c in patches.DELTA_COLUMNS]
    assert lines[1] == ['wild'] + patches.format_patches(wild) + ['+0.000', '+0.0000', '+0.0000', '+0.00', '+0.000'] + ['+0.0000'] * 4
    assert lines[2] == ['0'] + patches.format_patches(d0) + patches.format_delta(d0, wild) and lines[3][1 + NP:] == lines[1][1 + NP:]
    path = design._write_patches(str(tmp_path), 'x_H_L_A', wild, [(5, d0 + wild + wild)], True)
    lines = [ln.split('\t') for ln in open(path).read().splitlines()]
    assert lines[0][1 + NP + ND:] == [c + '_relaxed' for c in patches.PATCHES_COLUMNS] and lines[1][1 + NP + ND:] == ['nan'] * NP
    assert lines[2] == ['5'] + patches.format_patches(d0) + patches.format_delta(d0, wild) + patches.format_patches(wild)


def test_sampler_signature_defaults_to_no_patches():
    import inspect
    from abx_amd import sampler
    assert inspect.signature(sampler.sample_fn).parameters['patches'].default is None
