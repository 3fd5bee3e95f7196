"""CPU-only checks of the secondary-structure analysis (abx_secondary_scores, abx_amd.secondary): C layout of the descriptor, argument
checks without a GPU, the float64 host twin on chains built from given dihedrals, on two-strand sheets and on the crystal complexes,
seven deliberate mistakes that each move a named column or string, breaks / a missing O / res_mask, that no decision of a structure the
GPU test scores is borderline, and the wiring of the design driver."""
import ctypes

import numpy as np
import pytest
import torch

import host_cases as HC
import relax_cases as RC
import secondary_cases as SS

NS = 22


@pytest.fixture(scope='module')
def lib():
    return HC.load_lib()


def col(name):
    from abx_amd import secondary
    return secondary.SECONDARY_COLUMNS.index(name)


def string(h):
    from abx_amd import secondary
    return ''.join(secondary.LETTERS[v] for v in h['classes'])


def pairs(h, kind):
    return int(np.triu(h[kind], 1).sum())


def test_secondary_args_match_c_layout():
    from abx_amd import _lib, secondary
    c_layout = HC.assert_c_layout({'AbxSecondaryArgs': _lib.AbxSecondaryArgs}, ['ABX_SECONDARY_COLS', 'ABX_SECONDARY_MAX_LAB'])
    assert c_layout['ABX_SECONDARY_COLS'] == _lib.SECONDARY_COLS == len(secondary.SECONDARY_COLUMNS) == NS
    assert c_layout['ABX_SECONDARY_MAX_LAB'] == _lib.SECONDARY_MAX_LAB == secondary.MAX_LAB == 800
    cols = secondary.SECONDARY_COLUMNS
    assert secondary.DELTA_COLUMNS == tuple(cols[k] for k in (1, 2, 5, 6, 9, 10, 11, 12, 13, 14, 15, 16, 20))
    assert secondary.MEAN_COLUMNS == ('hb_energy_region',) and len(secondary.COUNT_COLUMNS) == NS - 1
    assert secondary.ROW_COLUMNS == ('state', 'donated', 'accepted', 'partner0', 'partner1', 'flags') and secondary.LETTERS == '.HGIEBTS-'
    assert 'abx_secondary_scores' in _lib.EXPORTED and 'abx_secondary_scores_workspace_bytes' in _lib.EXPORTED
    th = secondary.thresholds()
    assert th['hb_energy'] == -0.5 and abs(th['bend'][0] - np.cos(np.deg2rad(70.0))) < 1e-15 and abs(th['bend'][0] ** 2 + th['bend'][1] ** 2 - 1) < 1e-15
    for bad in (0.0, 0.5, float('nan'), float('-inf')):
        with pytest.raises(ValueError):
            secondary.thresholds(bad)


def test_argument_checks_without_gpu(lib):
    """Every malformed descriptor comes back negative before any launch, with the entry's name in the error string."""
    from abx_amd import secondary
    from abx_amd._lib import AbxSecondaryArgs
    PTR = 0x1000                                    # any non-null "device pointer": nothing is dereferenced
    operands = ('pred_atom14', 'pred_seq', 'gt_atom14', 'gt_exists', 'gt_seq', 'radius', 'chain_id', 'out')
    th = secondary.thresholds()

    def good():
        a = AbxSecondaryArgs()
        for f in operands:
            setattr(a, f, PTR)
        a.B, a.L, a.Lab, a.Lpred = 4, 40, 30, 30
        a.pred_sb, a.pred_seq_sb, a.out_stride = 30 * 42, 30, NS
        a.hb_energy, a.pro = th['hb_energy'], 14
        a.bend[0], a.bend[1] = th['bend']
        return a

    def bad(a, ws=PTR):
        rc = lib.abx_secondary_scores(ctypes.byref(a) if a is not None else None, ws, None)
        msg = lib.abx_last_error_string()
        assert rc < 0 and b'abx_secondary_scores' in msg, (rc, msg)
        return msg

    bad(None)
    bad(AbxSecondaryArgs())
    assert b'null workspace' in bad(good(), ws=None)
    for field in operands:
        a = good()
        setattr(a, field, None)
        bad(a)
    for field, v in (('B', 0), ('B', 65536), ('L', 0), ('Lab', 41), ('Lab', 0), ('Lpred', 29), ('out_stride', NS - 1), ('pro', -1), ('pro', 21)):
        a = good()
        setattr(a, field, v)
        bad(a)
    for v in (0.0, 0.5, float('nan'), float('-inf')):
        a = good()
        a.hb_energy = v
        assert b'hb_energy' in bad(a)
    for v in ((2.0, 0.0), (float('nan'), 0.0), (0.0, 0.0)):
        a = good()
        a.bend[0], a.bend[1] = v
        assert b'(cos, sin)' in bad(a)
    a = good()                                      # more antibody rows than the LDS image holds
    a.L, a.Lab, a.Lpred = 900, 801, 801
    assert b'Lab <= 800' in bad(a)
    words = lambda Lab: ((Lab + 31) // 32) | 1
    for Lab in (1, 32, 33, 228, 800):
        assert lib.abx_secondary_scores_workspace_bytes(100, Lab) == 100 * Lab * (words(Lab) + 1) * 4
    assert lib.abx_secondary_scores_workspace_bytes(0, 228) == 0 and lib.abx_secondary_scores_workspace_bytes(1, 0) == 0


def test_built_chains():
    """The 12-residue chains: the alpha helix has the 8 bonds i + 4 -> i and reads -HHHHHHHHHH- (by hand: turn_4 at 0..7, start_4 at
    1..7, H from 1 to 7 + 3), the 3-10 helix 9 bonds i + 3 -> i, the pi helix 7 bonds i + 5 -> i, the two extended chains none."""
    for o in SS.built_chains():
        h = SS.twin(SS.as_complex(o['x'], o['mask']))
        assert string(h) == o['letters'] and np.argwhere(h['hb']).tolist() == o['bonds'] and h['n_borderline'] == 0, (o['letters'], string(h))
        assert pairs(h, 'par') == pairs(h, 'anti') == 0
        r = h['row']
        assert r[col('n_hb')] == r[col('n_hb_region')] == r[col('n_hb_inside')] == r[col('hb_wild_region')] == r[col('hb_kept_region')] == len(o['bonds'])
        assert r[col('n_ss')] == r[col('q8_same')] == r[col('q3_same')] == SS.N_RES
        assert h['rows'][:, 1].tolist() == h['hb'].sum(1).tolist() and h['rows'][:, 2].tolist() == h['hb'].sum(0).tolist()
        if o['bonds']:
            assert r[col('hb_energy_region')] < -0.5 * len(o['bonds']) and r[col('helix_ab')] == 10 and r[col('ss_C')] == 2
            assert r[col('hb_energy_region')] * 2 ** 20 == np.rint(r[col('hb_energy_region')] * 2 ** 20)


@pytest.mark.parametrize('parallel', [False, True])
def test_two_strand_sheets(parallel):
    """Antiparallel: -EEEEE--EEEEE-, 6 bonds, 5 antiparallel bridge pairs and no parallel one; the translated copy: 5 parallel pairs."""
    from abx_amd import secondary
    s = SS.sheet(parallel)
    h = SS.twin(SS.as_complex(s['x'], s['mask'], s['chain']))
    assert string(h) == s['letters'] and int(h['hb'].sum()) == s['bonds'] and h['n_borderline'] == 0
    assert pairs(h, 'anti') == s['anti'] and pairs(h, 'par') == s['par']
    r = h['row']
    assert r[col('n_bridge_region')] == r[col('bridge_wild_region')] == r[col('bridge_kept_region')] == 5 and r[col('strand_ab')] == r[col('ss_E')] == 10
    flag = secondary.F_PARALLEL if parallel else secondary.F_ANTIPARALLEL
    other = secondary.F_ANTIPARALLEL if parallel else secondary.F_PARALLEL
    assert all((f & flag) and not (f & other) for f in h['rows'][[1, 2, 3, 4, 5, 8, 9, 10, 11, 12], 5].tolist())
    assert h['rows'][1, 3] >= SS.N_STRAND and h['rows'][1, 4] == -1 and h['rows'][0, 3:5].tolist() == [-1, -1]


# the crystal numbers: (Lab, bonds, antiparallel pairs, parallel pairs, E rows, G rows, H rows, the string of H3, bonds touching it, inside it)
CRYSTALS = {'6qd7': (227, 150, 70, 7, 110, 15, 0, 'EEBSSSSS---B-E', 9, 5), '6ct7': (221, 144, 62, 6, 97, 15, 0, 'ESSS', 4, 2)}
HEAVY_6QD7 = '-EEEEE--EEE-TT--EEEEEEEESS-GGGS-EEEEEE-TTS-EEE-EEE-SSTT-EEE-GGGTTTEEEEEEGGGTEEEEEE-S--GGG-EEEEEEEBSSSSS---B-EE---EEEEE--'


@pytest.mark.parametrize('code', ['6qd7', '6ct7'])
def test_crystals(code):
    """The twin on the shipped crystal structures gives the numbers written down with the definitions (found: it agrees with all of
    them); under the seeded perturbations H3 of 6qd7 keeps 6, 7 and 5 of its 9 bonds and its string changes at 2, 4 and 2 positions."""
    from abx_amd import secondary
    c = RC.load_complex(code, 'h3')
    h = SS.twin(c)
    Lab, n_hb, anti, par, n_e, n_g, n_h, h3, touch, inside = CRYSTALS[code]
    cl = h['classes']
    assert (c['Lab'], int(h['hb'].sum()), pairs(h, 'anti'), pairs(h, 'par')) == (Lab, n_hb, anti, par)
    assert (int((cl == 4).sum()), int((cl == 2).sum()), int((cl == 1).sum())) == (n_e, n_g, n_h)
    assert int((h['par'] | h['anti']).sum(1).max()) == 2 and int(h['hb'].sum(1).max()) == 2 and h['n_borderline'] == 0
    assert secondary.ss_string(cl, c['mov']) == h3 and h['row'][[col('n_hb_region'), col('n_hb_inside')]].tolist() == [touch, inside]
    # wild against itself
    r = h['row']
    assert r[col('hb_wild_region')] == r[col('hb_kept_region')] == r[col('n_hb_region')]
    assert r[col('bridge_wild_region')] == r[col('bridge_kept_region')] == r[col('n_bridge_region')]
    assert r[col('n_ss')] == r[col('q8_same')] == r[col('q3_same')] == len(h3)
    assert r[col('strand_ab')] == ((cl == 4) | (cl == 5)).sum() and r[col('helix_ab')] == n_g and np.array_equal(cl, h['wild_classes'])
    if code == '6qd7':
        heavy = c['chain'][:Lab] == c['chain'][torch.nonzero(c['mov'])[0, 0]]
        assert secondary.ss_string(cl, heavy) == HEAVY_6QD7
        kept, changed = [], []
        for seed in RC.SEEDS:
            p = SS.twin(c, RC.perturb(c, seed))
            kept.append(int(p['row'][col('hb_kept_region')]))
            changed.append(sum(a != b for a, b in zip(secondary.ss_string(p['classes'], c['mov']), h3)))
            assert p['row'][col('hb_wild_region')] == touch and p['row'][col('n_ss')] == len(h3) and p['row'][col('q8_same')] == len(h3) - changed[-1]
        assert kept == [6, 7, 5] and changed == [2, 4, 2]


def test_no_borderline_decision_on_what_the_gpu_scores():
    """Every structure tests/test_gpu_secondary.py compares with the twin: no energy within 1e-9 relative of the threshold, no C-alpha
    distance of the cutoff, no bend of its angle - the device cannot take a decision differently."""
    for code, sel in RC.MOVABLE_SETS[:2]:
        c = RC.load_complex(code, sel)
        for x, seq, mask in SS.gpu_structures(c):
            assert SS.twin(c, x, mask=mask, seq=seq)['n_borderline'] == 0
    cx, xh, region = SS.tiny_structures()
    for k in range(2):
        assert SS.synthetic_twin(cx, xh[k], region)['n_borderline'] == 0
    assert SS.synthetic_twin(cx, cx['atom14_gt_positions'], region)['n_borderline'] == 0       # the wild line of the driver test
    for n in (1, 2, 4, 5, 31, 32, 33, 40, 64, 65, 255, 256, 257, 800):      # the Lab edges, the shapes of the limits and of the reused workspace
        c = SS.concatenated(n)
        assert SS.twin(c)['n_borderline'] == 0
        m2 = c['mask'].clone()                          # the second structure of the Lab edges: the O of the middle row missing
        m2[n // 2, 3] = False
        assert SS.twin(c, mask=m2)['n_borderline'] == 0
    c = RC.load_complex('6ct7', 'h3')                   # the two structures scored with a row taken out by res_mask
    keep = torch.ones(c['aa'].shape[0], dtype=torch.uint8)
    keep[int(torch.nonzero(c['mov'])[1, 0])] = 0
    for x, seq, mask in SS.gpu_structures(c)[:2]:
        assert SS.twin(c, x, mask=mask, seq=seq, res_mask=keep)['n_borderline'] == 0
    for o in SS.built_chains():                         # the built chains against the helix, the sheets against the antiparallel one
        helix = SS.built_chains()[0]
        assert SS.twin(SS.as_complex(helix['x'], helix['mask']), torch.from_numpy(o['x']))['n_borderline'] == 0
    anti, par = SS.sheet(False), SS.sheet(True)
    assert SS.twin(SS.as_complex(anti['x'], anti['mask'], anti['chain']), torch.from_numpy(par['x']))['n_borderline'] == 0


def test_mistakes_move_a_named_column_or_string():
    from abx_amd import secondary
    helix = SS.built_chains()[0]
    c = SS.as_complex(helix['x'], helix['mask'])
    right = SS.twin(c)
    # donor and acceptor swapped: hb(i -> i+4) is no longer read as a turn at i; row 0 donates instead of accepting
    h = SS.twin(c, mistake='acceptor_donor_swapped')
    assert 'H' not in string(h) and h['rows'][0, 1:3].tolist() == [1, 0] and right['rows'][0, 1:3].tolist() == [0, 1]
    # the own peptide bond counted: N-H of i against C=O of i-1 lies far below -0.5 kcal/mol: 11 bonds more
    h = SS.twin(c, mistake='own_peptide_bond')
    assert h['row'][col('n_hb')] == right['row'][col('n_hb')] + 11 == 19
    # Pro donates: a poly-Pro helix has no H at all
    pro = torch.full((SS.N_RES,), secondary.type_index('P'))
    assert SS.twin(c, seq=pro)['row'][col('n_hb')] == 0 and not (SS.twin(c, seq=pro)['rows'][:, 5] & secondary.F_HAS_H).any()
    assert SS.twin(c, seq=pro, mistake='pro_donates')['row'][col('n_hb')] == 8
    # H built from C and O of the own row: in a strand it points along the chain, the six bonds of the sheet are lost
    s = SS.sheet()
    cs = SS.as_complex(s['x'], s['mask'], s['chain'])
    h = SS.twin(cs, mistake='h_from_own_row')
    assert SS.twin(cs)['row'][col('n_hb')] == 6 and h['row'][col('n_hb')] == 0 and string(h) == '-' * 14
    # chains linked: the first row of the second strand gets an H
    h = SS.twin(cs, mistake='chain_linked')
    assert h['rows'][SS.N_STRAND, 5] & secondary.F_HAS_H and not SS.twin(cs)['rows'][SS.N_STRAND, 5] & secondary.F_HAS_H
    # parallel read as antiparallel: the bridges stay, the ladder rule of the other type finds no neighbour: B, not E
    h = SS.twin(cs, mistake='parallel_as_antiparallel')
    assert string(h) == '-BBBBB--BBBBB-' and h['row'][col('ss_B')] == 10 and h['rows'][1, 5] & secondary.F_PARALLEL
    # G over H: a helix with both the i+3 and the i+4 bonds is H; with the priority reversed G
    x, mask = SS.chain_of(*SS.BOTH_TURNS)
    cb = SS.as_complex(x, mask)
    assert int(SS.twin(cb)['hb'].sum()) == 17 and string(SS.twin(cb)) == '-HHHHHHHHHH-' and string(SS.twin(cb, mistake='g_over_h')) == '-GGGGGGGGGG-'


def test_breaks_undefine_turns_and_bridges():
    """A residx gap before row 6 of the helix: the bonds stay, but the turns that span the gap (rows 2..5 for n = 4) do not, and row 6
    has no H; a missing O or res_mask = 0 at row 6 removes the row, its bonds as donor and as acceptor, and both links."""
    from abx_amd import secondary
    G = SS.GAP_AT
    turn4 = lambda h: [bool(f & secondary.F_TURN4) for f in h['rows'][:, 5].tolist()]
    h = SS.twin(SS.helix_with_gap())
    assert turn4(h) == [True, True] + [False] * 4 + [True, True] + [False] * 4
    assert int(h['hb'].sum()) == 7 and not h['rows'][G, 5] & secondary.F_HAS_H and h['rows'][G, 1] == 0
    assert string(h) == '-HHHH--HHHH-'                   # start_4 at 1 (turns 0, 1): H over 1..4; start_4 at 7 (turns 6, 7): H over 7..10
    c, m = SS.helix_without_o()
    for kw in (dict(mask=m), dict(res_mask=SS.res_mask_without(SS.N_RES))):
        h = SS.twin(c, **kw)
        assert h['classes'][G] == 0 and not h['rows'][G, 5] & secondary.F_PRESENT and h['rows'][G, 1:3].tolist() == [0, 0]
        assert int(h['hb'].sum()) == 5 and not h['rows'][G + 1, 5] & secondary.F_HAS_H                 # donors 6, 7 and acceptor 6 (of donor 10) are gone
        assert turn4(h)[2:7] == [False] * 5 and h['row'][col('n_ss')] == SS.N_RES - 1
    # a bridge next to a removed row: the sheet without row 3 keeps no bridge at rows 2, 3, 4
    s = SS.sheet()
    cs = SS.as_complex(s['x'], s['mask'], s['chain'])
    h = SS.twin(cs, res_mask=SS.res_mask_without(2 * SS.N_STRAND, 3))
    assert not (h['par'] | h['anti'])[2:5].any() and pairs(h, 'anti') < 5 and string(h)[2:5] == '-.-'


# ---------------------------------------------------------------------------------------------------------------------
PARSER = None


def parser():
    global PARSER
    if PARSER is None:
        from abx_amd import design
        PARSER = design.build_parser()
    return PARSER


def test_driver_declares_a_further_analysis():
    """ANALYSES keeps its order: --patches stays in front, --secondary is walked after --torsions."""
    from abx_amd import analyses
    before = analyses.ANALYSES[:9]
    further = [an.flag for an in analyses.ANALYSES[9:]]
    assert [an.flag for an in analyses.ANALYSES] == ['score', 'relax', 'interface', 'confidence', 'accuracy', 'polar', 'ensemble', 'developability', 'shape', 'patches', 'torsions', 'secondary']
    assert [an.flag for an in before] == ['score', 'relax', 'interface', 'confidence', 'accuracy', 'polar', 'ensemble', 'developability', 'shape']
    assert further[0] == 'patches' and further.index('secondary') > further.index('torsions') > 0
    assert analyses.SECONDARY.kw == 'secondary' and analyses.SECONDARY.extra == 'secondary_rows'
    a = parser().parse_args([])
    assert a.secondary is False and a.secondary_rows is False and a.secondary_hb_energy == -0.5
    assert analyses.check_options(a, False) == []
    a = parser().parse_args(['--secondary'] + ['--' + an.flag for an in before])
    active = [an.flag for an in analyses.check_options(a, True)]
    assert active[:len(before)] == [an.flag for an in before] and 'secondary' in active[len(before):]
    a = parser().parse_args(['--secondary', '--secondary_rows', '--secondary_hb_energy', '-1'])
    assert [an.flag for an in analyses.check_options(a, False)] == ['secondary']
    shapes = lambda a: {f.name: (f.dtype, f.shape, f.rows) for f in analyses.fields_of(analyses.check_options(a, False), a)}
    assert shapes(a) == {'seq': (torch.int64, ('Lab',), True), 'pLDDT': (torch.float32, ('Lab',), False), 'secondary': (torch.float64, (2 * NS,), True),
                         'secondary_ss': (torch.int32, (3, 'Lab'), True), 'secondary_rows': (torch.int32, ('Lab', 6), False)}
    a = parser().parse_args(['--secondary', '--relax'])
    assert shapes(a)['secondary'] == (torch.float64, (3 * NS,), True) and 'secondary_rows' not in shapes(a)
    a = parser().parse_args(['--torsions', '--secondary'])
    assert [an.flag for an in analyses.check_options(a, True)] == ['torsions', 'secondary']


@pytest.mark.parametrize('argv, set_level, text', [
    (['--secondary_rows'], False, '--secondary_rows needs --secondary'),
    (['--secondary', '--secondary_rows'], True, '--secondary_rows needs the sample-sharded schedule (--shard_samples): a set-level run gathers one table only'),
    (['--secondary', '--secondary_hb_energy', '0'], False, '--secondary_hb_energy must be a finite energy below 0 kcal/mol'),
    (['--secondary', '--secondary_hb_energy', '0.5'], False, '--secondary_hb_energy must be a finite energy below 0 kcal/mol'),
    (['--secondary', '--secondary_hb_energy', 'nan'], False, '--secondary_hb_energy must be a finite energy below 0 kcal/mol'),
    (['--secondary', '--secondary_hb_energy=-inf'], False, '--secondary_hb_energy must be a finite energy below 0 kcal/mol'),
])
def test_option_checks_exit_by_name(argv, set_level, text):
    from abx_amd import analyses
    with pytest.raises(SystemExit) as e:
        analyses.check_options(parser().parse_args(argv), set_level)
    assert e.value.code == text


class Scorer:
    """A SecondaryScorer as analyses.collect sees one: a wild row with its states, the region and Lab."""

    def __init__(self, Lab, L, wild_states):
        self.Lab, self.states = Lab, torch.tensor(wild_states, dtype=torch.int32)
        self.region = torch.zeros(L, dtype=torch.uint8)
        self.region[2:5] = 1

    def new_classes(self, B):
        return torch.zeros(B, self.Lab, dtype=torch.int32)

    def wild(self, classes=None):
        classes[0] = self.states
        return torch.full((1, NS), 0.5, dtype=torch.float64)


@pytest.mark.parametrize('relax', [False, True])
def test_fields_round_trip_and_table(tmp_path, relax):
    """The filled block and the zero-row block have the same fields; RowLayout carries the row and the states through a set-level row
    (a wider layout than the job's Lab); the writer puts the header, the `wild` line and the `dssp` column."""
    from abx_amd import analyses, design, secondary
    L, Lab, n = 9, 7, 2
    a = parser().parse_args(['--secondary'] + (['--relax'] if relax else ['--secondary_rows']))
    active = [an for an in analyses.check_options(a, set_level=False) if an.flag == 'secondary']
    g = torch.Generator().manual_seed(3)
    table = lambda: (torch.rand(n, NS, generator=g, dtype=torch.float64) * 50).round()
    rec = {'seq': torch.randint(0, 20, (n, Lab), generator=g), 'pLDDT': torch.full((n, Lab), 70.0), 'secondary': table(), 'secondary_relaxed': table(),
           'secondary_classes': torch.tensor([[8, 1, 2, 3, 4, 5, 0], [8, 6, 7, 8, 4, 4, 8]], dtype=torch.int32),
           'secondary_rows': torch.randint(-1, 300, (n, Lab, 6), generator=g, dtype=torch.int32)}
    sc = Scorer(Lab, L, [8, 4, 4, 5, 6, 7, 8])
    filled = analyses.collect(active, a, [rec], {'secondary': sc})
    zero = analyses.zero_rows(active, a, L, Lab, 'cpu')
    assert list(filled) == list(zero) == [f.name for f in analyses.fields_of(active, a)]
    assert list(filled)[2:] == ['secondary', 'secondary_ss'] + ([] if relax else ['secondary_rows'])
    for k in filled:
        assert filled[k].dtype == zero[k].dtype and filled[k].shape[1:] == zero[k].shape[1:] and filled[k].shape[0] == n and zero[k].shape[0] == 0, k
    assert filled['secondary'].shape == (n, (3 if relax else 2) * NS) and bool((filled['secondary'][:, -NS:] == 0.5).all())
    assert torch.equal(filled['secondary'][:, :NS], rec['secondary']) and filled['secondary_ss'].shape == (n, 3, Lab)
    assert torch.equal(filled['secondary_ss'][:, 0], rec['secondary_classes']) and filled['secondary_ss'][1, 1].tolist() == [8, 4, 4, 5, 6, 7, 8]
    assert filled['secondary_ss'][0, 2].tolist() == [0, 0, 1, 1, 1, 0, 0]
    # through the rows of a set-level run
    rows_fields = [f for f in analyses.fields_of(active, a) if f.rows]
    layout = analyses.RowLayout(rows_fields, maxLab=Lab + 4)
    ids, F = layout.unpack(layout.pack(3, [11, 10], filled))
    assert ids == [10, 11] and torch.equal(F['secondary_ss'], filled['secondary_ss'].flip(0)) and F['secondary_ss'].dtype == torch.int32
    assert torch.equal(F['secondary'], filled['secondary'].flip(0)) and torch.equal(F['seq'], rec['seq'].flip(0))
    # the table
    files = active[0].write(a, str(tmp_path), 'x_H_L_A', [0, 1], filled, None)
    assert [f.rsplit('/', 1)[1] for f in files] == ['x_H_L_A_secondary.tsv'] + ([] if relax else ['x_H_L_A_secondary_rows.npy'])
    lines = [ln.split('\t') for ln in open(files[0]).read().splitlines()]
    ND = len(secondary.DELTA_COLUMNS)
    head = ['sample'] + list(secondary.SECONDARY_COLUMNS) + ['delta_' + c for c in secondary.DELTA_COLUMNS]
    assert lines[0] == head + ([c + '_relaxed' for c in secondary.SECONDARY_COLUMNS] if relax else []) + ['dssp'] and len(lines) == 4
    wild = [0.5] * NS
    assert lines[1] == ['wild'] + secondary.format_secondary(wild) + secondary.format_delta(wild, wild) + (['nan'] * NS if relax else []) + ['EBT']
    assert lines[2][0] == '0' and lines[2][1:1 + NS] == secondary.format_secondary(rec['secondary'][0].tolist()) and lines[2][-1] == 'GIE' and lines[3][-1] == 'S-E'
    assert lines[2][1 + NS:1 + NS + ND] == secondary.format_delta(rec['secondary'][0].tolist(), wild)
    if relax:
        assert lines[3][1 + NS + ND:-1] == secondary.format_secondary(rec['secondary_relaxed'][1].tolist())
    else:
        got = np.load(files[1])
        assert got.dtype == np.int32 and np.array_equal(got, rec['secondary_rows'].numpy())
    # the writer under the name design exports; no strings: '-'
    path = design._write_secondary(str(tmp_path), 'y_H_L_A', wild, [(5, rec['secondary'][0].tolist() + wild)], False)
    assert open(path).read().splitlines()[2].split('\t')[-1] == '-'


def test_format_and_string():
    from abx_amd import secondary
    row = [150, 9, 5, 9, 6, -15.287378, 5, 5, 4, 0, 0, 0, 3, 2, 0, 5, 4, 14, 12, 13, 112, 15]
    assert secondary.format_secondary(row) == ['150', '9', '5', '9', '6', '-15.29', '5', '5', '4', '0', '0', '0', '3', '2', '0', '5', '4', '14', '12', '13', '112', '15']
    wild = [150, 9, 5, 9, 9, -16.0, 5, 5, 5, 0, 0, 0, 4, 2, 0, 4, 4, 14, 14, 14, 110, 15]
    assert secondary.format_delta(row, wild) == ['+0', '+0', '+0.71', '+0', '+0', '+0', '+0', '-1', '+0', '+0', '+1', '+0', '+2']
    assert secondary.ss_string([0, 1, 2, 3, 4, 5, 6, 7, 8], [1] * 9 + [0, 0]) == '.HGIEBTS-' and secondary.ss_string([4, 4, 8], [0, 1, 1]) == 'E-'


def test_sampler_signature_defaults_to_no_secondary():
    import inspect
    from abx_amd import sampler
    assert inspect.signature(sampler.sample_fn).parameters['secondary'].default is None
