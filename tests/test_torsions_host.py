"""CPU-only checks of the torsion analysis (abx_torsion_scores, abx_amd.torsions): C layout of the descriptor, argument checks without a
GPU, the float64 host twin on chains built from given dihedrals, on the crystal complexes and on structures with one chi angle turned or
one residue mutated, six deliberate mistakes that each move a named column, that no decision of a structure the GPU test scores is
borderline, and the wiring of the design driver."""
import ctypes

import numpy as np
import pytest
import torch

import analysis_gpu_cases as AG
import host_cases as HC
import relax_cases as RC
import torsions_cases as TC


@pytest.fixture(scope='module')
def lib():
    return HC.load_lib()


def col(name):
    from abx_amd import torsions
    return torsions.TORSIONS_COLUMNS.index(name)


def test_torsion_args_match_c_layout():
    from abx_amd import _lib, torsions
    c_layout = HC.assert_c_layout({'AbxTorsionArgs': _lib.AbxTorsionArgs}, ['ABX_TORSION_COLS', 'ABX_TORSION_MAX_LAB'])
    assert c_layout['ABX_TORSION_COLS'] == _lib.TORSION_COLS == len(torsions.TORSIONS_COLUMNS) == 25
    assert c_layout['ABX_TORSION_MAX_LAB'] == _lib.TORSION_MAX_LAB == torsions.MAX_LAB == 800
    assert set(torsions.DELTA_COLUMNS) <= set(torsions.COUNT_COLUMNS) and len(torsions.DELTA_COLUMNS) == 12
    assert torsions.MEAN_COLUMNS == ('dphi_region', 'dpsi_region', 'domega_region', 'dbb_max_region', 'chi_mae_region')
    assert len(torsions.ROW_COLUMNS) == 8 and torsions.ABEGO == '-ABGEO'
    assert 'abx_torsion_scores' in _lib.EXPORTED and 'abx_torsion_scores_workspace_bytes' in _lib.EXPORTED


def test_argument_checks_without_gpu(lib):
    """Every malformed descriptor comes back negative before any launch, with the entry's name in the error string."""
    from abx_amd import torsions
    from abx_amd._lib import AbxTorsionArgs
    PTR = 0x1000                                    # any non-null "device pointer": nothing is dereferenced
    operands = ('pred_atom14', 'pred_seq', 'gt_atom14', 'gt_exists', 'gt_seq', 'radius', 'chain_id', 'chi_atoms', 'chi_pi', 'out')
    pairs = ('cis', 'trans', 'o', 'a_mid', 'a_half', 'g_half', 'chi_tol')
    th = torsions.thresholds(40.0)

    def good():
        a = AbxTorsionArgs()
        for f in operands:
            setattr(a, f, PTR)
        a.B, a.L, a.Lab, a.Lpred = 4, 40, 30, 30
        a.pred_sb, a.pred_seq_sb, a.out_stride = 30 * 42, 30, 25
        for p in pairs:
            getattr(a, p)[0], getattr(a, p)[1] = th[p]
        a.gly, a.pro = 7, 14
        return a

    def bad(a, ws=PTR):
        rc = lib.abx_torsion_scores(ctypes.byref(a) if a is not None else None, ws, None)
        msg = lib.abx_last_error_string()
        assert rc < 0 and b'abx_torsion_scores' in msg, (rc, msg)
        return msg

    bad(None)
    bad(AbxTorsionArgs())
    bad(good(), ws=None)
    for field in operands:
        a = good()
        setattr(a, field, None)
        bad(a)
    for field, v in (('B', 0), ('B', 65536), ('L', 0), ('Lab', 41), ('Lab', 0), ('Lpred', 29), ('out_stride', 24), ('gly', -1), ('gly', 21), ('pro', 21)):
        a = good()
        setattr(a, field, v)
        bad(a)
    for p in pairs:
        for v in ((2.0, 0.0), (float('nan'), 0.0), (0.0, 0.0)):
            a = good()
            getattr(a, p)[0], getattr(a, p)[1] = v
            assert b'(cos, sin)' in bad(a)
    a = good()                                      # more antibody rows than the LDS image holds
    a.L, a.Lab, a.Lpred = 900, 801, 801
    assert b'Lab <= 800' in bad(a)
    assert lib.abx_torsion_scores_workspace_bytes(100, 228) == 100 * 228 * 16 * 8
    assert lib.abx_torsion_scores_workspace_bytes(0, 228) == 0 and lib.abx_torsion_scores_workspace_bytes(1, 0) == 0


def test_tables_and_thresholds():
    """The chi table in atom14 slots: Asp chi2 = CA CB CG OD1 and folded, Leu chi2 not folded, Ala and Gly without chi; the pairs are
    unit vectors of the named angles."""
    from abx_amd import residue_constants as rc, torsions
    atoms, pi = torsions.chi_table()
    assert atoms.shape == (21, 4, 4) and atoms.dtype == np.int32 and pi.shape == (21, 4) and pi.dtype == np.uint8
    names = lambda t, k: [rc.restype_name_to_atom14_names[rc.restype_1to3[rc.restypes[t]]][s] for s in atoms[t, k]]
    assert names(TC.D_, 0) == ['N', 'CA', 'CB', 'CG'] and names(TC.D_, 1) == ['CA', 'CB', 'CG', 'OD1'] and names(TC.L_, 1) == ['CA', 'CB', 'CG', 'CD1']
    assert names(TC.K_, 3) == ['CG', 'CD', 'CE', 'NZ'] and (atoms[[TC.A_, TC.G_, 20]] == -1).all() and (atoms[TC.D_, 2:] == -1).all()
    assert [(t, k) for t in range(21) for k in range(4) if pi[t, k]] == [(TC.D_, 1), (TC.E_, 2), (TC.F_, 1), (TC.Y_, 1)]
    th = torsions.thresholds(40.0)
    assert set(th) == {'cis', 'trans', 'o', 'a_mid', 'a_half', 'g_half', 'chi_tol'}
    for k, deg in dict(torsions.ANGLES, chi_tol=40.0).items():
        assert abs(np.degrees(np.arctan2(th[k][1], th[k][0])) - deg) < 1e-12, k
    for bad_tol in (0.0, -1.0, 180.5):
        with pytest.raises(ValueError, match='chi_tol'):
            torsions.thresholds(bad_tol)
    assert torsions.abego_string([1, 2, 0, 5, 3, 4], [1, 1, 1, 0, 1, 1, 0, 0]) == 'AB-GE'


# ---------------------------------------------------------------------------------------------------------------------
# built chains
# ---------------------------------------------------------------------------------------------------------------------
def test_built_chains_are_measured_and_classified():
    """Every interior phi / psi / omega within 0.01 degrees of the built value: float32 coordinates of a chain under 64 Angstrom are
    rounded by at most 4e-6 Angstrom against bond vectors of at least 1.2 Angstrom, about 1e-5 rad or 6e-4 degrees per dihedral, and
    0.01 leaves a factor of ten.  The classes, the cis and the twisted counts are exactly the built ones: every built angle lies at
    least 10 degrees from every boundary."""
    from abx_amd import torsions
    chains = TC.built_chains()
    assert len(chains) == 5 and all(ch['x'].shape == (TC.N_RES, 14, 3) and np.abs(ch['x']).max() < 64.0 for ch in chains)
    circ = lambda a, b: np.abs((a - b + 180.0) % 360.0 - 180.0)
    for k, ch in enumerate(chains):
        c = TC.chain_complex(ch)
        h = TC.twin(c, c['x'])
        rows = h['rows']
        n = TC.N_RES
        assert circ(rows[1:, 0], ch['phi'][1:]).max() < 0.01 and circ(rows[:-1, 1], ch['psi'][:-1]).max() < 0.01, k
        assert circ(rows[1:, 2], ch['omega'][1:]).max() < 0.01, k
        assert np.isnan(rows[0, [0, 2]]).all() and np.isnan(rows[n - 1, 1]) and np.isnan(rows[:, 3:7]).all()
        assert ''.join(torsions.ABEGO[v] for v in h['classes']) == ch['letters'], k
        row = h['row']
        assert row[col('n_links')] == n - 1 and row[col('cis')] == ch['cis'] == row[col('cis_nonpro')] and row[col('twisted')] == ch['twisted']
        assert row[col('n_abego')] == row[col('abego_same')] == n - 2 and row[col('n_chi1')] == 0 and np.isnan(row[col('chi_mae_region')])
        assert row[col('phi_pos')] == (n - 1 if ch['phi'][1] > 0 else 0)
        assert h['n_borderline'] == 0
    # the cis link is flagged on its upper residue, the twisted one too
    flags = TC.twin(TC.chain_complex(chains[4]), torch.from_numpy(chains[4]['x']))['rows'][:, 7].astype(np.int64)
    assert [int(f) & (torsions.F_CIS | torsions.F_TWISTED) for f in flags] == [torsions.F_CIS if i == TC.CIS_LINK else torsions.F_TWISTED if i == TC.TWISTED_LINK
                                                                              else 0 for i in range(TC.N_RES)]
    # a strand against the helix: six residues compared, none in the same class, phi differs by 63 and psi by 177 degrees
    h = TC.twin(TC.chain_complex(chains[0]), torch.from_numpy(chains[1]['x']))
    assert h['row'][col('n_abego')] == 6 and h['row'][col('abego_same')] == 0
    assert abs(h['row'][col('dphi_region')] - 63.0) < 0.01 and abs(h['row'][col('dpsi_region')] - 177.0) < 0.01 and abs(h['row'][col('dbb_max_region')] - 177.0) < 0.01


# ---------------------------------------------------------------------------------------------------------------------
# the shipped complexes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def crystal():
    out = {}
    for code, sel in RC.MOVABLE_SETS:
        c = RC.load_complex(code, sel)
        out[code, sel] = dict(c=c, h=TC.twin(c, c['x']))
    return out


@pytest.mark.parametrize('code, sel', RC.MOVABLE_SETS)
def test_the_wild_row(crystal, code, sel):
    """The crystal structure against itself: every class kept, every difference 0, every compared chi recovered."""
    from abx_amd import torsions
    c, h = crystal[code, sel]['c'], crystal[code, sel]['h']
    row = h['row']
    print(code, sel, dict(zip(torsions.TORSIONS_COLUMNS, row.tolist())), torsions.abego_string(h['classes'], c['mov']))
    assert row[col('abego_same')] == row[col('n_abego')] > 0 and np.array_equal(h['classes'], h['wild_classes'])
    assert [row[col(n)] for n in torsions.MEAN_COLUMNS] == [0.0] * 5
    assert row[col('chi1_ok')] == row[col('n_chi1')] > 0 and row[col('chi12_ok')] == row[col('n_chi12')] <= row[col('n_chi1')]
    assert row[col('cis_nonpro')] <= row[col('cis')] and row[col('n_links_region')] <= row[col('n_links')] < c['Lab']
    assert h['n_borderline'] == 0
    if code == '6qd7':
        assert row[col('cis')] == 3 and row[col('cis_nonpro')] == 0
        if sel == 'h3':
            assert torsions.abego_string(h['classes'], c['mov']) == 'BBBABAABABOBAB' and row[col('cis_region')] == 1 and row[col('abego_O')] == 1
    else:
        assert row[col('cis')] == 0 and torsions.abego_string(h['classes'], c['mov']) == 'BBGB' and row[col('phi_pos_region')] == 1


def test_perturbations_twist_peptides(crystal):
    """One seeded relax_cases.perturb of each complex adds twisted peptides and moves the backbone angles of the region."""
    for (code, sel), s in crystal.items():
        c = s['c']
        for seed in TC.SEEDS:
            row = TC.twin(c, RC.perturb(c, seed))['row']
            assert 1 <= row[col('twisted')] - s['h']['row'][col('twisted')] <= 20 and row[col('twisted_region')] == row[col('twisted')], (code, sel, seed)
            assert row[col('dphi_region')] > 5.0 and row[col('dbb_max_region')] >= max(row[col('dphi_region')], row[col('dpsi_region')])
            assert row[col('n_links')] == s['h']['row'][col('n_links')]              # a moved residue keeps its links: no distance is asked


# ---------------------------------------------------------------------------------------------------------------------
# chi
# ---------------------------------------------------------------------------------------------------------------------
def test_chi_recovery(crystal):
    """chi1 turned by 30 degrees stays recovered, by 50 it does not; an Asp or a Phe chi2 turned by 180 stays recovered (the two ends are
    the same group), a Leu chi2 does not; a mutated residue leaves the comparison."""
    from abx_amd import torsions
    c, w = crystal['6qd7', 'all']['c'], crystal['6qd7', 'all']['h']['row']
    x0 = c['x'].float().double()
    asp, phe, leu = TC.region_rows(c, TC.D_)[-1], TC.region_rows(c, TC.F_)[-1], TC.region_rows(c, TC.L_)[0]
    flag = lambda h, r: int(h['rows'][r, 7])
    near = TC.twin(c, TC.turn_chi(c, x0, asp, 1, 30.0))
    assert near['row'][col('chi1_ok')] == w[col('chi1_ok')] and flag(near, asp) & torsions.F_CHI1_OK and 0.0 < near['row'][col('chi_mae_region')] < 30.0
    far = TC.twin(c, TC.turn_chi(c, x0, asp, 1, 50.0))
    assert far['row'][col('chi1_ok')] == w[col('chi1_ok')] - 1 and far['row'][col('n_chi1')] == w[col('n_chi1')]
    assert flag(far, asp) & torsions.F_CHI1 and not flag(far, asp) & torsions.F_CHI1_OK and far['row'][col('chi12_ok')] == w[col('chi12_ok')] - 1
    assert abs(abs((far['rows'][asp, 3] - crystal['6qd7', 'all']['h']['rows'][asp, 3] + 180.0) % 360.0 - 180.0) - 50.0) < 0.01
    for r in (asp, phe):
        flip = TC.twin(c, TC.turn_chi(c, x0, r, 2, 180.0))
        assert flip['row'][col('chi12_ok')] == w[col('chi12_ok')] and flip['row'][col('chi_mae_region')] < 1e-3, r
    flip = TC.twin(c, TC.turn_chi(c, x0, leu, 2, 180.0))
    assert flip['row'][col('chi12_ok')] == w[col('chi12_ok')] - 1 and flip['row'][col('chi1_ok')] == w[col('chi1_ok')] and flip['row'][col('chi_mae_region')] > 1.0
    seq, mask = TC.mutate(c, c['aa'], [asp], TC.A_)
    mut = TC.twin(c, x0, mask=mask, seq=seq)['row']
    assert mut[col('n_chi1')] == w[col('n_chi1')] - 1 and mut[col('n_chi12')] == w[col('n_chi12')] - 1 and mut[col('chi1_ok')] == mut[col('n_chi1')]
    seq, mask = TC.mutate(c, c['aa'], [asp], TC.N_)           # Asn has the Asp atoms in other slots' names: still a mutation
    assert TC.twin(c, x0, mask=mask, seq=seq)['row'][col('n_chi1')] == w[col('n_chi1')] - 1
    # a wider tolerance recovers the 50 degree turn
    assert TC.twin(c, TC.turn_chi(c, x0, asp, 1, 50.0), chi_tol=60.0)['row'][col('chi1_ok')] == w[col('chi1_ok')]


@pytest.mark.parametrize('mistake, code, column', [
    ('atan2_swapped', '6ct7', 'twisted'),               # every trans peptide reads as 90 degrees
    ('phi_next', '6ct7', 'phi_pos'),                    # phi taken with residue i + 1
    ('omega_following', '6qd7', 'cis_nonpro'),          # the cis peptides before Pro move onto the residue in front of it
    ('chain_linked', '6ct7', 'n_links'),                # the H -> L boundary linked
    ('chi_unfolded', '6qd7', 'chi12_ok'),               # an Asp chi2 flipped by 180 degrees no longer counts as recovered
    ('gly_phi_pos', '6ct7', 'phi_pos'),                 # Gly counted
])
def test_a_deliberate_mistake_moves_its_column(mistake, code, column):
    c = RC.load_complex(code, 'all' if code == '6qd7' else 'h3')
    x = c['x'].float().double()
    if mistake == 'chi_unfolded':
        x = TC.turn_chi(c, x, TC.region_rows(c, TC.D_)[-1], 2, 180.0)
    good, wrong = TC.twin(c, x)['row'], TC.twin(c, x, mistake=mistake)['row']
    print(mistake, code, column, good[col(column)], wrong[col(column)])
    assert good[col(column)] != wrong[col(column)]
    if mistake == 'chain_linked':
        assert wrong[col(column)] == good[col(column)] + 1


# ---------------------------------------------------------------------------------------------------------------------
# no borderline decision in what the GPU test scores
# ---------------------------------------------------------------------------------------------------------------------
def test_no_structure_of_the_gpu_test_is_borderline():
    """n_borderline == 0 for the built chains, the seven structures of every movable set (typed masks too), the tiny workload, the
    structure with CA masked out and structure 57 of the L = 352 batch."""
    from abx_amd import residue_constants as rc
    chains = TC.built_chains()
    for k in (0, 1):
        c = TC.chain_complex(chains[k])
        assert all(TC.twin(c, torch.from_numpy(o['x']))['n_borderline'] == 0 for o in chains)
    for code, sel in RC.MOVABLE_SETS:
        c = RC.load_complex(code, sel)
        for k, (x, seq, mask) in enumerate(TC.gpu_structures(c)):
            assert TC.twin(c, x, mask=mask, seq=seq)['n_borderline'] == 0, (code, sel, k)
            if (code, sel) == ('6ct7', 'h3') and k in (0, 2, 5):
                typed = torch.zeros_like(c['mask'])
                typed[:c['Lab']] = torch.as_tensor(rc.restype_atom14_mask)[seq[:c['Lab']]].bool()
                assert TC.twin(c, x, mask=typed, seq=seq)['n_borderline'] == 0, ('typed', k)
    cx, xh, region = TC.tiny_structures()
    assert all(TC.synthetic_twin(cx, xh[k], region)['n_borderline'] == 0 for k in range(2))
    c = RC.load_complex('6ct7', 'h3')
    m = c['mask'].clone()
    m[int(torch.nonzero(c['mov'])[1, 0]), 1] = False
    assert TC.twin(c, c['x'], mask=m)['n_borderline'] == 0
    cx, xh, _, _, _ = AG.l352_designs(device=None)
    assert TC.synthetic_twin(cx, xh[57], cx['cdr_def'] == 5)['n_borderline'] == 0


def test_borderline_decisions_are_counted():
    """A chain whose atoms all lie in one plane has y == 0 exactly for every dihedral: each sign test on it is borderline, and the twin
    says so instead of deciding silently."""
    from abx_amd import torsions
    x = np.zeros((3, 14, 3))
    for i in range(3):
        x[i, 0], x[i, 1], x[i, 2] = (3.8 * i, 0.0, 0.0), (3.8 * i + 1.2, 0.8, 0.0), (3.8 * i + 2.5, 0.0, 0.0)
    mask = np.zeros((3, 14), bool)
    mask[:, :3] = True
    c = TC.chain_complex(dict(x=x, mask=mask))
    h = TC.twin(c, c['x'])
    assert h['classes'][1] != 0 and h['n_borderline'] >= 2                            # the sign of phi of residue 1, in the wild type and in the design
    b = torsions._Borderline()
    b(np.array([1.0, 1.0 + 1e-12, 2.0]), np.array([1.0, 1.0, 1.0]), np.array([1.0, 1.0, 1.0]), np.array([True, True, True]))
    assert b.n == 2


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
    """ANALYSES keeps its order: --patches stays in front of --torsions, which is walked after the first nine."""
    from abx_amd import analyses, torsions
    before = analyses.ANALYSES[:9]
    further = [an.flag for an in analyses.ANALYSES[9:]]
    assert [an.flag for an in analyses.ANALYSES] == ['score', 'relax', 'interface', 'confidence', 'accuracy', 'polar', 'ensemble', 'developability', 'shape', 'patches', 'torsions', 'secondary']
    assert [an.flag for an in before] == ['score', 'relax', 'interface', 'confidence', 'accuracy', 'polar', 'ensemble', 'developability', 'shape']
    assert further[0] == 'patches' and 'torsions' in further and analyses.TORSIONS.kw == 'torsions' and analyses.TORSIONS.extra == 'torsions_rows'
    assert 'torsions' not in [an.flag for an in before]
    a = parser().parse_args([])
    assert a.torsions is False and a.torsions_rows is False and a.torsions_chi_tol == 40.0
    assert analyses.check_options(a, False) == []
    a = parser().parse_args(['--torsions'] + ['--' + an.flag for an in before])
    active = [an.flag for an in analyses.check_options(a, True)]
    assert active[:len(before)] == [an.flag for an in before] and 'torsions' in active[len(before):]
    a = parser().parse_args(['--torsions', '--torsions_rows', '--torsions_chi_tol', '30'])
    assert [an.flag for an in analyses.check_options(a, False)] == ['torsions']
    NT = len(torsions.TORSIONS_COLUMNS)
    shapes = lambda a: {f.name: (f.dtype, f.shape, f.rows) for f in analyses.fields_of(analyses.check_options(a, False), a)}
    assert shapes(a) == {'seq': (torch.int64, ('Lab',), True), 'pLDDT': (torch.float32, ('Lab',), False), 'torsions': (torch.float64, (2 * NT,), True),
                         'torsions_abego': (torch.int32, (3, 'Lab'), True), 'torsions_rows': (torch.float64, ('Lab', 8), False)}
    a = parser().parse_args(['--torsions', '--relax'])
    assert shapes(a)['torsions'] == (torch.float64, (3 * NT,), True) and 'torsions_rows' not in shapes(a)


@pytest.mark.parametrize('argv, set_level, text', [
    (['--torsions_rows'], False, '--torsions_rows needs --torsions'),
    (['--torsions', '--torsions_rows'], True, '--torsions_rows needs the sample-sharded schedule (--shard_samples): a set-level run gathers one table only'),
    (['--torsions', '--torsions_chi_tol', '0'], False, '--torsions_chi_tol must be in (0, 180] degrees'),
    (['--torsions', '--torsions_chi_tol', '-5'], False, '--torsions_chi_tol must be in (0, 180] degrees'),
    (['--torsions', '--torsions_chi_tol', '180.5'], False, '--torsions_chi_tol must be in (0, 180] degrees'),
    (['--torsions', '--torsions_chi_tol', 'nan'], False, '--torsions_chi_tol must be in (0, 180] degrees'),
])
def test_option_checks_exit_by_name(argv, set_level, text):
    from abx_amd import analyses
    with pytest.raises(SystemExit) as e:
        analyses.check_options(parser().parse_args(argv), set_level)
    assert e.value.code == text


class Scorer:
    """A TorsionScorer as analyses.collect sees one: a wild row with its codes, the region and Lab."""

    def __init__(self, Lab, L, wild_codes):
        self.Lab, self.codes = Lab, torch.tensor(wild_codes, dtype=torch.int32)
        self.region = torch.zeros(L, dtype=torch.uint8)
        self.region[2:5] = 1

    def new_classes(self, B):
        return torch.zeros(B, self.Lab, dtype=torch.int32)

    def wild(self, classes=None):
        classes[0] = self.codes
        return torch.full((1, 25), 0.5, dtype=torch.float64)


@pytest.mark.parametrize('relax', [False, True])
def test_fields_round_trip_and_table(tmp_path, relax):
    """The filled block and the zero-row block have the same fields; RowLayout carries the codes through a set-level row (a wider
    layout than the job's Lab); the writer puts the header, the `wild` line and the `abego` column."""
    from abx_amd import analyses, design, torsions
    L, Lab, n, NT = 9, 7, 2, 25
    a = parser().parse_args(['--torsions'] + (['--relax'] if relax else ['--torsions_rows']))
    active = [an for an in analyses.check_options(a, set_level=False) if an.flag == 'torsions']
    g = torch.Generator().manual_seed(3)
    table = lambda: (torch.rand(n, NT, generator=g, dtype=torch.float64) * 50).round()
    rec = {'seq': torch.randint(0, 20, (n, Lab), generator=g), 'pLDDT': torch.full((n, Lab), 70.0), 'torsions': table(), 'torsions_relaxed': table(),
           'torsions_classes': torch.tensor([[0, 1, 2, 3, 4, 5, 0], [0, 2, 2, 0, 1, 1, 0]], dtype=torch.int32),
           'torsions_rows': torch.rand(n, Lab, 8, generator=g, dtype=torch.float64)}
    sc = Scorer(Lab, L, [0, 1, 1, 5, 2, 2, 0])
    filled = analyses.collect(active, a, [rec], {'torsions': sc})
    zero = analyses.zero_rows(active, a, L, Lab, 'cpu')
    assert list(filled) == list(zero) == [f.name for f in analyses.fields_of(active, a)]
    assert list(filled)[2:] == ['torsions', 'torsions_abego'] + ([] if relax else ['torsions_rows'])
    for k in filled:
        assert filled[k].dtype == zero[k].dtype and filled[k].shape[1:] == zero[k].shape[1:] and filled[k].shape[0] == n and zero[k].shape[0] == 0, k
    assert filled['torsions'].shape == (n, (3 if relax else 2) * NT) and bool((filled['torsions'][:, -NT:] == 0.5).all())
    assert torch.equal(filled['torsions'][:, :NT], rec['torsions']) and filled['torsions_abego'].shape == (n, 3, Lab)
    assert torch.equal(filled['torsions_abego'][:, 0], rec['torsions_classes']) and filled['torsions_abego'][1, 1].tolist() == [0, 1, 1, 5, 2, 2, 0]
    assert filled['torsions_abego'][0, 2].tolist() == [0, 0, 1, 1, 1, 0, 0]
    # through the rows of a set-level run
    rows_fields = [f for f in analyses.fields_of(active, a) if f.rows]
    layout = analyses.RowLayout(rows_fields, maxLab=Lab + 4)
    ids, F = layout.unpack(layout.pack(3, [11, 10], filled))
    assert ids == [10, 11] and torch.equal(F['torsions_abego'], filled['torsions_abego'].flip(0)) and F['torsions_abego'].dtype == torch.int32
    assert torch.equal(F['torsions'], filled['torsions'].flip(0)) and torch.equal(F['seq'], rec['seq'].flip(0))
    # the table
    files = active[0].write(a, str(tmp_path), 'x_H_L_A', [0, 1], filled, None)
    assert [f.rsplit('/', 1)[1] for f in files] == ['x_H_L_A_torsions.tsv'] + ([] if relax else ['x_H_L_A_torsions_rows.npy'])
    lines = [ln.split('\t') for ln in open(files[0]).read().splitlines()]
    ND = len(torsions.DELTA_COLUMNS)
    head = ['sample'] + list(torsions.TORSIONS_COLUMNS) + ['delta_' + c for c in torsions.DELTA_COLUMNS]
    assert lines[0] == head + ([c + '_relaxed' for c in torsions.TORSIONS_COLUMNS] if relax else []) + ['abego'] and len(lines) == 4
    wild = [0.5] * NT
    assert lines[1] == ['wild'] + torsions.format_torsions(wild) + torsions.format_delta(wild, wild) + (['nan'] * NT if relax else []) + ['AOB']
    assert lines[2][0] == '0' and lines[2][1:1 + NT] == torsions.format_torsions(rec['torsions'][0].tolist()) and lines[2][-1] == 'BGE' and lines[3][-1] == 'B-A'
    assert lines[2][1 + NT:1 + NT + ND] == torsions.format_delta(rec['torsions'][0].tolist(), wild)
    if relax:
        assert lines[3][1 + NT + ND:-1] == torsions.format_torsions(rec['torsions_relaxed'][1].tolist())
    else:
        assert np.array_equal(np.load(files[1]), rec['torsions_rows'].numpy())
    # the writer under the name design exports; no strings: '-'
    path = design._write_torsions(str(tmp_path), 'y_H_L_A', wild, [(5, rec['torsions'][0].tolist() + wild)], False)
    assert open(path).read().splitlines()[2].split('\t')[-1] == '-'


def test_format():
    from abx_amd import torsions
    row = [219, 0, 0, 2, 5, 0, 2, 7, 1, 0, 3, 1, 0, 0, 4, 4, 20.328, 24.977, 18.4686, 72.9975, 3, 3, 1, 0, float('nan')]
    assert torsions.format_torsions(row) == ['219', '0', '0', '2', '5', '0', '2', '7', '1', '0', '3', '1', '0', '0', '4', '4', '20.33', '24.98', '18.47',
                                             '73.00', '3', '3', '1', '0', 'nan']
    wild = [219, 0, 0, 0, 5, 0, 0, 7, 1, 0, 3, 1, 0, 0, 4, 4, 0, 0, 0, 0, 3, 3, 1, 1, 0]
    assert torsions.format_delta(row, wild) == ['+0', '+0', '+2', '+0', '+2', '+0', '+0', '+0', '+0', '+0', '+0', '+0']


def test_sampler_signature_defaults_to_no_torsions():
    import inspect
    from abx_amd import sampler
    assert inspect.signature(sampler.sample_fn).parameters['torsions'].default is None
