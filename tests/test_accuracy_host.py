"""CPU-only checks of the accuracy analysis (abx_accuracy_scores, abx_amd.accuracy): the float64 host twin against vectors of the
reference's lddt / lddt_ca_torch / TMscoreHead loop, hand-checkable cases, the borderline condition under which the GPU test may ask
for equal integers, the C layout of the descriptor, argument checks without a GPU, and the formats of the design driver."""
import ctypes
import os

import numpy as np
import pytest
import torch

import host_cases as HC
import accuracy_cases as AC
import relax_cases as RC
from conftest import load_npz



def col(name):
    from abx_amd import accuracy
    return accuracy.ACCURACY_COLUMNS.index(name)


@pytest.fixture(scope='module')
def lib():
    return HC.load_lib()


def test_host_twin_against_the_reference_vectors():
    """Class `ca` of the twin is upstream's lddt on the C-alpha (per residue and pair-pooled) and lddt_ca_torch, its TM block is
    TMscoreHead's Kabsch -> TMscore with GDT TS / HA and RMSD of the same aligned sets: to 1e-4, the project's parity bound for fp32
    reference values.  Rows without pairs: the twin says nan where upstream's eps / eps gives 1 and lddt_ca_torch 0 / 0."""
    from abx_amd import accuracy
    g = load_npz('accuracy.npz')
    true, exists, seq = g['true'], g['exists'], g['seq']
    N = true.shape[0]
    worst = 0.0
    for key in g['cases']:
        h = accuracy.accuracy_host(g[f'{key}.pred'], exists, seq, true, exists, seq, N, radius=float(g['radius']))
        assert h['n_borderline'] == 0 and h['n_borderline_gdt'] == 0
        ca, has = h['rows'][:, 2], h['counts'][:, 2, 0] > 0
        assert has.sum() >= 30 and not has[17] and not has[3] and not has[9] and np.isnan(ca[~has]).all()
        errs = dict(per_residue=np.abs(ca[has] - g[f'{key}.lddt_per_residue'][has]).max(),
                    ca_torch=np.abs(ca[has] - g[f'{key}.lddt_ca_torch'][has]).max(),
                    pooled=abs(h['row'][col('lddt_ca_all')] - float(g[f'{key}.lddt_pooled'])),
                    tm=abs(h['row'][col('tm_score')] - float(g[f'{key}.tm_score'][0])),
                    gdt_ts=abs(h['row'][col('gdt_ts')] - float(g[f'{key}.gdt_ts'][0])),
                    gdt_ha=abs(h['row'][col('gdt_ha')] - float(g[f'{key}.gdt_ha'][0])),
                    # upstream's RMSD is the root of the mean over coordinates AND points: sqrt(sum d^2 / (3 N))
                    rmsd=abs(h['row'][col('rmsd_ca')] / np.sqrt(3.0) - float(g[f'{key}.rmsd'][0])))
        print(key, {k: f'{v:.2e}' for k, v in errs.items()})
        worst = max(worst, *errs.values())
        # the isolated and the masked residues count as 1 in upstream's per-residue form (eps / eps)
        assert np.all(g[f'{key}.lddt_per_residue'][~has] == 1.0)
    print(f'largest difference to the reference vectors: {worst:.3e}')
    assert worst <= 1e-4
    assert 0.8 < float(g['c0.lddt_pooled']) < 0.95 and 0.4 < float(g['c1.lddt_pooled']) < 0.6      # non-trivial cases


@pytest.fixture(scope='module')
def small():
    """The 40-residue fixture as a complex of 30 antibody and 10 antigen rows (the far residue 17 moved back so that the hand cases
    see an ordinary chain), and its row against itself."""
    g = load_npz('accuracy.npz')
    x = torch.from_numpy(g['true']).double()
    x[17] -= 80.0
    x = x.float().double()
    c = dict(x=x, mask=torch.from_numpy(g['exists']).clone(), aa=torch.from_numpy(g['seq']).clone(), Lab=30)
    c['mask'][[3, 22, 23]] = True
    c['mask'][9, 1] = True
    typed = typed_mask(c['aa'])
    c['mask'] &= typed
    c['mov'] = torch.zeros(40, dtype=torch.bool)
    c['mov'][8:14] = True
    return c, AC.host(c, c['x'])


def typed_mask(aa):
    from abx_amd import residue_constants as rc
    return torch.as_tensor(rc.restype_atom14_mask)[aa].bool()


def test_identical_structure_and_rigid_motion(small):
    c, same = small
    L = 40
    row = same['row']
    assert row[:6].tolist() == [1.0] * 6 and row[col('tm_score')] == 1.0 and row[col('gdt_ts')] == 1.0 == row[col('gdt_ha')]
    assert row[col('rmsd_ca')] <= 1e-12 and np.isnan(row[col('plddt_region')]) and np.isnan(row[col('plddt_err_region')])
    assert row[col('n_native')] == row[col('n_kept')] > 0 and row[col('fnat')] == 1.0 and row[col('n_new')] == 0
    assert row[col('n_atoms_scored')] == int(c['mask'].sum()) and same['contacts'].shape == (30, 10)
    assert set(np.unique(same['contacts']).tolist()) == {0, 3}
    assert (same['counts'][:, :, 1:] == same['counts'][:, :, :1]).all() and (same['counts'][:, 0, 0] > 0).all()
    assert (same['counts'][:, 2, 0] <= same['counts'][:, 1, 0]).all() and (same['counts'][:, 1, 0] <= same['counts'][:, 0, 0]).all()
    # a rigid motion of the whole complex: every distance survives float32 rounding to ~1e-5 A
    R, t = AC.rigid(4)
    moved = torch.from_numpy(c['x'].numpy() @ R.T + t).float().double()
    h = AC.host(c, moved)
    assert np.array_equal(h['counts'], same['counts']) and np.array_equal(h['contacts'], same['contacts'])
    assert h['row'][:6].tolist() == [1.0] * 6 and h['row'][col('rmsd_ca')] < 1e-4 and h['row'][col('gdt_ha')] == 1.0
    assert abs(h['row'][col('tm_score')] - 1.0) < 1e-8
    # plddt: the mean over the region and the error against 100 * lDDT-ca (1 everywhere here)
    pl = torch.linspace(50.0, 89.0, L)
    h = AC.host(c, c['x'], plddt=pl)
    assert abs(h['row'][col('plddt_region')] - float(pl[8:14].double().mean())) < 1e-12
    assert abs(h['row'][col('plddt_err_region')] - float((100.0 - pl[8:14].double()).mean())) < 1e-12


def test_moving_one_residue_touches_only_its_pairs(small):
    c, same = small
    i = 10
    x = c['x'].clone()
    x[i] += torch.tensor([3.0, 0.0, 0.0], dtype=torch.float64)
    h = AC.host(c, x)
    # 3 A < 4 A: every pair is still preserved at the last threshold, the pair sets are the wild type's
    assert np.array_equal(h['counts'][:, :, 0], same['counts'][:, :, 0]) and np.array_equal(h['counts'][:, :, 4], same['counts'][:, :, 0])
    assert h['counts'][i, 0, 1] < same['counts'][i, 0, 1] and h['row'][col('lddt_region')] < 1.0
    # no row gains, and the rows beyond the radius of every atom of residue i lose nothing
    lost = same['counts'][:, 0, 1] - h['counts'][:, 0, 1]
    d_ca = (c['x'][:, 1] - c['x'][i, 1]).norm(dim=1).numpy()
    assert (lost >= 0).all() and (lost[d_ca > 15.0 + 12.0] == 0).all()
    n_i = int(c['mask'][i].sum())
    # without residue i (res_mask) nothing is left of the move
    keep = torch.ones(40, dtype=torch.bool)
    keep[i] = False
    a, b = AC.host(c, x, res_mask=keep), AC.host(c, c['x'], res_mask=keep)
    assert np.array_equal(a['counts'], b['counts']) and np.array_equal(a['contacts'], b['contacts'])
    assert a['row'][:6].tolist() == [1.0] * 6 and a['row'][col('n_atoms_scored')] == same['row'][col('n_atoms_scored')] - n_i
    # res_mask = the row absent from both structures
    cut = c['mask'].clone()
    cut[i] = False
    from abx_amd import accuracy
    region = c['mov'].clone()
    region[i] = False
    d = accuracy.accuracy_host(x, cut, c['aa'], c['x'], cut, c['aa'], c['Lab'], region=region)
    assert np.array_equal(a['counts'], d['counts']) and np.array_equal(a['row'], d['row'], equal_nan=True) and not a['counts'][i].any()


def test_a_mutated_residue_is_compared_on_backbone_and_cb(small):
    c, same = small
    LEU, ALA = 10, 0
    i = next(k for k in range(8, 14) if int(c['aa'][k]) not in (AC.GLY, ALA, LEU) and int(c['mask'][k].sum()) > 5)
    aa = c['aa'].clone()
    aa[i] = LEU
    mask = c['mask'].clone()
    mask[i] = typed_mask(aa)[i]
    x = c['x'].clone()
    x[i, 5:] = x[i, 1] + 1.0                                      # wherever the new side chain is: it is not scored
    h = AC.host(c, x, aa, mask)
    beyond_cb = int(c['mask'][i, 5:].sum())
    assert h['row'][col('n_atoms_scored')] == same['row'][col('n_atoms_scored')] - beyond_cb
    # the same counts as the unmutated residue cut to its first five slots
    cut = c['mask'].clone()
    cut[i, 5:] = False
    k = AC.host(c, c['x'], mask=cut)
    assert np.array_equal(h['counts'], k['counts']) and (h['counts'][:, :, 1:] == h['counts'][:, :, :1]).all()
    assert np.array_equal(h['counts'][:, 1:], same['counts'][:, 1:])            # classes bb and ca do not see the side chain
    assert h['counts'][i, 0, 0] < same['counts'][i, 0, 0]
    # Gly <-> Ala at a designed row: the CB exists in one of the two structures only, four atoms are scored
    gly = next(k for k in range(40) if int(c['aa'][k]) == AC.GLY)
    aa2, m2 = c['aa'].clone(), c['mask'].clone()
    aa2[gly] = ALA
    m2[gly] = typed_mask(aa2)[gly]
    x2 = c['x'].clone()
    x2[gly, 4] = x2[gly, 1] + 1.5
    g2 = AC.host(c, x2, aa2, m2, region=np.arange(40) == gly)
    assert g2['row'][col('n_atoms_scored')] == same['row'][col('n_atoms_scored')] and np.array_equal(g2['counts'], same['counts'])
    aa3, m3 = c['aa'].clone(), c['mask'].clone()
    ala = next(k for k in range(40) if int(c['mask'][k].sum()) >= 5 and int(c['aa'][k]) != AC.GLY)
    aa3[ala] = AC.GLY
    m3[ala] = typed_mask(aa3)[ala]
    g3 = AC.host(c, c['x'], aa3, m3)
    assert g3['row'][col('n_atoms_scored')] == same['row'][col('n_atoms_scored')] - int(c['mask'][ala, 4:].sum())
    assert np.array_equal(g3['counts'][:, 2], same['counts'][:, 2]) and g3['counts'][ala, 1, 0] < same['counts'][ala, 1, 0]


def test_no_antigen_and_no_region(small):
    c, same = small
    from abx_amd import accuracy
    h = accuracy.accuracy_host(c['x'], c['mask'], c['aa'], c['x'], c['mask'], c['aa'], 40, region=c['mov'])
    r = h['row']
    assert h['contacts'].shape == (40, 0) and r[col('n_native')] == r[col('n_kept')] == r[col('n_new')] == r[col('n_native_region')] == 0
    assert np.isnan(r[col('fnat')]) and np.isnan(r[col('fnat_region')]) and np.array_equal(h['counts'], same['counts'])
    assert np.array_equal(r[:12], same['row'][:12], equal_nan=True)
    e = AC.host(c, c['x'], region=None)
    e2 = AC.host(c, c['x'], region=np.zeros(40, bool))
    assert np.array_equal(e['row'], e2['row'], equal_nan=True)
    reg_cols = [col(n) for n in ('lddt_region', 'lddt_bb_region', 'lddt_ca_region', 'plddt_region', 'plddt_err_region', 'fnat_region')]
    zero_cols = [col(n) for n in ('n_native_region', 'n_kept_region', 'n_pairs_region')]
    assert np.isnan(e['row'][reg_cols]).all() and (e['row'][zero_cols] == 0).all()
    others = [k for k in range(21) if k not in reg_cols + zero_cols]
    assert np.array_equal(e['row'][others], same['row'][others], equal_nan=True)
    assert same['row'][col('n_pairs_region')] == same['counts'][8:14, 0, 0].sum() > 0


@pytest.mark.parametrize('code,sel', RC.MOVABLE_SETS)
def test_no_borderline_decision_on_the_gpu_test_structures(code, sel):
    """The structures tests/test_gpu_accuracy.py compares exactly - MOVABLE_SETS x SEEDS and their mutated versions - hold no pair
    within 1e-9 of a threshold and no C-alpha within 1e-6 A of a GDT cutoff, and their values are not trivial."""
    from abx_amd import accuracy
    c = RC.load_complex(code, sel)
    wild = AC.host(c, c['x'])
    assert wild['n_borderline'] == 0 and wild['row'][col('n_native')] == {'6ct7': 51, '6qd7': 3}[code]
    if (code, sel) == ('6ct7', 'h3'):
        assert wild['row'][col('n_native_region')] == 9
    for seed in RC.SEEDS:
        x = RC.perturb(c, seed)
        xm, aa, m = AC.mutate(c, x, seed)
        assert (aa[c['mov']] == AC.GLY).any() and int((aa != c['aa']).sum()) >= 2 and not (aa != c['aa'])[~c['mov']].any()
        for what, h in (('perturbed', AC.host(c, x)), ('mutated', AC.host(c, xm, aa, m))):
            r = dict(zip(accuracy.ACCURACY_COLUMNS, h['row'].tolist()))
            print(code, sel, seed, what, {k: round(v, 4) for k, v in r.items()})
            assert h['n_borderline'] == 0 and h['n_borderline_gdt'] == 0, (code, sel, seed, what)
            assert 0.7 < r['lddt_region'] < 0.9 and 0.9 < r['lddt_all'] < 1.0 and r['lddt_region'] < r['lddt_all']
            assert r['n_native'] == wild['row'][col('n_native')] and 0 < r['n_kept'] <= r['n_native']
            if code == '6ct7':
                assert 48 <= r['n_kept'] <= 50


def test_accuracy_args_match_c_layout():
    """sizeof / offsetof of AbxAccuracyArgs as gcc lays it out, and ABX_ACC_COLS against the Python side."""
    from abx_amd import _lib, accuracy
    st = _lib.AbxAccuracyArgs
    c_layout = HC.assert_c_layout({'AbxAccuracyArgs': st}, ['ABX_ACC_COLS'])
    assert c_layout['ABX_ACC_COLS'] == _lib.ACC_COLS == len(accuracy.ACCURACY_COLUMNS) == 21
    assert accuracy.ACCURACY_COLUMNS[:6] == ('lddt_all', 'lddt_antibody', 'lddt_region', 'lddt_bb_region', 'lddt_ca_all', 'lddt_ca_region')
    assert accuracy.ACCURACY_COLUMNS[6:12] == ('plddt_region', 'plddt_err_region', 'tm_score', 'gdt_ts', 'gdt_ha', 'rmsd_ca')
    assert accuracy.ACCURACY_COLUMNS[12:] == ('n_native', 'n_kept', 'fnat', 'n_new', 'n_native_region', 'n_kept_region', 'fnat_region',
                                              'n_pairs_region', 'n_atoms_scored')
    assert set(accuracy.COUNT_COLUMNS) == {c for c in accuracy.ACCURACY_COLUMNS if c.startswith('n_')}
    assert set(accuracy.DELTA_COLUMNS) <= set(accuracy.ACCURACY_COLUMNS) and accuracy.ROW_COLUMNS == ('lddt_all', 'lddt_bb', 'lddt_ca', 'n_pairs')


def test_accuracy_argument_checks_without_gpu(lib):
    """Every malformed descriptor comes back negative before any launch, with the entry's name in the error string."""
    from abx_amd._lib import AbxAccuracyArgs
    P = 0x1000                                      # any non-null "device pointer": nothing is dereferenced

    def good():
        a = AbxAccuracyArgs()
        a.pred_atom14 = a.pred_seq = a.gt_atom14 = a.gt_exists = a.gt_seq = a.radius = a.out = P
        a.B, a.L, a.Lab, a.Lpred = 4, 40, 30, 30
        a.pred_sb, a.pred_seq_sb, a.out_stride = 30 * 42, 30, 21
        a.lddt_radius, a.contact = 15.0, 5.0
        return a

    def bad(a, ws=P):
        rc = lib.abx_accuracy_scores(ctypes.byref(a) if a is not None else None, ws, None)
        msg = lib.abx_last_error_string()
        assert rc < 0 and b'abx_accuracy_scores' in msg, (rc, msg)

    assert lib.abx_accuracy_scores_workspace_bytes(4, 40) >= 4 * 40 * 18 * 4
    assert lib.abx_accuracy_scores_workspace_bytes(0, 40) == lib.abx_accuracy_scores_workspace_bytes(4, -1) == 0
    assert lib.abx_accuracy_scores_workspace_bytes(100, 352) < 4 << 20
    bad(None)
    bad(AbxAccuracyArgs())
    for field in ('pred_atom14', 'pred_seq', 'gt_atom14', 'gt_exists', 'gt_seq', 'radius', 'out'):
        a = good()
        setattr(a, field, None)
        bad(a)
    for field, v in (('B', 0), ('B', -3), ('B', 65536), ('L', 0), ('L', -1), ('Lab', 41), ('Lab', 0), ('Lpred', 29), ('Lpred', 31), ('Lpred', 41),
                     ('out_stride', 20), ('lddt_radius', 0.0), ('lddt_radius', -15.0), ('lddt_radius', float('nan')), ('lddt_radius', float('inf')),
                     ('contact', 0.0), ('contact', -5.0), ('contact', float('nan'))):
        a = good()
        setattr(a, field, v)
        bad(a)
    bad(good(), ws=None)


def test_driver_formats(tmp_path):
    from abx_amd import accuracy, design
    NA = len(accuracy.ACCURACY_COLUMNS)
    nan = float('nan')
    wild = [1.0] * 6 + [nan, nan, 1.0, 1.0, 1.0, 0.0, 51.0, 51.0, 1.0, 0.0, 9.0, 9.0, 1.0, 16882.0, 1741.0]
    assert accuracy.format_accuracy(wild) == ['1.0000'] * 6 + ['nan', 'nan', '1.0000', '1.0000', '1.0000', '0.000', '51', '51', '1.0000', '0', '9', '9',
                                              '1.0000', '16882', '1741']
    d0 = [0.98794, 0.98811, 0.74851, 0.7857, 0.98992, 0.81659, 71.237, 10.4249, 0.99923, 0.99676, 0.99243, 0.16624, 51.0, 48.0, 48 / 51, 1.0,
          9.0, 6.0, 6 / 9, 16882.0, 1741.0]
    d1 = list(d0)
    d1[2], d1[3], d1[11], d1[13] = 0.76, 0.7857, 0.2, 50.0
    assert accuracy.format_accuracy(d0) == ['0.9879', '0.9881', '0.7485', '0.7857', '0.9899', '0.8166', '71.24', '10.42', '0.9992', '0.9968', '0.9924',
                                            '0.166', '51', '48', '0.9412', '1', '9', '6', '0.6667', '16882', '1741']
    assert accuracy.format_delta(d1, d0) == ['+0.0115', '+0.0000', '+0.034', '+2']
    path = design._write_accuracy(str(tmp_path), '6ct7_H_L_S', wild, [(0, d0), (1, d1)], False)
    assert os.path.basename(path) == '6ct7_H_L_S_accuracy.tsv'
    lines = [ln.split('\t') for ln in open(path).read().splitlines()]
    assert lines[0] == ['sample'] + list(accuracy.ACCURACY_COLUMNS) and len(lines) == 4
    assert lines[1] == ['wild'] + accuracy.format_accuracy(wild)
    assert lines[2] == ['0'] + accuracy.format_accuracy(d0) and lines[3] == ['1'] + accuracy.format_accuracy(d1)
    # with --relax: the relaxed structure's columns follow, suffixed _relaxed, then relaxed minus design; the wild type has none
    path = design._write_accuracy(str(tmp_path), 'x_H_L_A', wild, [(5, d0 + d1)], True)
    lines = [ln.split('\t') for ln in open(path).read().splitlines()]
    assert lines[0][1 + NA:] == [c + '_relaxed' for c in accuracy.ACCURACY_COLUMNS] + ['delta_' + c for c in accuracy.DELTA_COLUMNS] and len(lines) == 3
    assert lines[1][0] == 'wild' and lines[1][1 + NA:] == ['nan'] * (NA + len(accuracy.DELTA_COLUMNS))
    assert lines[2] == ['5'] + accuracy.format_accuracy(d0) + accuracy.format_accuracy(d1) + accuracy.format_delta(d1, d0)
    ap = design.build_parser()
    a = ap.parse_args([])
    assert a.accuracy is False and a.accuracy_rows is False and (a.accuracy_radius, a.accuracy_contact) == (15.0, 5.0)
    a = ap.parse_args(['--accuracy', '--accuracy_radius', '12', '--accuracy_contact', '4.5', '--accuracy_rows'])
    assert a.accuracy is True and a.accuracy_rows is True and (a.accuracy_radius, a.accuracy_contact) == (12.0, 4.5)


def test_sampler_signature_defaults_to_no_accuracy():
    import inspect
    from abx_amd import sampler
    assert inspect.signature(sampler.sample_fn).parameters['accuracy'].default is None
