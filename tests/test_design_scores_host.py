"""CPU-only checks of the design scores (abx_design_scores, abx_amd.metrics.DesignScorer): C layout of the descriptor, argument checks
without a GPU, the column names, the TSV formats of the design driver, and the host twin of the violation counts against the
reference's masks (tests/golden/vio_pdb.npz)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import host_cases as HC
from conftest import load_npz, tt



@pytest.fixture(scope='module')
def lib():
    return HC.load_lib()


def test_design_score_args_match_c_layout():
    """sizeof / offsetof of AbxDesignScoreArgs as gcc lays it out (the method of test_host_cpu.py::test_ctypes_structs_match_c_layout,
    whose struct list is fixed) and ABX_SCORE_COLS against the Python side."""
    from abx_amd import _lib, metrics
    st = _lib.AbxDesignScoreArgs
    c_layout = HC.assert_c_layout({'AbxDesignScoreArgs': st}, ['ABX_SCORE_COLS'])
    assert c_layout['ABX_SCORE_COLS'] == _lib.SCORE_COLS == len(metrics.SCORE_COLUMNS)


def test_design_scores_argument_checks_without_gpu(lib):
    """Every malformed descriptor comes back negative before any launch, with the entry's name in the error string."""
    from abx_amd._lib import AbxDesignScoreArgs
    P = 0x1000                                      # any non-null "device pointer": nothing is dereferenced

    def good():
        a = AbxDesignScoreArgs()
        a.pred_atom14 = a.pred_seq = a.gt_atom14 = a.gt_exists = a.gt_seq = a.cdr_def = a.chain_id = a.radius = a.out = P
        a.B, a.L, a.Lab, a.Lpred = 4, 40, 30, 30
        a.pred_sb, a.pred_seq_sb, a.out_stride = 30 * 42, 30, 19
        return a

    def bad(a, ws=P):
        rc = lib.abx_design_scores(ctypes.byref(a) if a is not None else None, ws, None)
        msg = lib.abx_last_error_string()
        assert rc < 0 and b'abx_design_scores' in msg, (rc, msg)

    assert lib.abx_design_scores_workspace_bytes(4, 40) > 0
    assert lib.abx_design_scores_workspace_bytes(100, 352) == 100 * 22 * 16
    bad(None)
    bad(AbxDesignScoreArgs())
    for field in ('pred_atom14', 'pred_seq', 'gt_atom14', 'gt_exists', 'gt_seq', 'cdr_def', 'chain_id', 'radius', 'out'):
        a = good()
        setattr(a, field, None)
        bad(a)
    for field, v in (('B', 0), ('B', -3), ('L', 0), ('L', -1), ('L', 1), ('Lab', 41), ('Lab', 0), ('Lpred', 29), ('Lpred', 41), ('out_stride', 18)):
        a = good()
        setattr(a, field, v)
        bad(a)
    bad(good(), ws=None)                            # the queried workspace size is non-zero: a null workspace is an error


def test_score_columns_start_with_the_calc_ab_metrics_keys():
    from abx_amd import metrics
    names = [str(k) for k in load_npz('metrics_6qd7.npz')['c1.names']]
    assert len(names) == 14
    for mine, ref in zip(metrics.SCORE_COLUMNS[:14], names):
        assert mine == ref
    assert metrics.SCORE_COLUMNS[14:] == ('n_viol_c_n', 'n_viol_ca_c_n', 'n_viol_c_n_ca', 'n_clash', 'n_clash_inter')


def test_write_designs_formats(tmp_path):
    """Without scores: today's three columns, byte for byte.  With scores: header and rows parse back to the values given."""
    from abx_amd import design, metrics
    rows = [(0, 71.23456, [0, 1, 2, 3, 19]), (7, 5.0, [4, 4, 14])]
    path = design._write_designs(str(tmp_path), '6ct7_H_L_S', rows)
    assert os.path.basename(path) == '6ct7_H_L_S_designs.tsv'
    assert open(path, 'rb').read() == b'sample\tmean_pLDDT\tantibody_sequence\n0\t71.235\tARNDV\n7\t5.000\tCCP\n'
    sc = [0.5, 1.23456789, 1.0, 0.0, 0.25, float('nan'), 12.5, float('nan'), 0.0, 3.00004, 1.0, 2.5, 0.125, 0.99996, 3.0, 0.0, 17.0, 1234567.0, 12.0]
    path = design._write_designs(str(tmp_path), 'x_H_L_A', [(3, 50.0, [0, 1], sc)])
    head, line = open(path).read().splitlines()
    assert head.split('\t') == ['sample', 'mean_pLDDT', 'antibody_sequence'] + list(metrics.SCORE_COLUMNS)
    f = line.split('\t')
    assert f[:3] == ['3', '50.000', 'AR'] and len(f) == 3 + len(metrics.SCORE_COLUMNS)
    for name, txt, v in zip(metrics.SCORE_COLUMNS, f[3:], sc):
        if name.startswith('n_'):
            assert txt == str(int(v))
        elif v != v:
            assert txt == 'nan'
        else:
            assert '.' in txt and len(txt.split('.')[1]) == 4 and abs(float(txt) - v) <= 0.5e-4 + 1e-12
    table = torch.tensor([[[0.5] + sc, [0.01] + sc]], dtype=torch.float64)
    lines = open(design._write_trajectory_scores(str(tmp_path), 'x_H_L_A', table)).read().splitlines()
    assert lines[0].split('\t') == ['sample', 'step', 't'] + list(metrics.SCORE_COLUMNS) and len(lines) == 3
    assert lines[2].split('\t')[:3] == ['0', '1', '0.0100'] and lines[2].split('\t')[3:] == f[3:]


def test_violation_counts_equal_the_reference_mask_sums():
    """metrics.violation_counts on every case of vio_pdb.npz: the sums of the reference's three violation masks, exactly (no residue
    pair of these cases lies within 2.5e-4 A / 9e-4 of a threshold: three orders above fp32 rounding)."""
    from abx_amd import metrics
    z = load_npz('vio_pdb.npz')
    total = 0
    for c in z['cases']:
        p = load_npz(f'pdb_{str(c).split(".")[0]}.npz')
        got = metrics.violation_counts(tt(z[f'{c}.pos']), tt(p['batch.atom14_gt_exists']), tt(p['batch.seq']), tt(p['batch.chain_id']))
        want = [int(z[f'{c}.{k}'].sum()) for k in ('c_n_violation_mask', 'ca_c_n_violation_mask', 'c_n_ca_violation_mask')]
        assert got.tolist() == [want], (c, got.tolist(), want)
        total += sum(want)
    assert total == 1056
    p = load_npz('pdb_6qd7.npz')
    args = (tt(z['6qd7.s0.pos']), tt(p['batch.atom14_gt_exists']), tt(p['batch.seq']), tt(p['batch.chain_id']))
    assert metrics.violation_counts(*args)[0, 0] == 1 and metrics.violation_counts(*args, residx=tt(p['batch.residx']))[0, 0] == 0


def test_clash_counts_host_twin():
    """metrics.clash_counts: two residues 100 A apart do not clash; overlapping ones do, across chains when the chain ids differ; the
    peptide bond of linked neighbours and SG-SG are not counted."""
    from abx_amd import metrics, residue_constants as rc
    aa = torch.tensor([[0, 0]])
    m = torch.as_tensor(rc.restype_atom14_mask)[aa]
    x = torch.zeros(1, 2, 14, 3)
    x[0, :, :, 0] = 3.0 * torch.arange(14.)[None]           # atoms of one residue 3 A apart along x
    x[0, 1, :, 1] = 100.0
    ch = torch.tensor([[0, 1]])
    assert [int(v) for v in metrics.clash_counts(x, m, aa, ch)] == [0, 0, 0]
    x[0, 1, :, 1] = 1.0                                     # slot k of one residue 1 A from slot k of the other: 5 atom pairs (ALA)
    assert [int(v) for v in metrics.clash_counts(x, m, aa, ch)] == [5, 5, 0]
    assert [int(v) for v in metrics.clash_counts(x, m, aa, torch.tensor([[0, 0]]))] == [5, 0, 0]
    # C (slot 2) of residue 0 on N (slot 0) of residue 1: excluded only while the two are linked
    y = x.clone()
    y[0, 1, :, 1] = 100.0
    y[0, 1, 0] = y[0, 0, 2] + torch.tensor([0., 1.3, 0.])
    same = torch.tensor([[0, 0]])
    assert int(metrics.clash_counts(y, m, aa, same)[0]) == 0 and int(metrics.clash_counts(y, m, aa, ch)[0]) == 1
    assert int(metrics.clash_counts(y, m, aa, same, residx=torch.tensor([[5, 9]]))[0]) == 1
