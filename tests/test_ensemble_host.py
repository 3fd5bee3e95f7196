"""CPU-only checks of the ensemble analysis (abx_ensemble_pairs / abx_ensemble_cluster, abx_amd.ensemble): C layout of both
descriptors, argument checks without a GPU, the float64 host twin against the pinned Kabsch route on the shipped 6qd7 antibody, the
Daura rule on hand-made graphs, the synthetic ensemble the GPU tests use, and the formats of the design driver."""
import ctypes
import os

import numpy as np
import pytest

import host_cases as HC
import ensemble_cases as EC
from conftest import load_npz



@pytest.fixture(scope='module')
def lib():
    return HC.load_lib()


def test_ensemble_args_match_c_layout():
    """sizeof / offsetof of both descriptors as gcc lays them out, and the three constants against the Python side."""
    from abx_amd import _lib, ensemble
    structs = {'AbxEnsemblePairsArgs': _lib.AbxEnsemblePairsArgs, 'AbxEnsembleClusterArgs': _lib.AbxEnsembleClusterArgs}
    c_layout = HC.assert_c_layout(structs, ['ABX_ENS_COLS', 'ABX_ENS_MAX_POINTS', 'ABX_ENS_MAX_N'])
    assert c_layout['ABX_ENS_COLS'] == _lib.ENS_COLS == len(ensemble.ENSEMBLE_COLUMNS) == 10
    assert c_layout['ABX_ENS_MAX_POINTS'] == _lib.ENS_MAX_POINTS == ensemble.MAX_POINTS == 512
    assert c_layout['ABX_ENS_MAX_N'] == _lib.ENS_MAX_N == ensemble.MAX_N == 1024
    assert set(ensemble.COUNT_COLUMNS) <= set(ensemble.ENSEMBLE_COLUMNS)


def test_ensemble_argument_checks_without_gpu(lib):
    """Every malformed descriptor comes back negative before any HIP call, with the entry's name in the error string."""
    from abx_amd._lib import AbxEnsembleClusterArgs, AbxEnsemblePairsArgs
    P = 0x1000                                      # any non-null "device pointer": nothing is dereferenced

    def pairs():
        a = AbxEnsemblePairsArgs()
        a.pred_atom14 = a.pred_seq = a.region = a.planes = P
        a.N, a.Lpred, a.M, a.atoms = 24, 30, 13, 4
        a.pred_sb, a.pred_seq_sb, a.plane_stride = 30 * 42, 30, 24 * 24
        return a

    def cluster():
        a = AbxEnsembleClusterArgs()
        a.planes = a.out = a.centres = a.n_clusters = P
        a.N, a.metric, a.cutoff, a.plane_stride, a.out_stride = 24, 0, 1.0, 24 * 24, 10
        return a

    def bad_pairs(a):
        rc = lib.abx_ensemble_pairs(ctypes.byref(a) if a is not None else None, None, None)
        msg = lib.abx_last_error_string()
        assert rc < 0 and b'abx_ensemble_pairs' in msg, (rc, msg)

    def bad_cluster(a):
        rc = lib.abx_ensemble_cluster(ctypes.byref(a) if a is not None else None, None)
        msg = lib.abx_last_error_string()
        assert rc < 0 and b'abx_ensemble_cluster' in msg, (rc, msg)

    assert lib.abx_ensemble_pairs_workspace_bytes(100, 52) >= 0
    bad_pairs(None)
    bad_pairs(AbxEnsemblePairsArgs())
    for field in ('pred_atom14', 'pred_seq', 'region', 'planes'):
        a = pairs()
        setattr(a, field, None)
        bad_pairs(a)
    # N < 1; P = 0 and P = 513 (both atom sets); atoms outside {1, 4}; fewer rows than compared residues; planes that overlap
    for field, v in (('N', 0), ('N', -2), ('M', 0), ('M', -1), ('M', 129), ('atoms', 0), ('atoms', 2), ('atoms', 3), ('atoms', 5), ('atoms', 14),
                     ('Lpred', 12), ('Lpred', 0), ('plane_stride', 24 * 24 - 1)):
        a = pairs()
        setattr(a, field, v)
        bad_pairs(a)
    a = pairs()
    a.atoms, a.M, a.Lpred = 1, 513, 600
    bad_pairs(a)
    bad_cluster(None)
    bad_cluster(AbxEnsembleClusterArgs())
    for field in ('planes', 'out', 'centres', 'n_clusters'):
        a = cluster()
        setattr(a, field, None)
        bad_cluster(a)
    for field, v in (('N', 0), ('N', -1), ('N', 1025), ('out_stride', 9), ('metric', 2), ('metric', -1), ('cutoff', -0.5), ('cutoff', float('nan')),
                     ('plane_stride', 24 * 24 - 1)):
        a = cluster()
        setattr(a, field, v)
        if field == 'N' and v > 0:
            a.plane_stride = v * v
        bad_cluster(a)


def test_twin_rmsd_fit_is_the_pinned_kabsch_route_on_6qd7():
    """ensemble_host's rmsd_fit of (ground truth, perturbed copy) on the CDR-H3 C-alpha of the 6qd7 antibody = metrics.kabsch of the
    two point sets + root mean square, the function tests/test_oracle_golden.py pins to the reference at 1e-9.  Same operations on the
    same float32-representable inputs: 1e-12 max(1, r) allows for nothing but the order of a few sums."""
    from abx_amd import ensemble, metrics
    z = load_npz('metrics_6qd7.npz')
    cases = [str(c) for c in z['cases']]
    ca = np.stack([z['gt_coord']] + [z[f'{c}.pred_coord'] for c in cases]).astype(np.float32)        # (5, 227, 3)
    N, L = ca.shape[:2]
    x = np.zeros((N, L, 14, 3), np.float32)
    x[:, :, 1] = ca
    region = z['cdr_def'] == 5
    assert 3 <= region.sum() <= 40
    seq = np.array([[ord(ch) for ch in str(z['gt_str_seq'])]] + [[ord(ch) for ch in str(z[f'{c}.pred_str_seq'])] for c in cases])
    host = ensemble.ensemble_host(x, seq, region, atoms='ca')
    assert host['planes'].shape == (3, N, N)
    for k in range(1, N):
        A, B = metrics.kabsch(ca[0, region].astype(np.float64).T, ca[k, region].astype(np.float64).T)
        r = float(np.sqrt(np.mean(np.sum(np.square(A - B), axis=0))))
        got = host['planes'][0, 0, k]
        print(f'6qd7 H3, ground truth vs {cases[k - 1]}: rmsd_fit {got:.12f} (pinned route {r:.12f}), rmsd_frame {host["planes"][1, 0, k]:.6f}')
        assert abs(got - r) <= 1e-12 * max(1.0, r) and r > 0
        assert host['planes'][0, k, 0] == got and host['planes'][1, 0, k] >= got - 1e-12
        assert host['planes'][2, 0, k] == sum(a != b for a, b in zip(np.array(list(str(z['gt_str_seq'])))[region],
                                                                       np.array(list(str(z[f'{cases[k - 1]}.pred_str_seq'])))[region]))
    assert np.array_equal(host['planes'], host['planes'].transpose(0, 2, 1)) and not host['planes'][:, np.arange(N), np.arange(N)].any()


def graph(N, edges):
    d = np.full((N, N), 9.0)
    for i, j in edges:
        d[i, j] = d[j, i] = 1.0
    np.fill_diagonal(d, 0.0)
    return d


def test_daura_rule_on_hand_made_graphs():
    from abx_amd import ensemble
    clique = lambda nodes: [(a, b) for a in nodes for b in nodes if a < b]
    # two cliques that share node 3, and the singleton 6: node 3 has the most neighbours (5) and takes both cliques whole
    d = graph(7, clique([0, 1, 2, 3]) + clique([3, 4, 5]))
    cl, cen = ensemble.cluster_host(d, 1.0)
    assert cl.tolist() == [0, 0, 0, 0, 0, 0, 1] and cen == [3, 6]
    # a clique with a tail 3-4-5: node 3 (neighbours 0, 1, 2, 4) takes 4 away from 5, which is left alone like 6
    d = graph(7, clique([0, 1, 2, 3]) + [(3, 4), (4, 5)])
    cl, cen = ensemble.cluster_host(d, 1.0)
    assert cl.tolist() == [0, 0, 0, 0, 0, 1, 2] and cen == [3, 5, 6]
    # a tie: on the path 0-1-2-3 the nodes 1 and 2 both have two neighbours, the lower index wins and leaves 3 alone
    cl, cen = ensemble.cluster_host(graph(4, [(0, 1), (1, 2), (2, 3)]), 1.0)
    assert cl.tolist() == [0, 0, 0, 1] and cen == [1, 3]
    # the cutoff is inclusive, a value just above it is no neighbour, the diagonal never counts
    cl, cen = ensemble.cluster_host(np.array([[0.0, 1.0, 1.0 + 1e-12], [1.0, 0.0, 5.0], [1.0 + 1e-12, 5.0, 0.0]]), 1.0)
    assert cl.tolist() == [0, 0, 1] and cen == [0, 2]
    # counts are of UNASSIGNED neighbours: after the star around 0 is gone, 5 (two free neighbours) beats 4 (one free, two taken)
    d = graph(8, [(0, 1), (0, 2), (0, 3), (4, 1), (4, 2), (4, 7), (5, 6), (5, 7)])
    cl, cen = ensemble.cluster_host(d, 1.0)
    assert cen == [0, 5, 4] and cl.tolist() == [0, 0, 0, 0, 2, 1, 1, 1]
    # the table of the first graph: cluster, is_centre, n_neighbours (all designs), first_same_seq from the third plane
    d = graph(7, clique([0, 1, 2, 3]) + clique([3, 4, 5]))
    sd = np.ones((7, 7)) - np.eye(7)
    sd[2, 5] = sd[5, 2] = 0.0
    t, cen = ensemble.table_host(np.stack([d, 2 * d, sd]), 'fit', 1.0)
    assert t[:, 0].tolist() == [0, 0, 0, 0, 0, 0, 1] and t[:, 1].tolist() == [0, 0, 0, 1, 0, 0, 1] and t[:, 2].tolist() == [3, 3, 3, 5, 2, 2, 0]
    assert t[:, 8].tolist() == [0, 0, 1, 0, 0, 1, 0] and t[:, 9].tolist() == [0, 1, 2, 3, 4, 2, 6]
    assert abs(t[0, 3] - (3 * 1.0 + 3 * 9.0) / 6) < 1e-15 and t[0, 4] == 1.0 and t[6, 4] == 9.0 and t[0, 6] == 2.0 and abs(t[0, 7] - 1.0) < 1e-15
    # on the frame plane (2 d) nothing is within 1.0: seven singletons in index order
    t2, cen2 = ensemble.table_host(np.stack([d, 2 * d, sd]), 'frame', 1.0)
    assert cen2 == list(range(7)) and t2[:, 2].tolist() == [0] * 7
    # a single design: means and minima are NaN, counts 0, it is its own cluster and centre
    t1, cen1 = ensemble.table_host(np.zeros((3, 1, 1)), 'fit', 1.0)
    assert cen1 == [0] and t1[0, :3].tolist() == [0, 1, 0] and np.isnan(t1[0, 3:8]).all() and t1[0, 8:].tolist() == [0, 0]


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_synthetic_ensemble_has_the_clusters_it_was_built_with(seed):
    """What tests/test_gpu_ensemble.py relies on: three clusters far from the cutoff, a duplicate, a moved copy."""
    x, seq, region, host = EC.case(seed)
    p, N = host['planes'], x.shape[0]
    cl = host['table'][:, 0].astype(int)
    same, off = cl[:, None] == cl[None], ~np.eye(N, dtype=bool)
    print(f'seed {seed}: within <= {p[0][same & off].max():.4f}, between >= {p[0][~same].min():.4f}, rmsd_fit[4][5] = {p[0, 4, 5]:.3e}, '
          f'rmsd_fit[6][7] = {p[0, 6, 7]:.3e}, rmsd_frame[6][7] = {p[1, 6, 7]:.3f}')
    assert host['n_clusters'] == 3 and host['centres'][:4].tolist() == [0, 1, 2, -1]
    base = np.arange(N) % 3
    base[5], base[7] = base[4], base[6]                 # the copies follow their originals
    assert np.array_equal(cl, base)                     # (9, 8 and 7 designs: discovered in the order of the bases)
    assert p[0][same & off].max() <= 0.42 and p[0][~same].min() >= 3.2
    assert np.abs(p[0][off] - 1.0).min() >= 0.5
    assert p[0, 4, 5] <= 1e-14 and p[1, 4, 5] == 0.0 and p[2, 4, 5] == 0
    assert 5e-8 <= p[0, 6, 7] <= 5e-7 and 5.0 <= p[1, 6, 7] <= 8.0 and p[2, 6, 7] == 0
    assert host['table'][5, 9] == 4 and host['table'][7, 9] == 6 and host['table'][4, 8] >= 1


def test_twin_handles_degenerate_and_mirrored_sets():
    """Collinear C-alpha triples: the rotation is not unique, the RMSD is (and equals the 1-D fit of the sorted spacings here: the
    lines can be laid on each other); a mirrored copy keeps a non-zero rmsd_fit (proper rotations only) although its distances agree."""
    x, seq, region, host = EC.case(0, N=4, M=3, atoms='ca', kind='collinear')
    r = np.nonzero(region)[0]
    for i in range(4):
        for j in range(i + 1, 4):
            a, b = x[i, r, 1].astype(np.float64), x[j, r, 1].astype(np.float64)
            ta, tb = np.linalg.norm(a - a.mean(0), axis=1) * [-1, 0, 1], np.linalg.norm(b - b.mean(0), axis=1) * [-1, 0, 1]
            assert abs(host['planes'][0, i, j] - np.sqrt(np.mean((ta - tb) ** 2))) <= 1e-12
    x, seq, region, host = EC.case(0, N=2, M=8, kind='mirror')
    pts = x[:, np.nonzero(region)[0], :4].reshape(2, -1, 3).astype(np.float64)
    dist = lambda q: np.linalg.norm(q[:, None] - q[None], axis=-1)
    assert np.abs(dist(pts[0]) - dist(pts[1])).max() == 0.0 and host['planes'][0, 0, 1] > 0.5


def test_formats_and_summary(tmp_path):
    from abx_amd import design, ensemble
    table = np.array([[0, 1, 2, 1.25, 0.5, 3.0, 0.75, 2.0, 0, 0],
                      [0, 0, 1, 1.5, 0.5, 3.5, 0.75, 2.5, 1, 1],
                      [1, 1, 0, 2.25, 1.0, 4.0, 2.0, 3.0, 0, 2],
                      [0, 0, 1, 1.0, 0.25, 2.5, 0.5, 2.5, 1, 1]], dtype=np.float64)
    assert ensemble.format_ensemble(table[1]) == ['0', '0', '1', '1.5000', '0.5000', '3.5000', '0.7500', '2.5000', '1', '1']
    assert ensemble.format_ensemble([0, 1, 0] + [float('nan')] * 5 + [0, 0]) == ['0', '1', '0', 'nan', 'nan', 'nan', 'nan', 'nan', '0', '0']
    s = ensemble.summary(table, n_region=10)
    assert tuple(s) == ensemble.SUMMARY_COLUMNS
    assert [s[k] for k in ('n_designs', 'n_clusters', 'largest_cluster', 'n_unique_seq')] == [4, 2, 3, 3]
    assert (s['rmsd_fit_mean'], s['rmsd_frame_mean'], s['seq_diff_mean'], s['seq_identity_mean']) == (1.5, 3.25, 2.5, 0.75)
    assert np.isnan(ensemble.summary(table)['seq_identity_mean'])
    one = ensemble.summary([[0, 1, 0] + [float('nan')] * 5 + [0, 0]], n_region=3)
    assert (one['n_designs'], one['n_clusters'], one['largest_cluster'], one['n_unique_seq']) == (1, 1, 1, 1) and np.isnan(one['rmsd_fit_mean'])
    # the driver's table: header, the `all` line, one line per sample id with the sample id of its cluster's centre
    ids = [10, 11, 12, 13]
    path = design._write_ensemble(str(tmp_path), '6ct7_H_L_S', s, list(zip(ids, table.tolist())), [0, 2])
    assert os.path.basename(path) == '6ct7_H_L_S_ensemble.tsv'
    lines = [ln.split('\t') for ln in open(path).read().splitlines()]
    own = ['n_designs', 'n_clusters', 'largest_cluster', 'n_unique_seq', 'seq_identity_mean']
    assert lines[0] == ['sample'] + list(ensemble.ENSEMBLE_COLUMNS) + ['representative'] + ['all_' + c for c in own]
    assert len(lines) == 6 and all(len(r) == len(lines[0]) for r in lines)
    assert lines[1] == ['all', 'nan', 'nan', 'nan', '1.5000', 'nan', '3.2500', 'nan', '2.5000', 'nan', 'nan', 'nan', '4', '2', '3', '3', '0.7500']
    for k, r in enumerate(lines[2:]):
        assert r == [str(ids[k])] + ensemble.format_ensemble(table[k]) + [['10', '10', '12', '10'][k]] + ['nan'] * 5
    ap = design.build_parser()
    a = ap.parse_args([])
    assert a.ensemble is False and a.ensemble_matrix is False
    assert (a.ensemble_cutoff, a.ensemble_metric, a.ensemble_atoms) == (1.0, 'fit', 'backbone')
    a = ap.parse_args(['--ensemble', '--ensemble_cutoff', '2.5', '--ensemble_metric', 'frame', '--ensemble_atoms', 'ca', '--ensemble_matrix'])
    assert a.ensemble and a.ensemble_matrix and (a.ensemble_cutoff, a.ensemble_metric, a.ensemble_atoms) == (2.5, 'frame', 'ca')
    for bad in (dict(atoms='all'), dict(metric='rmsd'), dict(cutoff=-1.0), dict(cutoff=float('nan'))):
        with pytest.raises(ValueError):
            ensemble.ensemble_host(np.zeros((2, 4, 14, 3)), np.zeros((2, 4), int), np.ones(4, bool), **bad)
