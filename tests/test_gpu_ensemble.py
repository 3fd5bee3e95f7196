"""GPU checks of the ensemble analysis (abx_ensemble_pairs / abx_ensemble_cluster, csrc/ensemble.hip; abx_amd.ensemble.EnsembleAnalyzer)
against the float64 host twin ensemble.ensemble_host on the same float32-representable inputs: the three planes of every pair, the
Daura clusters and the summary rows, the shapes at which the kernels take another path, independence of a pair from its batch, the
cluster kernel alone up to its size limit, and the path through the design driver."""
import os

import numpy as np
import pytest
import torch

from analysis_gpu_cases import CODES, DEV, assert_same_bytes, names, pdb_args, set_master_port, table_lines, ops  # noqa: F401  (ops: set up once per importing module)
import ensemble_cases as EC

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 2, 8, 9]            # cluster, is_centre, n_neighbours, n_same_seq, first_same_seq
STATS = [3, 4, 5, 6, 7]             # rmsd_fit_mean / min, rmsd_frame_mean / min, seq_diff_mean


def analyze(x, seq, region, Lab=None, **kw):
    """EnsembleAnalyzer of a complex whose antibody has Lab rows (default: all but the last two of x: the coordinates always reach
    the kernel as the [:, :Lab] view of a longer tensor) -> the result dict as numpy arrays."""
    from abx_amd import ensemble
    L = x.shape[1]
    Lab = L - 2 if Lab is None else Lab
    xd, sd = torch.from_numpy(np.array(x)).to(DEV), torch.from_numpy(np.array(seq)).to(DEV)
    an = ensemble.EnsembleAnalyzer({'seq': sd[0], 'anchor_flag': torch.zeros(Lab, dtype=torch.int32)}, region=torch.from_numpy(np.array(region)), **kw)
    assert not xd[:, :Lab].is_contiguous() or x.shape[0] == 1
    res = an.analyze(xd, sd)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def compare(got, host, cutoff=1.0, metric=0):
    """The bounds of the issue: planes 0 and 1 within 1e-9 max(1, r) (what tests/test_gpu_design_scores.py holds the same arithmetic
    to), plane 2 / clusters / centres / counts equal, means and minima within 1e-9 max(1, v), exact symmetry and zero diagonal."""
    N = host['planes'].shape[1]
    gp, hp = got['planes'], host['planes']
    off = ~np.eye(N, dtype=bool)
    near = np.abs(hp[metric][off] - cutoff).min() if N > 1 else np.inf
    err = [np.abs(gp[k] - hp[k]) / np.maximum(1.0, hp[k]) for k in (0, 1)]
    print(f'N = {N}: nearest pair to the cutoff {near:.3e}; plane errors / max(1, r): fit {err[0].max():.3e}, frame {err[1].max():.3e}')
    assert near > 1e-6, 'a pair of the TEST sits on the cutoff: its neighbour bit is not defined by the bounds below'
    assert gp.shape == (3, N, N) and np.isfinite(gp).all()
    for k in range(3):
        assert np.array_equal(gp[k], gp[k].T) and not gp[k][~off].any(), f'plane {k}: symmetric with a zero diagonal, exactly'
    assert err[0].max() <= 1e-9, f'rmsd_fit: pair {np.unravel_index(err[0].argmax(), (N, N))} off by {err[0].max():.3e}'
    assert err[1].max() <= 1e-9, f'rmsd_frame: off by {err[1].max():.3e}'
    assert np.array_equal(gp[2], hp[2])
    gt, ht = got['table'], host['table']
    assert gt.shape == ht.shape == (N, 10)
    assert int(got['n_clusters'][0]) == host['n_clusters'] and np.array_equal(got['centres'], host['centres'])
    assert np.array_equal(gt[:, COUNTS], ht[:, COUNTS]), (gt[:, COUNTS], ht[:, COUNTS])
    if N == 1:
        assert np.isnan(gt[:, STATS]).all() and np.isnan(ht[:, STATS]).all()
    else:
        assert (np.abs(gt[:, STATS] - ht[:, STATS]) <= 1e-9 * np.maximum(1.0, np.abs(ht[:, STATS]))).all()


def test_synthetic_ensemble_against_the_host_twin():
    """N = 24 designs of three base loops, M = 8, backbone (tests/ensemble_cases.py; its properties are asserted on the CPU in
    tests/test_ensemble_host.py).  The pair (6, 7) - the same loop moved rigidly, 1e-7 A apart after superposition on points with a
    10 A spread - fails the bound of plane 0 when the deviation is formed as G_a + G_b - 2 lambda."""
    x, seq, region, host = EC.case(0)
    got = analyze(x, seq, region)
    print(f'rmsd_fit[4][5] = {got["planes"][0, 4, 5]:.3e} (twin {host["planes"][0, 4, 5]:.3e}), rmsd_fit[6][7] = {got["planes"][0, 6, 7]:.6e} '
          f'(twin {host["planes"][0, 6, 7]:.6e}), rmsd_frame[6][7] = {got["planes"][1, 6, 7]:.9f}')
    compare(got, host)
    assert got['n_clusters'][0] == 3 and got['centres'][:3].tolist() == [0, 1, 2]
    assert abs(got['planes'][0, 6, 7] - host['planes'][0, 6, 7]) <= 1e-9 and 5e-8 <= got['planes'][0, 6, 7] <= 5e-7
    # clustering on the other plane, with another cutoff and the C-alpha only: the same kernels, other arguments
    xf, sf, rf, hf = EC.case(0, metric='frame', cutoff=0.9, atoms='ca')
    compare(analyze(xf, sf, rf, metric='frame', cutoff=0.9, atoms='ca'), hf, cutoff=0.9, metric=1)


@pytest.mark.parametrize('N', [1, 2, 17, 33])
def test_tile_edges(N):
    """8 x 8 tiles of pairs: one design, one pair, one past two tiles, one past four."""
    x, seq, region, host = EC.case(0, N=N)
    compare(analyze(x, seq, region), host)


@pytest.mark.parametrize('name,kw,atoms', [
    ('one residue, P = 4', dict(N=9, M=1), 'backbone'),
    ('three C-alpha, planar', dict(N=9, M=3), 'ca'),
    ('three C-alpha, exactly collinear', dict(N=9, M=3, kind='collinear'), 'ca'),
    ('the limit, P = 512', dict(N=5, M=128), 'backbone'),
    ('the limit with C-alpha, M = 512', dict(N=3, M=512), 'ca'),
    ('rows 0, 2, 3, 7, 11 and Lab - 1', dict(N=9, M=6, rows=(0, 2, 3, 7, 11, 15)), 'backbone'),
    ('a mirrored copy', dict(N=2, M=8, kind='mirror'), 'backbone'),
])
def test_shapes_at_which_the_kernel_can_go_wrong(name, kw, atoms):
    x, seq, region, host = EC.case(0, atoms=atoms, **kw)
    Lab = 16 if 'rows' in kw else None
    if 'rows' in kw:
        assert region[0] and region[Lab - 1] and x.shape[1] > Lab
    got = analyze(x, seq, region, Lab=Lab, atoms=atoms)
    compare(got, host)
    if kw.get('kind') == 'mirror':                       # proper rotations only: the mirror image does not fit
        assert host['planes'][0, 0, 1] > 0.5 and abs(got['planes'][0, 0, 1] - host['planes'][0, 0, 1]) <= 1e-9 * host['planes'][0, 0, 1]


def test_a_pair_does_not_depend_on_its_batch():
    """Designs 0..9 analysed alone: their planes are the bits of the corresponding block of the N = 33 call."""
    x, seq, region, _ = EC.case(0, N=33)
    big = analyze(x, seq, region)['planes']
    small = analyze(x[:10], seq[:10], region)['planes']
    assert torch.equal(torch.from_numpy(small), torch.from_numpy(np.ascontiguousarray(big[:, :10, :10])))
    # ... nor on the tile it lands in: designs 20..32 (tiles 2-4 of the large call, tiles 0-1 alone)
    tail = analyze(x[20:], seq[20:], region)['planes']
    assert torch.equal(torch.from_numpy(tail), torch.from_numpy(np.ascontiguousarray(big[:, 20:, 20:])))


def integer_planes(N, seed):
    rng = np.random.default_rng(seed)
    planes = np.zeros((3, N, N))
    for k in range(3):
        m = np.triu(rng.integers(0, 10, (N, N)), 1)
        planes[k] = m + m.T
    return planes


@pytest.mark.parametrize('N', [1, 2, 63, 64, 65, 100, 257, 1024])
def test_cluster_kernel_alone(ops, N):
    """Integer-valued symmetric planes, cutoff 3.5: no value is near the cutoff, every sum is exact.  Word edges of the neighbour
    bits (63, 64, 65), a partial last word (100, 257), the limit (1024)."""
    from abx_amd import ensemble
    planes = integer_planes(N, N)
    for metric in (('fit', 'frame') if N in (65, 100) else ('fit',)):
        ht, hc = ensemble.table_host(planes, metric, 3.5)
        table, centres, n = ops.ensemble_cluster(torch.from_numpy(planes).to(DEV), metric=ensemble.METRICS[metric], cutoff=3.5)
        torch.cuda.synchronize()
        table, centres = table.cpu().numpy(), centres.cpu().numpy()
        print(f'N = {N}, {metric}: {len(hc)} clusters, largest {np.bincount(ht[:, 0].astype(int)).max()}')
        assert int(n) == len(hc) and centres[:len(hc)].tolist() == hc and (centres[len(hc):] == -1).all()
        assert np.array_equal(table[:, COUNTS], ht[:, COUNTS])
        if N > 1:
            assert (np.abs(table[:, STATS] - ht[:, STATS]) <= 1e-9 * np.maximum(1.0, ht[:, STATS])).all()
        else:
            assert np.isnan(table[:, STATS]).all()
    # rows of a wider table are written in place
    wide = torch.full((N, 14), -7.0, dtype=torch.float64, device=DEV)
    ops.ensemble_cluster(torch.from_numpy(planes).to(DEV), metric=0, cutoff=3.5, out=wide[:, 2:12])
    ht, _ = ensemble.table_host(planes, 'fit', 3.5)
    w = wide.cpu().numpy()
    assert np.array_equal(w[:, 2:12][:, COUNTS], ht[:, COUNTS]) and (w[:, :2] == -7.0).all() and (w[:, 12:] == -7.0).all()


def test_cluster_kernel_refuses_more_than_its_limit(ops):
    from abx_amd._lib import AbxHipError
    planes = torch.zeros(3, 1025, 1025, dtype=torch.float64, device=DEV)
    with pytest.raises(AbxHipError, match='abx_ensemble_cluster'):
        ops.ensemble_cluster(planes, metric=0, cutoff=1.0)
    from abx_amd import ensemble
    with pytest.raises(ValueError):
        ensemble.EnsembleAnalyzer({'seq': torch.zeros(700, dtype=torch.int64, device=DEV), 'anchor_flag': torch.zeros(600)},
                                  region=torch.ones(600), atoms='ca')


def read_backbone(path, chain, residues):
    """(len(residues), 4, 3) N, CA, C, O of the 1-based residue numbers `residues` of `chain` in a written PDB file."""
    out = np.full((len(residues), 4, 3), np.nan)
    slot = {'N': 0, 'CA': 1, 'C': 2, 'O': 3}
    for ln in open(path):
        if ln.startswith('ATOM') and ln[21] == chain and ln[12:16].strip() in slot and int(ln[22:26]) in residues:
            out[residues.index(int(ln[22:26])), slot[ln[12:16].strip()]] = [float(ln[30:38]), float(ln[38:46]), float(ln[46:54])]
    assert np.isfinite(out).all(), path
    return out


def check_tsv(path, npy, pdbs, seqs, rows, **kw):
    """<complex>_ensemble.tsv and _ensemble_rmsd.npy against ensemble_host of what the PDB files and the designs table hold: the
    files carry 1e-3 A (8.3f), hence 2e-3 on every distance; tokens and, with the clusters the twin finds, every integer."""
    from abx_amd import ensemble
    N, M = len(pdbs), len(rows)
    x = np.zeros((N, max(rows) + 1, 14, 3))
    for k, p in enumerate(pdbs):
        x[k, rows, :4] = read_backbone(p, 'H', [r + 1 for r in rows])
    seq = np.array([[ord(c) for c in s] for s in seqs])[:, :max(rows) + 1]
    region = np.zeros(max(rows) + 1, bool)
    region[rows] = True
    host = ensemble.ensemble_host(x, seq, region, **kw)
    lines = [ln.split('\t') for ln in open(path).read().splitlines()]
    assert lines[0][:12] == ['sample'] + list(ensemble.ENSEMBLE_COLUMNS) + ['representative'] and lines[1][0] == 'all' and len(lines) == 2 + N
    assert all(len(r) == len(lines[0]) for r in lines)
    table = np.array([[float(v) for v in r[1:11]] for r in lines[2:]])
    assert [r[0] for r in lines[2:]] == [str(i) for i in range(N)]
    off = ~np.eye(N, dtype=bool)
    print('driver table\n', table, '\nhost\n', host['table'], '\nnearest to the cutoff', np.abs(host['planes'][0][off] - kw.get('cutoff', 1.0)).min())
    assert np.array_equal(table[:, [8, 9]], host['table'][:, [8, 9]])
    assert (np.abs(table[:, STATS] - host['table'][:, STATS]) <= 2e-3).all()
    planes = np.load(npy)
    assert planes.shape == (3, N, N) and planes.dtype == np.float64
    assert (np.abs(planes[:2] - host['planes'][:2]) <= 2e-3).all() and np.array_equal(planes[2], host['planes'][2])
    # clusters: those of the twin ON THE WRITTEN PLANES (a pair within 2e-3 of the cutoff may fall on either side in the files)
    ht, hc = ensemble.table_host(planes, kw.get('metric', 'fit'), kw.get('cutoff', 1.0))
    assert np.array_equal(table[:, COUNTS], ht[:, COUNTS])
    assert [r[11] for r in lines[2:]] == [str(hc[int(c)]) for c in ht[:, 0]]
    s = ensemble.summary(ht, M)
    head = lines[0]
    assert int(lines[1][head.index('all_n_designs')]) == N and int(lines[1][head.index('all_n_clusters')]) == len(hc)
    assert int(lines[1][head.index('all_n_unique_seq')]) == s['n_unique_seq'] and int(lines[1][head.index('all_largest_cluster')]) == s['largest_cluster']
    assert abs(float(lines[1][head.index('rmsd_fit_mean')]) - s['rmsd_fit_mean']) <= 2e-4
    assert abs(float(lines[1][head.index('all_seq_identity_mean')]) - s['seq_identity_mean']) <= 1e-4


def test_design_driver_writes_the_ensemble_table(tmp_path, monkeypatch):
    """`abx_amd.design --ensemble --ensemble_matrix` on the smallest synthetic workload, 6 samples: plainly and through the 1-rank
    collective (the backbone as one more gathered field).  Both write the same table, which equals the twin on the backbone read back
    from the PDB files; a run without the flag writes the other files with the same bytes and no _ensemble file."""
    from abx_amd import design, synthetic
    set_master_port(monkeypatch)
    common = ['--workload', 'tiny', '--num_samples', '6', '--num_t', '2']
    ens = ['--ensemble', '--ensemble_matrix', '--ensemble_cutoff', '40.0']
    files = design.main(common + ens + ['--output_dir', str(tmp_path / 'ens')])
    files_c = design.main(common + ens + ['--force_collective', '--output_dir', str(tmp_path / 'coll')])
    plain = design.main(common + ['--output_dir', str(tmp_path / 'plain')])
    extra = ['tiny_H_L_A_ensemble.tsv', 'tiny_H_L_A_ensemble_rmsd.npy']
    assert names(files) == names(files_c) == sorted(names(plain) + extra)
    assert not [n for n in names(plain) if 'ensemble' in n] and sorted(os.listdir(tmp_path / 'plain')) == names(plain)
    assert sorted(os.listdir(tmp_path / 'ens')) == names(files)
    for d in ('ens', 'coll'):
        assert_same_bytes(plain, tmp_path / d)
    for n in extra:
        assert open(tmp_path / 'ens' / n, 'rb').read() == open(tmp_path / 'coll' / n, 'rb').read(), n
    first, last = synthetic.WORKLOADS['tiny']['cdr']
    tsv = [ln.split('\t') for ln in open(tmp_path / 'ens' / 'tiny_H_L_A_designs.tsv').read().splitlines()[1:]]
    check_tsv(tmp_path / 'ens' / extra[0], tmp_path / 'ens' / extra[1], [tmp_path / 'ens' / f'tiny-{i:03d}_H_L_A.pdb' for i in range(6)],
              [r[2] for r in tsv], list(range(first, last)), cutoff=40.0)     # (the last CDR residue is not diffused: features.py)


def test_design_driver_set_level_rows_carry_the_backbone(tmp_path, monkeypatch):
    """Two complexes through the set-level schedule (one gather of rows, the backbone as 12 maxLab further columns): the same ensemble
    files as the complex-by-complex run, and every other file unchanged by the flag."""
    from abx_amd import design
    set_master_port(monkeypatch)
    codes = CODES
    common = pdb_args(codes) + ['--num_samples', '3', '--num_t', '2']
    ens = ['--ensemble', '--ensemble_matrix', '--ensemble_atoms', 'ca', '--ensemble_metric', 'frame', '--ensemble_cutoff', '3.0']
    set_level = ['--force_collective', '--min_block', '1']
    a = design.main(common + ens + ['--output_dir', str(tmp_path / 'one')])
    b = design.main(common + ens + set_level + ['--score', '--output_dir', str(tmp_path / 'set')])
    c = design.main(common + set_level + ['--score', '--output_dir', str(tmp_path / 'set_plain')])
    extra = sorted(f'{code}_ensemble{end}' for code in codes for end in ('.tsv', '_rmsd.npy'))
    assert names(a) == names(b) == sorted(names(c) + extra)
    for n in extra:
        assert open(tmp_path / 'one' / n, 'rb').read() == open(tmp_path / 'set' / n, 'rb').read(), n
    assert_same_bytes(c, tmp_path / 'set')
    for code in codes:
        lines = table_lines(tmp_path / 'set', code, 'ensemble')
        assert len(lines) == 2 + 3 and lines[1][0] == 'all' and [r[0] for r in lines[2:]] == ['0', '1', '2']
        planes = np.load(tmp_path / 'set' / f'{code}_ensemble_rmsd.npy')
        assert planes.shape == (3, 3, 3) and (planes[0][~np.eye(3, dtype=bool)] > 0).all() and (planes[1] >= planes[0] - 1e-9).all()
