"""GPU checks of the design scores (abx_design_scores, csrc/metrics.hip; abx_amd.metrics.DesignScorer): RMSD / AAR against the
reference-pinned host calc_ab_metrics, the violation counts against the reference's masks (vio_pdb.npz), the clash counts against the
fp64 host twin and the clash energy of abx_clash_grad, batch invariance, and the path through the sampler and the design driver."""
import os
import warnings

import numpy as np
import pytest
import torch

from analysis_gpu_cases import ALONE, CODES, DEV, SHARED, pdb_args, set_master_port, spy_on_sampler, ops, gpu_model  # noqa: F401  (ops, gpu_model: set up once per importing module)
from conftest import GOLDEN, load_npz, tt

pytestmark = pytest.mark.gpu

VIO_KEYS = ('c_n_violation_mask', 'ca_c_n_violation_mask', 'c_n_ca_violation_mask')


def col(name):
    from abx_amd import metrics
    return metrics.SCORE_COLUMNS.index(name)


def f32(x):
    """float64 array rounded to float32 and back: the values the kernel sees."""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def tokens(s):
    from abx_amd import residue_constants as rc
    return torch.tensor([rc.restypes.index(c) if c in rc.restypes else 20 for c in s], dtype=torch.int64)


def ca_atom14(ca):
    """(N,3) C-alpha coordinates as an atom14 tensor (all other slots at the origin)."""
    x = torch.zeros(ca.shape[0], 14, 3)
    x[:, 1] = torch.from_numpy(np.asarray(ca, dtype=np.float32))
    return x


def run_ca_cases(ops, gt, cdr, gs, preds, seqs, exists=None):
    """Scores of C-alpha-only structures: gt (N,3) float64 already float32-representable, preds list of (N,3), seqs list of strings;
    exists: None or list of (N,) bool ground-truth C-alpha masks (then the complex is passed per structure)."""
    N = gt.shape[0]
    x = torch.stack([ca_atom14(p) for p in preds]).to(DEV)
    sq = torch.stack([tokens(s) for s in seqs]).to(DEV)
    chain = torch.zeros(N, dtype=torch.int32)
    if exists is None:
        ge = torch.ones(N, 14, dtype=torch.bool)
        return ops.design_scores(x, sq, ca_atom14(gt).to(DEV), tokens(gs).to(DEV), ge.to(DEV), tt(cdr).int().to(DEV), chain.to(DEV)).cpu().numpy()
    B = len(preds)
    ge = torch.ones(B, N, 14, dtype=torch.bool)
    for b, e in enumerate(exists):
        ge[b, :, 1] = torch.as_tensor(e)
    rep = lambda t: t[None].expand(B, *t.shape).contiguous().to(DEV)
    return ops.design_scores(x, sq, rep(ca_atom14(gt)), rep(tokens(gs)), ge.to(DEV), tt(cdr).int().to(DEV), rep(chain)).cpu().numpy()


def assert_row_matches_host(row, want, what):
    """row: kernel scores; want: OrderedDict of calc_ab_metrics on the same float32-representable inputs.  RMSD at the bound the host
    code is held to against the reference (1e-9 max(1, |r|), test_host_cpu.py), AAR exactly."""
    for k, r in want.items():
        v = float(row[col(k)])
        print(f'{what} {k}: kernel {v!r} host {r!r} diff {abs(v - r):.3e}')
        assert abs(v - r) <= (0.0 if k.endswith('AAR') else 1e-9 * max(1.0, abs(r))), (what, k, v, r)


def test_rmsd_and_aar_match_host_calc_ab_metrics(ops):
    from abx_amd import metrics
    z = load_npz('metrics_6qd7.npz')
    gt, cdr, gs = f32(z['gt_coord']), z['cdr_def'], str(z['gt_str_seq'])
    cases = [str(c) for c in z['cases']]
    preds = [f32(z[f'{c}.pred_coord']) for c in cases]
    seqs = [str(z[f'{c}.pred_str_seq']) for c in cases]
    # ---- the four golden cases as one batch on a shared complex
    got = run_ca_cases(ops, gt, cdr, gs, preds, seqs)
    assert got.shape == (4, len(metrics.SCORE_COLUMNS))
    host = [metrics.calc_ab_metrics(gt, p, cdr, gs, s) for p, s in zip(preds, seqs)]
    for c, row, want in zip(cases, got, host):
        assert_row_matches_host(row, want, c)
        # the golden values themselves (unrounded inputs) are 1.2e-6 away at most
        for k, r in zip(z[f'{c}.names'], z[f'{c}.values']):
            assert abs(float(row[col(str(k))]) - float(r)) <= (0.0 if str(k).endswith('AAR') else 5e-6), (c, k)
    # ---- three more, one complex per structure
    rng = np.random.RandomState(11)
    mirrored = preds[1] * np.array([-1.0, 1.0, 1.0])                        # the reflection branch of the reference's kabsch
    X_, Y_ = gt - gt.mean(0), mirrored - mirrored.mean(0)
    V, _, W = np.linalg.svd(X_.T @ Y_)
    assert np.linalg.det(V) * np.linalg.det(W) < 0
    Q, _ = np.linalg.qr(rng.randn(3, 3))
    Q = Q * np.sign(np.linalg.det(Q))
    moved = f32(preds[2] @ Q.T + rng.randn(3) * 20.0)                       # a generic rigid motion, then what the kernel can hold
    # a rigid motion float32 holds exactly (a random proper axis permutation with signs): its RMSDs ARE c2's
    perm = rng.permutation(3)
    P = np.zeros((3, 3))
    P[np.arange(3), perm] = rng.choice([-1.0, 1.0], 3)
    if np.linalg.det(P) < 0:
        P[0] = -P[0]
    turned = preds[2] @ P.T
    assert np.array_equal(f32(turned), turned) and abs(np.linalg.det(P) - 1.0) < 1e-12
    keep = np.ones(gt.shape[0], dtype=bool)
    drop = [int(np.where(cdr == 1)[0][2]), 60, int(np.where(cdr == 12)[0][1])]       # heavy CDR1, framework, light CDR3
    keep[drop] = False
    ones = np.ones_like(keep)
    got3 = run_ca_cases(ops, gt, cdr, gs, [mirrored, moved, turned, preds[1]], [seqs[1], seqs[2], seqs[2], seqs[1]], exists=[ones, ones, ones, keep])
    assert_row_matches_host(got3[0], metrics.calc_ab_metrics(gt, mirrored, cdr, gs, seqs[1]), 'c1 mirrored')
    assert_row_matches_host(got3[1], metrics.calc_ab_metrics(gt, moved, cdr, gs, seqs[2]), 'c2 moved')
    assert_row_matches_host(got3[2], metrics.calc_ab_metrics(gt, turned, cdr, gs, seqs[2]), 'c2 turned')
    sub = lambda s: ''.join(ch for ch, k in zip(s, keep) if k)
    assert_row_matches_host(got3[3], metrics.calc_ab_metrics(gt[keep], preds[1][keep], cdr[keep], sub(gs), sub(seqs[1])), 'c1 masked')
    for k in host[2]:
        if k.endswith('RMSD'):
            # exact motion: c2's own RMSD at the same bound; generic motion: its float32 rounding displaces an atom by at most
            # sqrt(3) 2^-18 A (|x| < 128), and an RMSD by no more than the displacement it is built from
            assert abs(got3[2][col(k)] - host[2][k]) <= 1e-9 * max(1.0, host[2][k]), k
            assert abs(got3[1][col(k)] - host[2][k]) <= 1e-5, k
    assert got3[0][col('heavy_cdr1_RMSD')] > 5.0 and np.array_equal(got3[0][[0, 2, 4]], got[1][[0, 2, 4]])
    # ---- the Loop slice [4:-2] is taken on the CDR-H3 rows in sequence order; a masked row inside it is then skipped
    h3 = np.where(cdr == 5)[0]
    keep2 = np.ones_like(keep)
    keep2[h3[6]] = False
    row = run_ca_cases(ops, gt, cdr, gs, [preds[1]], [seqs[1]], exists=[keep2])[0]
    a_gt, a_pr = metrics.kabsch(gt[keep2].T, preds[1][keep2].T)
    pos = {int(i): n for n, i in enumerate(np.where(keep2)[0])}
    loop = [pos[int(i)] for i in h3[4:-2] if keep2[i]]
    assert len(loop) == len(h3) - 7
    want = float(np.sqrt(np.mean(np.sum((a_gt[:, loop] - a_pr[:, loop]) ** 2, axis=0))))
    assert abs(row[col('heavy_cdr3_Loop_RMSD')] - want) <= 1e-9 * max(1.0, want)
    assert row[col('heavy_cdr3_Loop_AAR')] == float(np.mean([gs[i] == seqs[1][i] for i in h3[4:-2] if keep2[i]]))


def test_no_light_chain_gives_nan_light_columns(ops):
    z = load_npz('metrics_6qd7.npz')
    gt, cdr = f32(z['gt_coord']), z['cdr_def'].copy()
    heavy = cdr < 7
    got = run_ca_cases(ops, gt[heavy], cdr[heavy], str(z['gt_str_seq'])[:int(heavy.sum())], [f32(z['c1.pred_coord'])[heavy]],
                       [str(z['c1.pred_str_seq'])[:int(heavy.sum())]])[0]
    assert np.isnan(got[8:14]).all() and np.isfinite(got[:8]).all() and np.isfinite(got[14:]).all()
    # the shipped 6ct7 has four CDR-H3 residues: its Loop slice [4:-2] is empty
    p = load_npz('pdb_6ct7.npz')
    assert int((p['batch.cdr_def'][0] == 5).sum()) == 4
    Lab = p['batch.anchor_flag'].shape[1]
    s = ops.design_scores(tt(p['batch.atom14_gt_positions']).to(DEV), tt(p['batch.seq'])[:, :Lab].to(DEV), tt(p['batch.atom14_gt_positions'])[0].to(DEV),
                          tt(p['batch.seq'])[0].to(DEV), tt(p['batch.atom14_gt_exists'])[0].to(DEV), tt(p['batch.cdr_def'])[0].int().to(DEV),
                          tt(p['batch.chain_id'])[0].int().to(DEV), Lab=Lab)[0].cpu().numpy()
    loop = [col('heavy_cdr3_Loop_AAR'), col('heavy_cdr3_Loop_RMSD')]
    assert np.isnan(s[loop]).all() and np.isfinite(np.delete(s, loop)).all()
    assert all(s[col(k)] == 1.0 for k in ('heavy_cdr3_AAR', 'light_cdr2_AAR')) and s[col('heavy_cdr3_RMSD')] < 1e-6


def complex_args(p, residx=True):
    """The complex of a pdb_*.npz fixture as design_scores takes it (shared by the batch)."""
    kw = dict(gt_atom14=tt(p['batch.atom14_gt_positions'])[0].to(DEV), gt_seq=tt(p['batch.seq'])[0].to(DEV),
              gt_exists=tt(p['batch.atom14_gt_exists'])[0].to(DEV), cdr_def=tt(p['batch.cdr_def'])[0].int().to(DEV),
              chain_id=tt(p['batch.chain_id'])[0].int().to(DEV), Lab=int(p['batch.anchor_flag'].shape[1]))
    if residx:
        kw['residx'] = tt(p['batch.residx'])[0].int().to(DEV)
    return kw


def test_violation_counts_equal_the_reference_masks(ops):
    """All eight cases of vio_pdb.npz, four per complex in one batch: the three counts are the sums of the reference's masks, exactly."""
    z = load_npz('vio_pdb.npz')
    for code in ('6ct7', '6qd7'):
        p = load_npz(f'pdb_{code}.npz')
        cases = [str(c) for c in z['cases'] if str(c).startswith(code)]
        assert len(cases) == 4
        x = torch.cat([tt(z[f'{c}.pos']) for c in cases]).to(DEV)
        B, Lab = 4, int(p['batch.anchor_flag'].shape[1])
        m = tt(p['batch.atom14_gt_exists']).expand(B, -1, -1).contiguous().to(DEV)
        sq = tt(p['batch.seq'])[:, :Lab].expand(B, -1).contiguous().to(DEV)
        got = ops.design_scores(x, sq, mask=m, **complex_args(p, residx=False)).cpu().numpy()
        for c, row in zip(cases, got):
            want = [float(z[f'{c}.{k}'].sum()) for k in VIO_KEYS]
            print(c, row[14:17].tolist(), want)
            assert row[14:17].tolist() == want, (c, row[14:17], want)
        if code == '6qd7':          # the bond across the gap of the cropped antigen patch is no bond once residue numbers link the pairs
            res = ops.design_scores(x[:1], sq[:1], mask=m[:1], **complex_args(p)).cpu().numpy()[0]
            assert got[0][14] == 1.0 and res[14] == 0.0 and res[15:17].tolist() == got[0][15:17].tolist()


def clash_cases():
    """(name, atom14 (1,L,14,3), fixture) of the clash checks: the coordinate sets of vio_pdb.npz; 6qd7.s3 has one candidate pair within
    1e-4 A of its bound, so its perturbation (sigma 0.4 A) is redrawn with another seed."""
    z = load_npz('vio_pdb.npz')
    out = []
    for c in z['cases']:
        p = load_npz(f'pdb_{str(c).split(".")[0]}.npz')
        x = tt(z[f'{c}.pos'])
        if str(c) == '6qd7.s3':
            x0 = tt(p['batch.atom14_gt_positions'])
            x = x0 + 0.4 * torch.randn(x0.shape, generator=torch.Generator().manual_seed(3))
        out.append((str(c), x, p))
    return out


def test_clash_counts_match_host_and_the_clash_energy(ops):
    from abx_amd import metrics, synthetic
    n_total = n_inter = 0
    for name, x, p in clash_cases():
        m, aa, ch, ri = tt(p['batch.atom14_gt_exists']), tt(p['batch.seq']), tt(p['batch.chain_id']), tt(p['batch.residx'])
        Lab = int(p['batch.anchor_flag'].shape[1])
        for residx in (ri, None):
            hn, hi, hb = (int(v) for v in metrics.clash_counts(x, m, aa, ch, residx))
            assert hb == 0, (name, 'a candidate pair within 1e-4 A of its bound: choose another perturbation')
            row = ops.design_scores(x.to(DEV), aa[:, :Lab].to(DEV), mask=m.to(DEV), **complex_args(p, residx=residx is not None)).cpu().numpy()[0]
            print(name, 'kernel', row[17:19].tolist(), 'host', hn, hi)
            assert row[17] == hn and row[18] == hi and row[18] <= row[17]
            e = ops.clash_grad(x.to(DEV), m.to(DEV), aa.to(DEV), ch.int().to(DEV), x[:, :, 1].contiguous().to(DEV), w_bond=0.0, w_angle=0.0,
                               residx=None if residx is None else residx.int().to(DEV))[0].cpu()
            assert (float(e[0, 0]) > 0.0) == (row[17] > 0), (name, float(e[0, 0]), row[17])
        n_total += hn
        n_inter += hi
    assert n_total > 100 and n_inter > 0
    # dense synthetic complexes: thousands of overlapping pairs, hundreds across chains; the atoms of the residue types (mask = None)
    for seed in (10, 19):
        cx = synthetic.make_complex(seed=seed, **synthetic.WORKLOADS['L256'])
        hn, hi, hb = (int(v) for v in metrics.clash_counts(cx['atom14_gt_positions'][None], cx['atom14_gt_exists'][None], cx['seq'][None],
                                                           cx['chain_id'][None], cx['residx'][None]))
        assert hb == 0 and hn > 2000 and hi > 100
        Lab = cx['anchor_flag'].shape[0]
        d = {k: v.to(DEV) for k, v in cx.items()}
        row = ops.design_scores(d['atom14_gt_positions'][None], d['seq'][None, :Lab], d['atom14_gt_positions'], d['seq'], d['atom14_gt_exists'],
                                d['cdr_def'], d['chain_id'], residx=d['residx'])[0].cpu().numpy()
        assert row[17] == hn and row[18] == hi, (seed, row[17:19], hn, hi)
        e = ops.clash_grad(d['atom14_gt_positions'][None], d['atom14_gt_exists'][None], d['seq'][None], d['chain_id'][None],
                           d['atom14_gt_positions'][None, :, 1].contiguous(), w_bond=0.0, w_angle=0.0, residx=d['residx'][None])[0]
        assert float(e[0, 0]) > 0.0
    # two residues 100 A apart
    aa = torch.zeros(2, dtype=torch.int64)
    x = torch.zeros(2, 14, 3)
    x[:, :, 0] = 3.0 * torch.arange(14.)[None]
    x[1, :, 1] = 100.0
    ex = torch.zeros(2, 14, dtype=torch.bool)
    ex[:, :5] = True
    args = (aa[None, :1].to(DEV), x.to(DEV), aa.to(DEV), ex.to(DEV), torch.tensor([1, 0], dtype=torch.int32).to(DEV), torch.tensor([0, 1], dtype=torch.int32).to(DEV))
    row = ops.design_scores(x[None].to(DEV), *args, Lab=1)[0].cpu().numpy()
    assert row[17] == 0.0 and row[18] == 0.0 and row[14:17].tolist() == [0.0, 0.0, 0.0]
    x[1, :, 1] = 1.0
    row = ops.design_scores(x[None].to(DEV), *args, Lab=1)[0].cpu().numpy()
    assert row[17] == 5.0 and row[18] == 5.0
    with pytest.raises(Exception, match='abx_design_scores'):                           # L > 1, the rule of abx_clash_grad
        ops.design_scores(x[None, :1].to(DEV), aa[None, :1].to(DEV), x[:1].to(DEV), aa[:1].to(DEV), ex[:1].to(DEV),
                          torch.zeros(1, dtype=torch.int32).to(DEV), torch.zeros(1, dtype=torch.int32).to(DEV), Lab=1)


def test_rows_do_not_depend_on_the_batch(ops):
    """B = 100 designs of the L = 352 workload: a structure's row is bit-identical when it is scored alone; a strided table keeps the rows
    in between."""
    from abx_amd import metrics, synthetic
    cx = synthetic.make_complex(seed=2, **synthetic.WORKLOADS['L352'])
    B, L, Lab = 100, cx['seq'].shape[0], cx['anchor_flag'].shape[0]
    assert (L, Lab) == (352, 228)
    g = torch.Generator().manual_seed(23)
    x = (cx['atom14_gt_positions'][None, :Lab] + 0.7 * torch.randn(B, Lab, 14, 3, generator=g)).to(DEV)
    sq = cx['seq'][None, :Lab].repeat(B, 1)
    mut = torch.rand(B, Lab, generator=g) < 0.2
    sq[mut] = torch.randint(0, 20, (int(mut.sum()),), generator=g)
    sq = sq.to(DEV)
    scorer = metrics.DesignScorer({k: v.to(DEV) for k, v in cx.items()})
    full = scorer.score(x, sq)
    assert full.shape == (B, len(metrics.SCORE_COLUMNS)) and full.dtype == torch.float64 and full.is_cuda
    h = full.cpu().numpy()
    assert np.isfinite(h[:, [col('heavy_cdr3_RMSD'), col('heavy_cdr3_Loop_RMSD'), col('heavy_cdr3_AAR')]]).all() and np.isfinite(h[:, 14:]).all()
    assert np.isnan(h[:, [col('heavy_cdr1_RMSD'), col('light_cdr3_AAR')]]).all()          # make_complex labels CDR-H3 only
    assert (h[:, 17] > 1000).all() and (h[:, 18] <= h[:, 17]).all() and h[:, 18].sum() > 0 and len({float(v) for v in h[:, 17]}) > 50
    for b in ALONE:
        alone = scorer.score(x[b:b + 1], sq[b:b + 1])
        assert torch.equal(alone[0].view(torch.int64), full[b].view(torch.int64)), b
    table = torch.full((3 * B, len(metrics.SCORE_COLUMNS)), -7.0, dtype=torch.float64, device=DEV)
    ret = scorer.score(x, sq, out=table[::3])
    assert ret.data_ptr() == table.data_ptr()
    assert torch.equal(table[::3].view(torch.int64), full.view(torch.int64))
    assert bool((table[1::3] == -7.0).all()) and bool((table[2::3] == -7.0).all())
    # the antibody-only view of a full-length tensor is read in place and scores the same
    xl = torch.cat([x, scorer.gt_atom14[None, Lab:].expand(B, -1, -1, -1)], 1)
    assert torch.equal(scorer.score(xl[:, :Lab], sq).view(torch.int64), full.view(torch.int64))
    assert torch.equal(scorer.score(xl, sq).view(torch.int64), full.view(torch.int64))


def host_scores(scorer, atom14, seq):
    """The host functions on one record: calc_ab_metrics on the antibody C-alpha (float64 of the float32 values), violation and clash
    counts on the antibody + ground-truth antigen."""
    from abx_amd import metrics, ops, residue_constants as rc
    Lab = scorer.Lab
    gt = scorer.gt_atom14.cpu()
    gseq = scorer.gt_seq.cpu()
    out = []
    for b in range(atom14.shape[0]):
        x = torch.cat([atom14[b].cpu(), gt[Lab:]], 0)
        aa = torch.cat([seq[b].cpu(), gseq[Lab:]], 0)
        m = torch.cat([torch.as_tensor(rc.restype_atom14_mask)[seq[b].cpu()].bool(), scorer.gt_exists.cpu()[Lab:].bool()], 0)
        to_s = lambda t: ''.join(rc.restypes[i] if i < 20 else 'X' for i in t.tolist())
        keep = scorer.gt_exists.cpu()[:Lab, 1].bool().numpy()
        assert keep.all()
        with warnings.catch_warnings():                      # (numpy warns about the mean of an empty region: the NaN is the point)
            warnings.simplefilter('ignore', RuntimeWarning)
            d = metrics.calc_ab_metrics(gt[:Lab, 1].double().numpy(), x[:Lab, 1].double().numpy(), scorer.cdr_def.cpu()[:Lab].numpy(), to_s(gseq[:Lab]),
                                        to_s(seq[b].cpu()))
        ch, ri = scorer.chain_id.cpu()[None], scorer.residx.cpu()[None]
        vio = metrics.violation_counts(x[None], m[None], aa[None], ch, ri)[0].tolist()
        cl = [int(v) for v in metrics.clash_counts(x[None], m[None], aa[None], ch, ri)]
        out.append((d, vio, cl))
    return out


def assert_scores_match_host(scorer, scores, atom14, seq, what):
    rows = scores.cpu().numpy()
    for b, (d, vio, cl) in enumerate(host_scores(scorer, atom14, seq)):
        for k, r in d.items():
            v = float(rows[b][col(k)])
            if r != r:
                assert v != v, (what, b, k)
            else:
                assert abs(v - r) <= (0.0 if k.endswith('AAR') else 1e-9 * max(1.0, abs(r))), (what, b, k, v, r)
        assert rows[b][14:17].tolist() == [float(v) for v in vio], (what, b, rows[b][14:17], vio)
        assert abs(rows[b][17] - cl[0]) <= cl[2] and abs(rows[b][18] - cl[1]) <= cl[2], (what, b, rows[b][17:19], cl)


def shipped_batch(D, n, seed=0):
    from abx_amd import features
    from abx_amd.data.antibody import load_complex
    cb = load_complex(os.path.join(GOLDEN, 'pdb', '6ct7_H_L_S.pdb'), seed=seed)
    one = {k: v.to(DEV) for k, v in cb.items() if torch.is_tensor(v)}
    L = one['seq'].shape[1]
    raw = {k: v.expand(n, *v.shape[1:]).contiguous() for k, v in one.items()}
    ids = list(range(n))
    batch = features.build_features(raw, D, generate_area='H3', noise=features.per_sample_init_noise(ids, L, seed, DEV))
    batch['_shared_context'] = True
    D.seed = seed
    return batch, torch.tensor(ids, device=DEV, dtype=torch.int64)


def test_sampler_scores_every_record_and_leaves_the_trajectory_alone(gpu_model, cfg):
    from abx_amd import metrics, sampler
    model, D = gpu_model
    batch, sid = shipped_batch(D, 3)
    assert {int(v) for v in batch['cdr_def'][0].unique()} >= {1, 3, 5, 8, 10, 12}
    scorer = metrics.DesignScorer(batch)
    plain = sampler.sample_fn(batch, cfg, D, model, mode='trajectory', num_t=4, sample_ids=sid)
    batch, sid = shipped_batch(D, 3)
    scored = sampler.sample_fn(batch, cfg, D, model, mode='trajectory', num_t=4, sample_ids=sid, scorer=scorer)
    assert len(plain) == len(scored) == 4 and all('scores' not in r for r in plain)
    base = scored[0]['scores'].data_ptr()
    for k, (a, b) in enumerate(zip(plain, scored)):
        for key in SHARED:
            assert torch.equal(a[key], b[key]), (k, key)
        s = b['scores']
        assert s.shape == (3, len(metrics.SCORE_COLUMNS)) and s.dtype == torch.float64
        assert s.data_ptr() == base + k * 3 * len(metrics.SCORE_COLUMNS) * 8          # rows of ONE table
        again = scorer.score(b['atom14_results'], b['seq'])
        assert torch.equal(again.view(torch.int64), s.view(torch.int64)), k
        assert_scores_match_host(scorer, s, b['atom14_results'], b['seq'], f'record {k}')
    last = sampler.sample_fn(shipped_batch(D, 3)[0], cfg, D, model, mode='design', num_t=4, sample_ids=sid, scorer=scorer)
    assert len(last) == 1 and torch.equal(last[0]['scores'].view(torch.int64), scored[-1]['scores'].view(torch.int64))


@pytest.mark.parametrize('collective', [False, True])
def test_design_driver_score_columns(tmp_path, monkeypatch, collective):
    """`abx_amd.design --score`: 3 + len(SCORE_COLUMNS) columns whose values are a DesignScorer run on the records the sampler returned,
    at print precision; without --score exactly three columns; in trajectory mode the second table.  collective = False: the shipped
    6ct7 complex in a plain process.  collective = True: the 1-rank RCCL path (--force_collective) on both shipped complexes, i.e. the
    scores as further columns of the set-level table and its one gather."""
    from abx_amd import design, metrics
    codes = CODES if collective else CODES[:1]
    seen = spy_on_sampler(monkeypatch, lambda batch, kw, traj: (metrics.DesignScorer(batch), traj))
    set_master_port(monkeypatch)
    common = pdb_args(codes) + ['--num_samples', '2', '--num_t', '4']
    if collective:
        common += ['--force_collective', '--min_block', '1']
    NC = len(metrics.SCORE_COLUMNS)

    def table(files, suffix, code):
        hit = [f for f in files if os.path.basename(f) == code + suffix]
        assert len(hit) == 1, (code, suffix, files)
        return [ln.split('\t') for ln in open(hit[0]).read().splitlines()]

    del seen[:]
    files = design.main(common + ['--score', '--output_dir', str(tmp_path / 'scored')])
    assert not [f for f in files if f.endswith('_trajectory_scores.tsv')] and len(seen) == len(codes) * (2 if collective else 1)
    plain_files = design.main(common + ['--output_dir', str(tmp_path / 'plain')])
    for code in codes:
        lines = table(files, '_designs.tsv', code)
        assert lines[0] == ['sample', 'mean_pLDDT', 'antibody_sequence'] + list(metrics.SCORE_COLUMNS)
        assert len(lines) == 3 and all(len(r) == 3 + NC for r in lines)
        # the records of this complex, one sampler call per work unit (sample block) in sample order
        runs = [(sc, tr) for sc, tr in seen[:len(codes) * (2 if collective else 1)] if sc.gt_atom14.shape[0] == (231 if code.startswith('6ct7') else 259)]
        want = torch.cat([sc.score(tr[-1]['atom14_results'], tr[-1]['seq']) for sc, tr in runs]).cpu().tolist()
        assert len(want) == 2
        for i, r in enumerate(lines[1:]):
            assert r[0] == str(i) and r[3:] == metrics.format_scores(want[i]), (code, i, r[3:], metrics.format_scores(want[i]))
            assert all(np.isfinite(float(v)) for v in r[3:] if v != 'nan')
        assert (lines[1][3 + col('heavy_cdr3_Loop_RMSD')] == 'nan') == code.startswith('6ct7')
        plain = table(plain_files, '_designs.tsv', code)
        assert len(plain) == 3 and all(len(r) == 3 for r in plain)
        assert [r[:3] for r in lines] == plain                              # same designs, same first three columns
    # trajectory mode: the second table, one line per (sample, step)
    del seen[:]
    files = design.main(common + ['--score', '--mode', 'trajectory', '--output_dir', str(tmp_path / 'traj')])
    for code in codes:
        tl = table(files, '_trajectory_scores.tsv', code)
        assert tl[0] == ['sample', 'step', 't'] + list(metrics.SCORE_COLUMNS) and len(tl) == 1 + 2 * 4
        runs = [tr for sc, tr in seen if sc.gt_atom14.shape[0] == (231 if code.startswith('6ct7') else 259)]
        recs = [torch.cat([tr[k]['scores'] for tr in runs]).cpu().tolist() for k in range(4)]
        for i in range(2):
            for k in range(4):
                row = tl[1 + i * 4 + k]
                assert row[:3] == [str(i), str(k), f'{runs[0][k]["time"]:.4f}'] and row[3:] == metrics.format_scores(recs[k][i]), (code, i, k)
        assert table(files, '_designs.tsv', code)[1][3:] == tl[4][3:]
