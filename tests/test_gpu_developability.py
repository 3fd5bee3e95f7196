"""GPU checks of the developability analysis (abx_developability_scores, csrc/developability.hip; abx_amd.developability.
DevelopabilityScorer): every column of the row and the per-residue table against the float64 / int64 host twin - equal, not close -,
the LDS chunks of the pair kernel, batch independence at the headline size, the edge cases of the radius, and the path through the
sampler and the design driver, where the surface kernel is shared with the interface and polar analyses."""
import os

import numpy as np
import pytest
import torch

from analysis_gpu_cases import (ALONE, CODES, DEV, driver_pair, l352_designs, names, pdb_args, runs_of, sample_tiny, sampler_pair,
                                set_master_port, spy_on_sampler, table_lines, tiny_batch, typed_or_gt, ops, gpu_model)  # noqa: F401  (ops, gpu_model: set up once per importing module)
import relax_cases as RC

pytestmark = pytest.mark.gpu

G = 7


def bits(t):
    return t.contiguous().view(torch.int64)


def batch_of(c, res_mask=None):
    """The un-batched complex of relax_cases.load_complex as a scorer takes it, on the device."""
    b = {'seq': c['aa'], 'atom14_gt_positions': c['x'].float(), 'atom14_gt_exists': c['mask'], 'anchor_flag': torch.zeros(c['Lab']),
         'chain_id': c['chain'], 'residx': c['residx'], 'cdr_def': c['cdr']}
    if res_mask is not None:
        b['mask'] = res_mask
    return {k: v.to(DEV) for k, v in b.items()}


def twin(c, x, mask, pts, seq=None, **kw):
    from abx_amd import developability as dv
    return dv.developability_host(x, mask, c['aa'] if seq is None else seq, c['Lab'], c['chain'], c['residx'], c['cdr'], region=c['mov'],
                                  points=pts, **kw)


def assert_equal_twin(row, rows, hrow, hrows, what):
    assert row.tolist() == hrow.tolist(), (what, row.tolist(), hrow.tolist())
    assert np.array_equal(rows.numpy(), hrows), (what, np.argwhere(rows.numpy() != hrows)[:8].tolist())


@pytest.mark.parametrize('code', ['6ct7', '6qd7'])
def test_rows_equal_the_host_twin(ops, code):
    """The wild type and three seeded perturbations in one batch (B = 4, L = 231 / 259): all 21 columns and the (L, 4) table equal the
    host twin's, with the scorer's own surface call and with the point counts handed over from InterfaceScorer.score; then with
    pred_mask NULL (the atoms of the residue types) and with a res_mask.  The host twin takes the device's point counts (their equality
    with interface_host is test_gpu_interface's subject); the wild type's are recomputed on the host as well."""
    from abx_amd import developability as dv, interface, residue_constants as rc
    c = RC.load_complex(code, 'h3')
    L, Lab = c['aa'].shape[0], c['Lab']
    xs = torch.stack([c['x'].float().double()] + [RC.perturb(c, s) for s in RC.SEEDS])
    B = xs.shape[0]
    x, sq = xs[:, :Lab].float().to(DEV), c['aa'][None, :Lab].repeat(B, 1).to(DEV)
    batch = batch_of(c)
    it = interface.InterfaceScorer(batch, region=c['mov'])
    own, shared = dv.DevelopabilityScorer(batch, region=c['mov']), dv.DevelopabilityScorer(batch, interface=it)
    assert shared.interface is it and own.interface is not it and torch.equal(shared.region, own.region)
    gt = c['mask'][None].repeat(B, 1, 1).to(DEV)
    pts = shared.new_points(B)
    it.score(x, sq, points=pts, mask=gt)
    rows_a, rows_b = torch.full((B, L, 4), -7.0, dtype=torch.float64, device=DEV), torch.full((B, L, 4), -7.0, dtype=torch.float64, device=DEV)
    a = own.score(x, sq, rows=rows_a, mask=gt)
    b = shared.score(x, sq, points=pts, rows=rows_b, mask=gt)
    assert a.shape == (B, 21) and a.dtype == torch.float64 and torch.equal(bits(a), bits(b)) and torch.equal(bits(rows_a), bits(rows_b))
    a, rows_a, hp = a.cpu(), rows_a.cpu(), pts.cpu()
    for k in range(B):
        hrow, hrows = twin(c, xs[k], c['mask'], hp[k])
        assert_equal_twin(a[k], rows_a[k], hrow, hrows, (code, k))
    print(code, 'sap_pos', a[:, 0].tolist(), 'sap_max_res', a[:, 3].tolist(), 'n_liab', a[:, 17].tolist(), 'atoms', a[:, 20].tolist())
    hrow, hrows = twin(c, xs[0], c['mask'], None)                               # points by interface_host
    assert_equal_twin(a[0], rows_a[0], hrow, hrows, (code, 'host points'))
    w = own.wild().cpu()[0]
    assert w.tolist() == a[0].tolist() == shared.wild(points=pts[:1].contiguous()).cpu()[0].tolist()
    # pred_mask NULL: the predicted rows have the atoms of their residue type
    typed = torch.cat([torch.as_tensor(rc.restype_atom14_mask)[c['aa'][:Lab]].bool(), c['mask'][Lab:]])
    rows_n = own.new_rows(2)
    pts_n = own.new_points(2)
    it.score(x[:2], sq[:2], points=pts_n)
    null = own.score(x[:2], sq[:2], rows=rows_n).cpu()
    for k in range(2):
        hrow, hrows = twin(c, xs[k], typed, pts_n[k].cpu())
        assert_equal_twin(null[k], rows_n[k].cpu(), hrow, hrows, (code, 'NULL mask', k))
    # res_mask: a removed row has no atoms, carries no charge and breaks the links through it
    keep = torch.ones(L, dtype=torch.bool)
    keep[[3, 50, Lab - 2]] = False
    cut = dv.DevelopabilityScorer(batch_of(c, res_mask=keep), region=c['mov'])
    rows_c, pts_c = cut.new_rows(1), cut.new_points(1)
    cut.interface.score(x[1:2], sq[1:2], points=pts_c, mask=gt[:1])
    got = cut.score(x[1:2], sq[1:2], rows=rows_c, mask=gt[:1]).cpu()
    hrow, hrows = twin(c, xs[1], c['mask'] & keep[:, None], pts_c[0].cpu())
    assert_equal_twin(got[0], rows_c[0].cpu(), hrow, hrows, (code, 'res_mask'))
    assert got[0, 20] < a[1, 20] and not rows_c[0, [3, 50, Lab - 2]].any()
    # rows of a wider table
    table = torch.full((B, 25), -1.0, dtype=torch.float64, device=DEV)
    shared.score(x, sq, points=pts, out=table[:, 2:23], mask=gt)
    t = table.cpu()
    assert torch.equal(bits(t[:, 2:23]), bits(a)) and bool((t[:, :2] == -1).all()) and bool((t[:, 23:] == -1).all())


def test_lds_chunks_give_the_same_rows(ops):
    """j_chunk = 64 on 6ct7: eight chunks of its 465 weighted atoms with a ragged last one (and seven tiles of 256 of its 1 663 atoms,
    the last one ragged too) give the rows of the default chunk; so do 1 and 100."""
    from abx_amd import developability as dv
    c = RC.load_complex('6ct7', 'h3')
    Lab = c['Lab']
    xs = torch.stack([c['x'].float().double(), RC.perturb(c, 5)])
    x, sq = xs[:, :Lab].float().to(DEV), c['aa'][None, :Lab].repeat(2, 1).to(DEV)
    sc = dv.DevelopabilityScorer(batch_of(c), region=c['mov'])
    gt = c['mask'][None].repeat(2, 1, 1).to(DEV)
    pts = sc.new_points(2)
    sc.interface.score(x, sq, points=pts, mask=gt)
    rows = sc.new_rows(2)
    base = sc.score(x, sq, points=pts, rows=rows, mask=gt)
    hrow, hrows, d = twin(c, xs[0], c['mask'], pts[0].cpu(), details=True)
    n_j = int((d['w'] != 0).sum())
    assert 6 * 64 < n_j <= 8 * 64 and n_j % 64 != 0 and base[0].cpu().tolist() == hrow.tolist() and hrow[20] == 1663
    for chunk in (64, 100, 1):
        r2 = sc.new_rows(2)
        got = sc.score(x, sq, points=pts, rows=r2, mask=gt, j_chunk=chunk)
        assert torch.equal(bits(got), bits(base)) and torch.equal(bits(r2), bits(rows)), chunk


def typed_mask(c):
    from abx_amd import residue_constants as rc
    return torch.as_tensor(rc.restype_atom14_mask)[c['aa']].bool()


def test_a_structure_does_not_depend_on_its_batch():
    """L = 352 synthetic workload, B = 100 perturbed copies: the rows of structures 0, 57 and 99 scored alone equal their rows in the
    batch bit for bit; a second call repeats the first; structure 57 equals the host twin."""
    from abx_amd import developability as dv
    cx, xh, x, sq, _ = l352_designs()
    (B, Lab), L = sq.shape, cx['seq'].shape[0]
    sc = dv.DevelopabilityScorer({k: v.to(DEV) for k, v in cx.items()}, region=cx['cdr_def'] == 5)
    pts = sc.new_points(B)
    sc.interface.score(x, sq, points=pts)
    rows = torch.full((B, L, 4), -7.0, dtype=torch.float64, device=DEV)
    full = sc.score(x, sq, points=pts, rows=rows)
    again = sc.score(x, sq, points=pts)
    assert full.shape == (B, 21) and torch.equal(bits(full), bits(again))
    h = full.cpu()
    print('L352 B=100: sap_pos', h[:, 0].min().item(), h[:, 0].max().item(), 'n_liab', h[:, 17].min().item(), h[:, 17].max().item(), 'atoms', h[0, 20].item())
    assert bool((h[:, 20] == h[0, 20]).all()) and len({tuple(r) for r in h.tolist()}) > 50
    for b in ALONE:
        r1 = torch.full((1, L, 4), -7.0, dtype=torch.float64, device=DEV)
        alone = sc.score(x[b:b + 1], sq[b:b + 1], points=pts[b:b + 1].contiguous(), rows=r1)
        assert torch.equal(bits(alone[0]), bits(full[b])) and torch.equal(bits(r1[0]), bits(rows[b])), b
    xs = torch.cat([xh[57], cx['atom14_gt_positions'][Lab:].float()])
    hrow, hrows = dv.developability_host(xs, typed_or_gt(cx, Lab, typed=True), cx['seq'], Lab, cx['chain_id'], cx['residx'], cx['cdr_def'],
                                         region=cx['cdr_def'] == 5, points=pts[57].cpu())
    assert_equal_twin(h[57], rows[57].cpu(), hrow, hrows, 'L352 structure 57')


def test_radius_and_weight_edge_cases(ops):
    """A radius below every distance (SAP_i = w_i), one beyond every distance (every atom carries the structure's sum) and all-Gly tokens
    (no weighted atom: the pair kernel must not read the empty list) against the twin."""
    from abx_amd import developability as dv
    c = RC.load_complex('6ct7', 'h3')
    L, Lab = c['aa'].shape[0], c['Lab']
    xs = torch.stack([c['x'].float().double(), RC.perturb(c, 6)])
    x, sq = xs[:, :Lab].float().to(DEV), c['aa'][None, :Lab].repeat(2, 1).to(DEV)
    typed = torch.cat([typed_mask(c)[:Lab], c['mask'][Lab:]])
    for radius in (1e-3, 1e4):
        sc = dv.DevelopabilityScorer(batch_of(c), region=c['mov'], radius=radius)
        pts, rows = sc.new_points(2), sc.new_rows(2)
        sc.interface.score(x, sq, points=pts)
        got = sc.score(x, sq, points=pts, rows=rows).cpu()
        for k in range(2):
            hrow, hrows, d = twin(c, xs[k], typed, pts[k].cpu(), radius=radius, details=True)
            assert_equal_twin(got[k], rows[k].cpu(), hrow, hrows, (radius, k))
            total = int(d['w'].sum())
            assert got[k, 0] == (np.maximum(d['w'], 0).sum() if radius < 1 else max(total, 0) * hrow[20]) / float(1 << 30)
    sc = dv.DevelopabilityScorer(batch_of(c), region=c['mov'])
    gly = torch.full_like(sq, G)
    pts, rows = sc.new_points(2), sc.new_rows(2)
    sc.interface.score(x, gly, points=pts)
    got = sc.score(x, gly, points=pts, rows=rows).cpu()
    seq = c['aa'].clone()
    seq[:Lab] = G
    gmask = torch.cat([torch.tensor([True] * 4 + [False] * 10)[None].repeat(Lab, 1), c['mask'][Lab:]])
    hrow, hrows = twin(c, xs[1], gmask, pts[1].cpu(), seq=seq)
    assert_equal_twin(got[1], rows[1].cpu(), hrow, hrows, 'all Gly')
    assert got[1, :6].tolist() == [0.0] * 6 and got[1, 20] == 4 * Lab and got[1, 6:20].tolist() == [0.0] * 14


def test_sampler_scores_the_last_record(gpu_model, cfg):
    """sample_fn(developability=) on the tiny workload: the plain trajectory is unchanged, 'developability' sits on the last record only
    and equals a direct .score() of that record; with a relaxer also 'developability_relaxed', with want_rows 'developability_rows';
    sharing the interface scorer changes no table."""
    from abx_amd import developability as dv, interface, relax
    b, sid = tiny_batch(gpu_model)
    B, L = sid.shape[0], b['seq'].shape[1]
    ND = len(dv.DEVELOPABILITY_COLUMNS)
    sc = dv.DevelopabilityScorer(b)
    _, scored = sampler_pair(gpu_model, cfg, b, sid, ('developability',), developability=sc)
    last = scored[-1]
    assert last['developability'].shape == (B, ND) and last['developability'].dtype == torch.float64
    assert not {'developability_relaxed', 'developability_rows', 'interface'} & set(last)
    assert torch.equal(bits(sc.score(last['atom14_results'], last['seq'])), bits(last['developability']))
    it = interface.InterfaceScorer(b)
    sh = dv.DevelopabilityScorer(b, interface=it)
    sh.want_rows = True
    full = sample_tiny(gpu_model, cfg, b, sid, mode='design', developability=sh, interface=it, relaxer=relax.ViolationRelaxer(b))
    assert len(full) == 1
    rec = full[0]
    assert torch.equal(bits(rec['developability']), bits(last['developability'])) and rec['developability_rows'].shape == (B, L, 4)
    rows = sh.new_rows(B)
    assert torch.equal(bits(sh.score(rec['atom14_results'], rec['seq'], rows=rows)), bits(rec['developability']))
    assert torch.equal(bits(rows), bits(rec['developability_rows']))
    assert torch.equal(bits(sh.score(rec['atom14_relaxed'], rec['seq'])), bits(rec['developability_relaxed']))
    assert torch.equal(bits(it.score(rec['atom14_results'], rec['seq'])), bits(rec['interface']))
    row = rec['developability'].cpu()
    print('tiny workload, developability rows', row.tolist(), 'wild', sc.wild().cpu().tolist())
    assert bool((row[:, 20] > 0).all()) and sc.wild().shape == (1, ND)


@pytest.mark.parametrize('collective', [False, True])
def test_design_driver_writes_the_developability_table(tmp_path, monkeypatch, collective):
    """`abx_amd.design --developability`: <complex>_developability.tsv with the header, the wild line and one line per sample whose fields
    are the sampler's records at print precision; every other file of the run is byte-identical to the run without the flag.
    collective = False: the shipped 6ct7 complex with --relax --developability_rows (the relaxed columns follow, the per-residue table is
    written).  collective = True: the 1-rank RCCL path on both shipped complexes, the table as further columns of the set-level gather."""
    from abx_amd import developability as dv
    out, codes, N, seen = driver_pair(tmp_path, monkeypatch, 'developability', ['--developability'] + ([] if collective else ['--developability_rows']),
                                        collective, plain_extra=['--relax', '--relax_iters', '20'],
                                        extra_files=[] if collective else [CODES[0] + '_developability_rows.npy'])
    ND, NDELTA = len(dv.DEVELOPABILITY_COLUMNS), len(dv.DELTA_COLUMNS)
    for code in codes:
        lines = table_lines(out, code, 'developability')
        head = ['sample'] + list(dv.DEVELOPABILITY_COLUMNS) + ['delta_' + c for c in dv.DELTA_COLUMNS]
        assert lines[0] == head + ([] if collective else [c + '_relaxed' for c in dv.DEVELOPABILITY_COLUMNS])
        assert len(lines) == 1 + 1 + N and all(len(r) == len(lines[0]) for r in lines)
        runs = runs_of(seen, code, collective)
        wild = runs[0][0].wild().cpu()[0].tolist()
        assert lines[1][:1 + ND] == ['wild'] + dv.format_developability(wild)
        assert lines[1][1 + ND:1 + ND + NDELTA] == dv.format_delta(wild, wild) == ['+0.000'] * 4 + ['+0'] * 4
        assert wild[20] == (1663 if code.startswith('6ct7') else 1722) and f'{wild[0]:.2f}' == ('55.07' if code.startswith('6ct7') else '80.01')
        rows = torch.cat([tr[-1]['developability'] for _, tr in runs]).cpu().tolist()
        for i, r in enumerate(lines[2:]):
            assert r[0] == str(i) and r[1:1 + ND] == dv.format_developability(rows[i]), (code, i, r)
            assert r[1 + ND:1 + ND + NDELTA] == dv.format_delta(rows[i], wild), (code, i, r)
        if not collective:
            relaxed = runs[0][1][-1]['developability_relaxed'].cpu().tolist()
            assert lines[1][1 + ND + NDELTA:] == ['nan'] * ND
            for i, r in enumerate(lines[2:]):
                assert r[1 + ND + NDELTA:] == dv.format_developability(relaxed[i]) and 'nan' not in r, (code, i)
            per_res = np.load(os.path.join(out, code + '_developability_rows.npy'))
            want = runs[0][1][-1]['developability_rows'].cpu().numpy()
            assert per_res.dtype == np.float64 and per_res.shape == (N, 231, 4) and np.array_equal(per_res, want)
            assert not per_res[:, runs[0][0].Lab:].any()
            assert [sum(bin(int(m)).count('1') for m in per_res[i, :, 2]) for i in range(N)] == [int(r[17]) for r in rows]


def test_one_surface_call_serves_three_tables(tmp_path, monkeypatch):
    """--interface --polar --developability: abx_interface_scores runs once per structure set (once inside the sampler call for the
    designs, once after it for the wild type), and the three tables are those of three separate runs byte for byte."""
    from abx_amd import design, ops as _ops
    set_master_port(monkeypatch)
    calls = []
    real = _ops.interface_scores

    def counted(*a, **kw):
        calls.append(a[0].shape[0])
        return real(*a, **kw)

    monkeypatch.setattr(_ops, 'interface_scores', counted)
    inside = spy_on_sampler(monkeypatch, lambda batch, kw, traj: len(calls))
    common = pdb_args(CODES[:1]) + ['--num_samples', '2', '--num_t', '3']
    flags = ['--interface', '--polar', '--developability']
    files = design.main(common + flags + ['--output_dir', str(tmp_path / 'all')])
    assert inside == [1] and calls == [2, 1], (inside, calls)
    assert [n for n in names(files) if n.endswith('.tsv')] == sorted(f'{CODES[0]}_{t}.tsv' for t in ('designs', 'developability', 'interface', 'polar'))
    for flag in flags:
        del calls[:], inside[:]
        design.main(common + [flag, '--output_dir', str(tmp_path / flag[2:])])
        assert inside == [1] and calls == [2, 1], (flag, inside, calls)
        name = f'{CODES[0]}_{flag[2:]}.tsv'
        assert open(tmp_path / 'all' / name, 'rb').read() == open(tmp_path / flag[2:] / name, 'rb').read(), flag
