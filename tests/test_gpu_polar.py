"""GPU checks of the polar-contact analysis (abx_polar_scores, csrc/polar.hip; abx_amd.polar.PolarScorer): the bonds of every atom14
slot and every count column against the float64 host twin - equal, not close -, the input conventions shared with
abx_interface_scores, batch independence at the headline size, and the path through the sampler and the design driver."""
import os

import numpy as np
import pytest
import torch

from analysis_gpu_cases import (ALONE, CODES, DEV, IDX13, assert_row as assert_columns, driver_pair, l352_designs, runs_of,
                                sample_tiny, sampler_pair, structure_inputs, table_lines, tiny_batch, typed_or_gt, ops, gpu_model)  # noqa: F401  (ops, gpu_model: set up once per importing module)
import relax_cases as RC

pytestmark = pytest.mark.gpu

COUNT = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13]
AREA = [10, 11]
P = 128


def gpu_scores(ops, c, xs, Lp=None, mask='gt', points=True, want=True, **kw):
    """abx_interface_scores for the point counts, then abx_polar_scores, on structures xs (B,L,14,3) of complex c (rows >= Lp come from
    the crystal structure, which xs holds there).  -> (rows, bonds, per-residue rows, points) on the host."""
    from abx_amd import interface, polar
    B, L = xs.shape[0], c['aa'].shape[0]
    x, sq, cx, m, region = structure_inputs(c, xs, Lp, mask)
    pts = None
    if points:
        pts = torch.full((B, L, 14, 2), -7, dtype=torch.int32, device=DEV)
        ops.interface_scores(x, sq, *cx, interface.sphere_points(P, DEV), Lab=c['Lab'], mask=m, points=pts, res_mask=kw.get('res_mask'))
    bonds = torch.full((B, L, 14, 2), -7, dtype=torch.int32, device=DEV) if want else None
    rows = torch.full((B, L, 4), -7, dtype=torch.int32, device=DEV) if want else None
    kw.setdefault('region', region)
    row = ops.polar_scores(x, sq, *cx, polar.polar_table_on(DEV), Lab=c['Lab'], mask=m, points=pts, n_points=P, bonds=bonds, rows=rows, **kw)
    return row.cpu(), (bonds.cpu() if want else None), (rows.cpu() if want else None), (pts.cpu() if points else None)


def assert_row(got, want, what):
    """count columns equal; areas to 1e-10 relative (the order of the sums is the only freedom)."""
    assert_columns(got, want, COUNT, AREA, 1e-10, what)


@pytest.mark.parametrize('code,sel', RC.MOVABLE_SETS)
def test_bonds_equal_the_host_twin(ops, code, sel):
    """The wild type and the three seeded perturbations of every movable set in one batch (B = 4, L = 231 / 259): the same-side and
    cross-side bonds of EVERY slot of every structure equal the host twin's, so do the count columns and the per-residue table; the two
    areas to 1e-10.  Repeated with hb_angle = 120 degrees and hb_max = 3.2 A.  The host twin takes the device's point counts (their
    equality with interface_host is test_gpu_interface's subject); the wild type's are recomputed on the host as well."""
    from abx_amd import polar
    c = RC.load_complex(code, sel)
    xs = torch.stack([c['x'].float().double()] + [RC.perturb(c, s) for s in RC.SEEDS])
    for kw in (dict(), dict(hb_angle=120.0, hb_max=3.2)):
        row, bonds, rows, pts = gpu_scores(ops, c, xs, **kw)
        for b in range(xs.shape[0]):
            hrow, hbonds, hd = polar.polar_host(xs[b], c['mask'], c['aa'], c['Lab'], region=c['mov'], points=pts[b], details=True, **kw)
            bad = torch.nonzero(bonds[b] != torch.from_numpy(hbonds))
            assert bad.shape[0] == 0, (code, sel, kw, b, bad[:8].tolist())
            assert torch.equal(bonds[b], torch.from_numpy(hbonds)) and torch.equal(rows[b], torch.from_numpy(hd['rows']))
            assert_row(row[b], hrow, (code, sel, kw, b))
            assert row[b, 13] == hrow[13] > 500 and int(bonds[b].sum()) == 2 * int(row[b, 12])
        print(code, sel, kw, 'hbond_int', row[:, 0].tolist(), 'total', row[:, 12].tolist(), 'salt', row[:, 4].tolist(), 'unsat', row[:, 8].tolist(),
              'intra_region', row[:, 3].tolist(), 'dsasa_polar', row[:, 10].tolist())
        if not kw:
            hrow = polar.polar_host(xs[0], c['mask'], c['aa'], c['Lab'], region=c['mov'], n_points=P)[0]      # points by interface_host
            assert_row(row[0], hrow, (code, sel, 'host points'))
            base = row
    assert bool((row[:, 12] < base[:, 12]).all())                               # the stricter rule keeps fewer bonds


def test_conventions_shared_with_the_interface_analysis(ops):
    """Lpred == Lab (antigen rows from the ground truth) and Lpred == L; pred_mask given and NULL; res_mask; points == NULL; region ==
    NULL; out_stride > 14 and successive calls into one table."""
    from abx_amd import polar, residue_constants as rc
    c = RC.load_complex('6ct7', 'h3')
    L, Lab = c['aa'].shape[0], c['Lab']
    xs = torch.stack([c['x'].float().double(), RC.perturb(c, 5)])
    full, bonds_full, rows_full, pts_full = gpu_scores(ops, c, xs)
    ab, bonds_ab, rows_ab, _ = gpu_scores(ops, c, xs, Lp=Lab)
    assert torch.equal(full.view(torch.int64), ab.view(torch.int64)) and torch.equal(bonds_full, bonds_ab) and torch.equal(rows_full, rows_ab)
    # NULL pred_mask: predicted rows have the atoms of their residue type, the others those of the ground truth
    typed = torch.as_tensor(rc.restype_atom14_mask)[c['aa']].bool()
    for Lp in (Lab, L):
        m = torch.cat([typed[:Lp], c['mask'][Lp:]])[None].repeat(2, 1, 1)
        given, bonds_g, _, pts_g = gpu_scores(ops, c, xs, Lp=Lp, mask=m)
        null, bonds_n, _, _ = gpu_scores(ops, c, xs, Lp=Lp, mask=None)
        assert torch.equal(given.view(torch.int64), null.view(torch.int64)) and torch.equal(bonds_g, bonds_n), Lp
        hrow, hbonds = polar.polar_host(xs[1], m[0], c['aa'], Lab, region=c['mov'], points=pts_g[1])
        assert torch.equal(bonds_n[1], torch.from_numpy(hbonds))
        assert_row(null[1], hrow, ('NULL mask', Lp))
    # res_mask: a removed row has no atoms (an antibody and an antigen row that are bonded across the interface)
    cross = torch.nonzero(bonds_full[0, ..., 1].sum(1))[:, 0]
    ra, rb = int(cross[cross < Lab][0]), int(cross[cross >= Lab][0])
    keep = torch.ones(L, dtype=torch.bool)
    keep[[ra, rb]] = False
    cut, bonds_cut, rows_cut, pts_cut = gpu_scores(ops, c, xs, res_mask=keep.to(DEV))
    assert not bonds_cut[:, [ra, rb]].any() and not rows_cut[:, [ra, rb]].any() and bool((cut[:, 13] < full[:, 13]).all())
    hrow, hbonds = polar.polar_host(xs[0], c['mask'] & keep[:, None], c['aa'], Lab, region=c['mov'], points=pts_cut[0])
    assert torch.equal(bonds_cut[0], torch.from_numpy(hbonds))
    assert_row(cut[0], hrow, 'res_mask')
    assert cut[0, 0] < full[0, 0]
    # no point counts: columns 6-11 are -1 (and the unsatisfied column of the per-residue table), the others do not change
    bare, bonds_bare, rows_bare, _ = gpu_scores(ops, c, xs, points=False)
    others = [0, 1, 2, 3, 4, 5, 12, 13]
    assert bool((bare[:, 6:12] == -1).all()) and torch.equal(bare[:, others], full[:, others]) and torch.equal(bonds_bare, bonds_full)
    assert torch.equal(rows_bare[..., :3], rows_full[..., :3]) and bool((rows_bare[..., 3] == -1).all())
    # no region: its four columns are 0, the others do not change
    nore, _, _, _ = gpu_scores(ops, c, xs, want=False, region=None)
    rest = [0, 1, 4, 6, 7, 8, 10, 11, 12, 13]
    assert nore[:, [2, 3, 5, 9]].abs().max() == 0 and torch.equal(nore[:, rest].view(torch.int64), full[:, rest].view(torch.int64))
    assert full[0, 2] > 0 and full[0, 3] > 0 and full[0, 9] > 0
    # rows of a wider table, and successive calls into one table
    table = torch.full((4, 18), -1.0, dtype=torch.float64, device=DEV)
    gpu_scores(ops, c, xs, want=False, out=table[:2, 2:16])
    gpu_scores(ops, c, xs[[1, 0]], want=False, out=table[2:, 2:16])
    t = table.cpu()
    assert torch.equal(t[:2, 2:16].view(torch.int64), full.view(torch.int64)) and torch.equal(t[[3, 2], 2:16].view(torch.int64), full.view(torch.int64))
    assert bool((t[:, :2] == -1).all()) and bool((t[:, 16:] == -1).all())
    # a 9 A "salt bridge": row pairs with several qualifying atom pairs (Arg x Asp: up to six) still count once
    wide, _, rows_wide, pts_w = gpu_scores(ops, c, xs, salt=9.0)
    for b in (0, 1):
        hrow, _, hd = polar.polar_host(xs[b], c['mask'], c['aa'], Lab, region=c['mov'], points=pts_w[b], salt=9.0, details=True)
        assert_row(wide[b], hrow, 'salt = 9')
        assert torch.equal(rows_wide[b], torch.from_numpy(hd['rows']))
    assert wide[0, 4] == 4 and full[0, 4] == 1                                  # the crystal structure (host twin)


def test_a_structure_does_not_depend_on_its_batch():
    """L = 352 synthetic workload, B = 100 perturbed copies: rows, bonds and per-residue tables are bit-identical alone, in a chunk of 13
    and in the batch of 100; a second call repeats the first bit for bit; one structure against the host twin."""
    from abx_amd import polar
    cx, xh, x, sq, _ = l352_designs()
    (B, Lab), L = sq.shape, cx['seq'].shape[0]
    sc = polar.PolarScorer({k: v.to(DEV) for k, v in cx.items()}, region=cx['cdr_def'] == 5)
    pts = sc.new_points(B)
    sc.interface.score(x, sq, points=pts)
    new = lambda n: (torch.full((n, L, 14, 2), -7, dtype=torch.int32, device=DEV), torch.full((n, L, 4), -7, dtype=torch.int32, device=DEV))
    bonds, rows = new(B)
    full = sc.score(x, sq, points=pts, bonds=bonds, rows=rows)
    again = sc.score(x, sq, points=pts)
    assert full.shape == (B, len(polar.POLAR_COLUMNS)) and full.dtype == torch.float64
    assert torch.equal(full.view(torch.int64), again.view(torch.int64))
    h = full.cpu()
    print('L352 B=100: hbond_total', h[:, 12].min().item(), h[:, 12].max().item(), 'hbond_int', h[:, 0].min().item(), h[:, 0].max().item(),
          'polar', h[0, 13].item(), 'unsat', h[:, 8].min().item(), h[:, 8].max().item())
    assert bool((h[:, 13] == h[0, 13]).all()) and len({tuple(r) for r in h.tolist()}) > 50
    b13, r13 = new(13)
    chunk = sc.score(x[IDX13], sq[IDX13], points=pts[IDX13].contiguous(), bonds=b13, rows=r13)
    for j, b in enumerate(IDX13):
        assert torch.equal(chunk[j].view(torch.int64), full[b].view(torch.int64)) and torch.equal(b13[j], bonds[b]) and torch.equal(r13[j], rows[b]), b
    for b in ALONE:
        b1, r1 = new(1)
        alone = sc.score(x[b:b + 1], sq[b:b + 1], points=pts[b:b + 1].contiguous(), bonds=b1, rows=r1)
        assert torch.equal(alone[0].view(torch.int64), full[b].view(torch.int64)) and torch.equal(b1[0], bonds[b]) and torch.equal(r1[0], rows[b]), b
    xs = torch.cat([xh[57], cx['atom14_gt_positions'][Lab:].float()])
    hrow, hbonds, hd = polar.polar_host(xs, typed_or_gt(cx, Lab), cx['seq'], Lab, region=cx['cdr_def'] == 5, points=pts[57].cpu(), details=True)
    assert torch.equal(bonds[57].cpu(), torch.from_numpy(hbonds)) and torch.equal(rows[57].cpu(), torch.from_numpy(hd['rows']))
    assert_row(h[57], hrow, 'L352 structure 57')


def test_scorer_shares_the_interface_scorer():
    """A PolarScorer given an InterfaceScorer yields the same rows as one that builds its own, from that scorer's point counts or its own."""
    from abx_amd import interface, polar
    c = RC.load_complex('6ct7', 'h3')
    L, Lab = c['aa'].shape[0], c['Lab']
    batch = {'seq': c['aa'].to(DEV), 'atom14_gt_positions': c['x'].float().to(DEV), 'atom14_gt_exists': c['mask'].to(DEV),
             'anchor_flag': torch.zeros(Lab, device=DEV)}
    xs = torch.stack([c['x'].float(), RC.perturb(c, 6).float()])[:, :Lab].to(DEV)
    sq = c['aa'][None, :Lab].repeat(2, 1).to(DEV)
    it = interface.InterfaceScorer(batch, region=c['mov'])
    own, shared = polar.PolarScorer(batch, region=c['mov']), polar.PolarScorer(batch, interface=it)
    assert shared.interface is it and own.interface is not it and torch.equal(shared.region, own.region)
    pts = shared.new_points(2)
    irow = it.score(xs, sq, points=pts)
    a, b, d = own.score(xs, sq), shared.score(xs, sq), shared.score(xs, sq, points=pts)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and torch.equal(a.view(torch.int64), d.view(torch.int64))
    assert float(((a[:, 10] + a[:, 11]) - irow[:, 3]).abs().max()) <= 1e-9
    w = own.wild().cpu()[0]
    assert torch.equal(w.view(torch.int64), shared.wild().cpu()[0].view(torch.int64))
    assert w[[13, 12, 0, 2, 3, 4, 6, 7, 8, 9]].tolist() == [629, 234, 9, 2, 5, 1, 47, 17, 3, 1]      # the crystal structure (test_polar_host)


def test_sampler_scores_the_last_record(gpu_model, cfg):
    """sample_fn(polar=) on the tiny workload: 'polar' sits on the last record only and equals a direct .score() of that record; with a
    relaxer also 'polar_relaxed', with want_rows 'polar_bonds' / 'polar_rows'; sharing the interface scorer changes neither table;
    with polar=None the records have exactly today's keys."""
    from abx_amd import interface, polar, relax
    b, sid = tiny_batch(gpu_model)
    B = sid.shape[0]
    it = interface.InterfaceScorer(b)
    sc, relaxer = polar.PolarScorer(b, interface=it), relax.ViolationRelaxer(b)
    sc.want_rows = True
    L = b['seq'].shape[1]
    new = ('polar', 'polar_relaxed', 'polar_bonds', 'polar_rows', 'interface', 'interface_relaxed')
    _, scored = sampler_pair(gpu_model, cfg, b, sid, new, polar=sc, interface=it, relaxer=relaxer)
    last = scored[-1]
    NP = len(polar.POLAR_COLUMNS)
    assert last['polar'].shape == last['polar_relaxed'].shape == (B, NP) and last['polar'].dtype == torch.float64
    assert last['polar_bonds'].shape == (B, L, 14, 2) and last['polar_rows'].shape == (B, L, 4)
    bonds, rows = torch.empty_like(last['polar_bonds']), torch.empty_like(last['polar_rows'])
    direct = sc.score(last['atom14_results'], last['seq'], bonds=bonds, rows=rows)
    assert torch.equal(direct.view(torch.int64), last['polar'].view(torch.int64))
    assert torch.equal(bonds, last['polar_bonds']) and torch.equal(rows, last['polar_rows'])
    assert torch.equal(sc.score(last['atom14_relaxed'], last['seq']).view(torch.int64), last['polar_relaxed'].view(torch.int64))
    assert torch.equal(it.score(last['atom14_results'], last['seq']).view(torch.int64), last['interface'].view(torch.int64))
    assert torch.equal(it.score(last['atom14_relaxed'], last['seq']).view(torch.int64), last['interface_relaxed'].view(torch.int64))
    design = sample_tiny(gpu_model, cfg, b, sid, mode='design', polar=polar.PolarScorer(b))
    assert len(design) == 1 and not {'polar_relaxed', 'polar_bonds', 'polar_rows', 'interface'} & set(design[0])
    assert torch.equal(design[0]['polar'].view(torch.int64), last['polar'].view(torch.int64))
    row = last['polar'].cpu()
    print('tiny workload, polar rows', row.tolist(), 'wild', sc.wild().cpu().tolist())
    assert bool((row[:, 13] > 0).all()) and bool((row[:, 6:12] >= 0).all()) and sc.wild().shape == (1, NP)
    assert bool((last['polar_bonds'].sum((1, 2, 3)).cpu() == 2 * row[:, 12].long()).all())


@pytest.mark.parametrize('collective', [False, True])
def test_design_driver_writes_the_polar_table(tmp_path, monkeypatch, collective):
    """`abx_amd.design --polar`: <complex>_polar.tsv with the header, the wild line and one line per sample whose fields are the sampler's
    records at print precision; every other file of the run is byte-identical to the run without the flag.  collective = False: the
    shipped 6ct7 complex with --relax --interface --polar_rows (the relaxed columns follow, the per-residue table is written).
    collective = True: the 1-rank RCCL path on both shipped complexes, the table as further columns of the set-level gather."""
    from abx_amd import polar
    out, codes, N, seen = driver_pair(tmp_path, monkeypatch, 'polar', ['--polar'] + ([] if collective else ['--polar_rows']), collective,
                                        plain_extra=['--relax', '--interface'], extra_files=[] if collective else [CODES[0] + '_polar_rows.npy'])
    NP, ND = len(polar.POLAR_COLUMNS), len(polar.DELTA_COLUMNS)
    for code in codes:
        lines = table_lines(out, code, 'polar')
        head = ['sample'] + list(polar.POLAR_COLUMNS) + ['delta_' + c for c in polar.DELTA_COLUMNS]
        assert lines[0] == head + ([] if collective else [c + '_relaxed' for c in polar.POLAR_COLUMNS])
        assert len(lines) == 1 + 1 + N and all(len(r) == len(lines[0]) for r in lines)
        runs = runs_of(seen, code, collective)
        wild = runs[0][0].wild().cpu()[0].tolist()
        assert lines[1][:1 + NP] == ['wild'] + polar.format_polar(wild) and lines[1][1 + NP:1 + NP + ND] == polar.format_delta(wild, wild)
        assert lines[1][1 + NP:1 + NP + ND] == ['+0'] * 6 + ['+0.00'] * 2
        assert wild[0] == (9 if code.startswith('6ct7') else 0) and wild[12] == 234            # the crystal structures (test_polar_host)
        rows = torch.cat([tr[-1]['polar'] for _, tr in runs]).cpu().tolist()
        for i, r in enumerate(lines[2:]):
            assert r[0] == str(i) and r[1:1 + NP] == polar.format_polar(rows[i]), (code, i, r)
            assert r[1 + NP:1 + NP + ND] == polar.format_delta(rows[i], wild), (code, i, r)
            k0, k10 = polar.POLAR_COLUMNS.index('n_hbond_int'), polar.POLAR_COLUMNS.index('dsasa_polar')
            assert int(r[1 + NP]) == int(rows[i][k0]) - int(wild[k0]) and abs(float(r[1 + NP + 6]) - (rows[i][k10] - wild[k10])) <= 0.005
        if not collective:
            relaxed = runs[0][1][-1]['polar_relaxed'].cpu().tolist()
            assert lines[1][1 + NP + ND:] == ['nan'] * NP
            for i, r in enumerate(lines[2:]):
                assert r[1 + NP + ND:] == polar.format_polar(relaxed[i]), (code, i)
            per_res = np.load(os.path.join(out, code + '_polar_rows.npy'))
            want = runs[0][1][-1]['polar_rows'].cpu().numpy()
            assert per_res.dtype == np.int16 and per_res.shape == (N, 231, 4) and np.array_equal(per_res, want)
            bonds = runs[0][1][-1]['polar_bonds'].cpu().numpy()
            assert np.array_equal(per_res[..., 0], bonds[..., 1].sum(2)) and np.array_equal(per_res[..., 1], bonds[..., 0].sum(2))
            assert per_res[..., 3].sum(1).tolist() == [int(r[8]) for r in rows] and per_res[..., 2].sum(1).tolist() == [2 * int(r[4]) for r in rows]
