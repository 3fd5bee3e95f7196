"""GPU checks of the torsion analysis (abx_torsion_scores, csrc/torsions.hip; abx_amd.torsions.TorsionScorer): the counts, the ABEGO codes
and the flag words against the float64 host twin - equal, not close -, the angles and the mean columns to atan2's last bits, on chains
built from given dihedrals and on the shipped complexes (crystal, seeded perturbations, mutated versions); the conventions of the entry
(pred_mask, out rows, optional outputs, guard values), the edge shapes, batch independence, and the path through the sampler and the
design driver."""
import os

import numpy as np
import pytest
import torch

from analysis_gpu_cases import (ALONE, CODES, DEV, IDX13, driver_pair, l352_designs, runs_of, sampler_pair, table_lines, tiny_batch,
                                ops, gpu_model)  # noqa: F401  (ops, gpu_model: set up once per importing module)
import relax_cases as RC
import shape_cases as SC
import torsions_cases as TC

pytestmark = pytest.mark.gpu

GUARD = 64
NT = 25
ANGLE_TOL = 1e-9            # degrees: equal (x, y) bits leave atan2's last bits, about 1e-13; the bound of such columns in test_gpu_accuracy.py


def bits(t):
    return t.contiguous().view(torch.int64)


def cols(*names):
    from abx_amd import torsions
    return [torsions.TORSIONS_COLUMNS.index(n) for n in names]


def guarded(shape, dtype, fill):
    """(view, whole): a contiguous tensor of `shape` with GUARD elements of `fill` in front of and behind it."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return whole[GUARD:GUARD + n].view(*shape), whole


def guards_intact(whole, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[-GUARD:] == fill).all())


def device_batch(c, triples):
    """Antibody coordinates, tokens and atom masks of (x, tokens, mask) structures of complex c on the device."""
    Lab = c['Lab']
    x = torch.stack([t[0][:Lab] for t in triples]).float().to(DEV)
    sq = torch.stack([t[1][:Lab] for t in triples]).to(DEV)
    mask = torch.stack([t[2] for t in triples]).to(DEV)
    return x, sq, mask


def scored(sc, x, sq, mask=None):
    """(row, rows, classes) on the host, every output and the workspace between guard values."""
    from abx_amd import ops as _ops
    B = x.shape[0]
    out, out_w = guarded((B, NT), torch.float64, -7.0)
    rows, rows_w = guarded((B, sc.Lab, 8), torch.float64, -7.0)
    cl, cl_w = guarded((B, sc.Lab), torch.int32, -7)
    ws, ws_w = guarded((_ops.torsion_workspace_bytes(B, sc.Lab),), torch.uint8, 0xA5)
    got = sc.score(x, sq, rows=rows, classes=cl, out=out, mask=mask, workspace=ws)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert guards_intact(out_w, -7.0) and guards_intact(rows_w, -7.0) and guards_intact(cl_w, -7) and guards_intact(ws_w, 0xA5)
    return out.cpu().clone(), rows.cpu().clone(), cl.cpu().clone()


def assert_equal_twin(row, rows, classes, h, what):
    """Counts, codes and flag words equal; angles and mean columns within ANGLE_TOL; nan positions equal."""
    from abx_amd import torsions
    row, rows, classes = row.numpy(), rows.numpy(), classes.numpy()
    cnt = [torsions.TORSIONS_COLUMNS.index(c) for c in torsions.COUNT_COLUMNS]
    mean = [torsions.TORSIONS_COLUMNS.index(c) for c in torsions.MEAN_COLUMNS]
    assert row[cnt].tolist() == h['row'][cnt].tolist(), (what, row[cnt].tolist(), h['row'][cnt].tolist())
    assert np.array_equal(classes, h['classes']), (what, np.argwhere(classes != h['classes'])[:8].tolist())
    assert np.array_equal(rows[:, 7], h['rows'][:, 7]), (what, np.argwhere(rows[:, 7] != h['rows'][:, 7])[:8].tolist())
    for got, want in ((row[mean], h['row'][mean]), (rows[:, :7], h['rows'][:, :7])):
        assert np.array_equal(np.isnan(got), np.isnan(want)), what
        err = np.abs(got - want)[~np.isnan(want)]
        assert float(err.max(initial=0.0)) <= ANGLE_TOL, (what, float(err.max(initial=0.0)))


def test_built_chains_equal_the_twin(ops):
    """The five built chains in one batch (B = 5, Lab = 8): A, B, G, E and the helix with one cis and one twisted link."""
    from abx_amd import torsions
    chains = TC.built_chains()
    for k, ch in enumerate(chains):
        c = TC.chain_complex(ch)
        sc = torsions.TorsionScorer(SC.batch_of(c, DEV), region=c['mov'])
        x, sq, mask = device_batch(c, [(torch.from_numpy(o['x']), c['aa'], c['mask']) for o in chains])
        row, rows, cl = scored(sc, x, sq, mask)
        for j, o in enumerate(chains):                  # chain j against wild type k
            h = TC.twin(c, torch.from_numpy(o['x']))
            assert h['n_borderline'] == 0
            assert_equal_twin(row[j], rows[j], cl[j], h, (k, j))
            assert ''.join(torsions.ABEGO[v] for v in cl[j].tolist()) == o['letters']
            assert row[j, cols('cis', 'twisted')].tolist() == [o['cis'], o['twisted']]
        assert row[k, cols('abego_same')] == row[k, cols('n_abego')] == TC.N_RES - 2
        if k:
            break                                       # (the other wild types repeat the first: two are enough)
    print('built chains, rows of chain 4:', rows[4, :, :3].tolist())


@pytest.fixture(scope='module')
def shipped(ops):
    """Per movable set: the complex, its seven structures, the device rows and the twin's - computed once, left unchanged."""
    from abx_amd import torsions
    out = {}
    for code, sel in RC.MOVABLE_SETS:
        c = RC.load_complex(code, sel)
        triples = TC.gpu_structures(c)
        sc = torsions.TorsionScorer(SC.batch_of(c, DEV), region=c['mov'])
        x, sq, mask = device_batch(c, triples)
        row, rows, cl = scored(sc, x, sq, mask)
        host = [TC.twin(c, t[0], mask=t[2], seq=t[1]) for t in triples]
        out[code, sel] = dict(c=c, sc=sc, x=x, sq=sq, mask=mask, row=row, rows=rows, cl=cl, host=host, triples=triples)
    return out


@pytest.mark.parametrize('code, sel', RC.MOVABLE_SETS)
def test_shipped_complexes_equal_the_twin(shipped, code, sel):
    """The wild type, three seeded perturbations and their mutated versions in one batch (B = 7; Lab = 221 and 227, ragged against the
    block of 256; the H -> L boundary; the three crystal cis peptides of 6qd7, one of them the designed O residue)."""
    from abx_amd import torsions
    s = shipped[code, sel]
    c = s['c']
    assert s['row'].shape == (7, NT) and c['Lab'] in (221, 227)
    for k, h in enumerate(s['host']):
        assert h['n_borderline'] == 0
        assert_equal_twin(s['row'][k], s['rows'][k], s['cl'][k], h, (code, sel, k))
    w = s['row'][0]
    assert w[cols('abego_same')] == w[cols('n_abego')] and w[cols('dphi_region', 'dpsi_region', 'domega_region', 'dbb_max_region', 'chi_mae_region')].tolist() == [0.0] * 5
    boundary = int(torch.nonzero(c['chain'][1:c['Lab']] != c['chain'][:c['Lab'] - 1])[0, 0]) + 1
    assert torch.isnan(s['rows'][:, boundary, [0, 2]]).all() and torch.isnan(s['rows'][:, boundary - 1, 1]).all()
    if code == '6qd7':
        assert w[cols('cis')] == 3 and 'O' in torsions.abego_string(s['cl'][0], c['mov'])
    assert torch.equal(bits(s['sc'].wild().cpu()[0]), bits(w))
    print(code, sel, 'wild', w.tolist(), 'abego', [torsions.abego_string(s['cl'][k], c['mov']) for k in range(7)])


def test_conventions(shipped):
    """pred_mask given equals NULL; out may be a slice of a wider table and takes successive calls; rows / classes may be NULL; no region
    gives region columns 0 / nan and leaves the others' bits unchanged."""
    from abx_amd import residue_constants as rc, torsions
    s = shipped['6ct7', 'h3']
    c, sc, x, sq = s['c'], s['sc'], s['x'], s['sq']
    B, Lab, L = x.shape[0], c['Lab'], c['aa'].shape[0]
    typed = torch.zeros(B, L, 14, dtype=torch.bool)
    typed[:, :Lab] = torch.as_tensor(rc.restype_atom14_mask)[sq.cpu()].bool()
    null = scored(sc, x, sq, None)
    given = scored(sc, x, sq, typed.to(DEV))
    for a, b in zip(null, given):
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)
    for k in (0, 2, 5):
        t = s['triples'][k]
        assert_equal_twin(null[0][k], null[1][k], null[2][k], TC.twin(c, t[0], mask=typed[k], seq=t[1]), ('typed', k))
    # rows of a wider table, filled by two successive calls; no optional output
    table = torch.full((B, NT + 5), -1.0, dtype=torch.float64, device=DEV)
    sc.score(x[:3], sq[:3], out=table[:3, 2:2 + NT], mask=s['mask'][:3])
    sc.score(x[3:], sq[3:], out=table[3:, 2:2 + NT], mask=s['mask'][3:])
    t = table.cpu()
    assert torch.equal(bits(t[:, 2:2 + NT]), bits(s['row'])) and bool((t[:, :2] == -1).all()) and bool((t[:, 2 + NT:] == -1).all())
    # no region
    none = torsions.TorsionScorer(SC.batch_of(c, DEV), region=torch.zeros(L, dtype=torch.bool))
    row = none.score(x, sq, mask=s['mask']).cpu()
    free = cols('n_links', 'cis', 'cis_nonpro', 'twisted', 'phi_pos')
    region = [k for k in range(NT) if k not in free]
    means = cols('dphi_region', 'dpsi_region', 'domega_region', 'dbb_max_region', 'chi_mae_region')
    assert torch.equal(bits(row[:, free]), bits(s['row'][:, free]))
    assert torch.isnan(row[:, means]).all() and bool((row[:, [k for k in region if k not in means]] == 0).all())


def test_edge_shapes(ops):
    """The tiny workload (Lab = 16); a one-residue and a two-residue chain: no class defined, no fault; a residue with CA masked out:
    its own and its neighbours' angles are undefined."""
    from abx_amd import torsions
    cx, xh, region = TC.tiny_structures()
    Lab = cx['anchor_flag'].shape[0]
    assert Lab == 16
    sc = torsions.TorsionScorer({k: v.to(DEV) for k, v in cx.items()}, region=region)
    row, rows, cl = scored(sc, xh.to(DEV), cx['seq'][None, :Lab].repeat(2, 1).to(DEV))
    for k in range(2):
        assert_equal_twin(row[k], rows[k], cl[k], TC.synthetic_twin(cx, xh[k], region), ('tiny', k))
    ch = TC.built_chains()[0]
    for n in (1, 2):
        c = TC.chain_complex(dict(ch, x=ch['x'][:n], mask=ch['mask'][:n]))
        sc = torsions.TorsionScorer(SC.batch_of(c, DEV), region=c['mov'])
        x, sq, mask = device_batch(c, [(c['x'], c['aa'], c['mask'])])
        row, rows, cl = scored(sc, x, sq, mask)
        assert_equal_twin(row[0], rows[0], cl[0], TC.twin(c, c['x']), ('chain of', n))
        assert cl.tolist() == [[0] * n] and row[0, cols('n_links', 'n_abego')].tolist() == [n - 1, 0] and bool(torch.isnan(row[0, cols('dbb_max_region')]).all()) == (n == 1)
    # CA masked out
    c = RC.load_complex('6ct7', 'h3')
    r = int(torch.nonzero(c['mov'])[1, 0])
    m = c['mask'].clone()
    m[r, 1] = False
    sc = torsions.TorsionScorer(SC.batch_of(c, DEV), region=c['mov'])
    x, sq, mask = device_batch(c, [(c['x'], c['aa'], m)])
    row, rows, cl = scored(sc, x, sq, mask)
    assert_equal_twin(row[0], rows[0], cl[0], TC.twin(c, c['x'], mask=m), 'CA masked')
    assert torch.isnan(rows[0, r, :3]).all() and torch.isnan(rows[0, r + 1, [0, 2]]).all() and torch.isnan(rows[0, r - 1, 1]).all()
    assert cl[0, r - 1:r + 2].tolist() == [0, 0, 0] and not torch.isnan(rows[0, r + 1, 1]) and not torch.isnan(rows[0, r - 1, 0])


def test_headline_size_and_batch_independence(ops):
    """L = 352 synthetic workload, B = 100 perturbed copies: structures 0, 57 and 99 are bit-identical alone, in IDX13 and in the full
    batch; a second call repeats the first; structure 57 equals the host twin."""
    from abx_amd import torsions
    cx, xh, x, sq, _ = l352_designs()
    (B, Lab) = sq.shape
    sc = torsions.TorsionScorer({k: v.to(DEV) for k, v in cx.items()}, region=cx['cdr_def'] == 5)
    rows, cl = sc.new_rows(B), sc.new_classes(B)
    full = sc.score(x, sq, rows=rows, classes=cl)
    again = sc.score(x, sq)
    assert full.shape == (B, NT) and torch.equal(bits(full), bits(again))
    idx = torch.tensor(IDX13, device=DEV)
    r13, c13 = sc.new_rows(13), sc.new_classes(13)
    part = sc.score(x[idx].contiguous(), sq[idx].contiguous(), rows=r13, classes=c13)
    for b in ALONE:
        r1, c1 = sc.new_rows(1), sc.new_classes(1)
        alone = sc.score(x[b:b + 1], sq[b:b + 1], rows=r1, classes=c1)
        k = IDX13.index(b)
        assert torch.equal(bits(alone[0]), bits(full[b])) and torch.equal(bits(r1[0]), bits(rows[b])) and torch.equal(c1[0], cl[b]), b
        assert torch.equal(bits(part[k]), bits(full[b])) and torch.equal(bits(r13[k]), bits(rows[b])) and torch.equal(c13[k], cl[b]), b
    h = TC.synthetic_twin(cx, xh[57], cx['cdr_def'] == 5)
    assert h['n_borderline'] == 0
    assert_equal_twin(full[57].cpu(), rows[57].cpu(), cl[57].cpu(), h, 'L352 structure 57')
    f = full.cpu()
    print('L352 B=100: twisted', f[:, 3].min().item(), f[:, 3].max().item(), 'phi_pos', f[:, 7].min().item(), f[:, 7].max().item())
    assert len({tuple(r) for r in torch.nan_to_num(f).tolist()}) > 50


def test_sampler_scores_the_last_record(gpu_model, cfg):
    """sample_fn(torsions=, relaxer=) on the tiny workload: the four keys sit on the last record only and equal a direct .score(); the
    plain records are unchanged (sampler_pair)."""
    from abx_amd import relax, torsions
    b, sid = tiny_batch(gpu_model)
    B, Lab = sid.shape[0], b['anchor_flag'].shape[1]
    sc = torsions.TorsionScorer(b)
    sc.want_rows = True
    _, got = sampler_pair(gpu_model, cfg, b, sid, ('torsions', 'torsions_classes', 'torsions_rows', 'torsions_relaxed'), torsions=sc,
                          relaxer=relax.ViolationRelaxer(b))
    last = got[-1]
    assert last['torsions'].shape == (B, NT) and last['torsions'].dtype == torch.float64
    assert last['torsions_classes'].shape == (B, Lab) and last['torsions_classes'].dtype == torch.int32 and last['torsions_rows'].shape == (B, Lab, 8)
    rows, cl = sc.new_rows(B), sc.new_classes(B)
    assert torch.equal(bits(sc.score(last['atom14_results'], last['seq'], rows=rows, classes=cl)), bits(last['torsions']))
    assert torch.equal(bits(rows), bits(last['torsions_rows'])) and torch.equal(cl, last['torsions_classes'])
    assert torch.equal(bits(sc.score(last['atom14_relaxed'], last['seq'])), bits(last['torsions_relaxed']))
    print('tiny workload, torsion rows', last['torsions'].cpu().tolist(), 'wild', sc.wild().cpu().tolist())
    assert sc.wild().shape == (1, NT)


@pytest.mark.parametrize('collective', [False, True])
def test_design_driver_writes_the_torsions_table(tmp_path, monkeypatch, collective):
    """`abx_amd.design --torsions`: <complex>_torsions.tsv with the header, the wild line and one line per sample whose fields are the
    sampler's records at print precision, the ABEGO string last; every other file of the run is byte-identical to the run without the
    flag.  collective = False: 6ct7 with --relax --torsions_rows; collective = True: the 1-rank RCCL path on both shipped complexes."""
    from abx_amd import torsions
    out, codes, N, seen = driver_pair(tmp_path, monkeypatch, 'torsions', ['--torsions'] + ([] if collective else ['--torsions_rows']), collective,
                                      plain_extra=['--relax', '--relax_iters', '20'], extra_files=[] if collective else [CODES[0] + '_torsions_rows.npy'])
    ND = len(torsions.DELTA_COLUMNS)
    for code in codes:
        lines = table_lines(out, code, 'torsions')
        head = ['sample'] + list(torsions.TORSIONS_COLUMNS) + ['delta_' + c for c in torsions.DELTA_COLUMNS]
        assert lines[0] == head + ([] if collective else [c + '_relaxed' for c in torsions.TORSIONS_COLUMNS]) + ['abego']
        assert len(lines) == 1 + 1 + N and all(len(r) == len(lines[0]) for r in lines)
        runs = runs_of(seen, code, collective)
        sc = runs[0][0]
        wcl = sc.new_classes(1)
        wild = sc.wild(classes=wcl).cpu()[0].tolist()
        region = sc.region.cpu().numpy()
        assert lines[1][:1 + NT] == ['wild'] + torsions.format_torsions(wild)
        assert lines[1][1 + NT:1 + NT + ND] == torsions.format_delta(wild, wild)
        # the crystal's string of the designed residues, from the twin
        h = torsions.torsions_host(sc.gt_atom14, sc.gt_exists, sc.gt_seq, sc.gt_atom14, sc.gt_exists, sc.gt_seq, sc.Lab, sc.chain_id, sc.residx,
                                   region=sc.region, res_mask=sc.res_mask)
        assert lines[1][-1] == torsions.abego_string(h['classes'], region) == torsions.abego_string(wcl.cpu()[0], region) and len(lines[1][-1]) == int(region[:sc.Lab].sum()) > 0
        assert lines[1][1 + 14] == lines[1][1 + 15] and int(lines[1][1 + 14]) > 0                  # abego_same == n_abego
        rows = torch.cat([tr[-1]['torsions'] for _, tr in runs]).cpu().tolist()
        classes = torch.cat([tr[-1]['torsions_classes'] for _, tr in runs]).cpu().numpy()
        for i, r in enumerate(lines[2:]):
            assert r[0] == str(i) and r[1:1 + NT] == torsions.format_torsions(rows[i]), (code, i, r)
            assert r[1 + NT:1 + NT + ND] == torsions.format_delta(rows[i], wild), (code, i, r)
            assert r[-1] == torsions.abego_string(classes[i], region), (code, i, r)
        if not collective:
            relaxed = runs[0][1][-1]['torsions_relaxed'].cpu().tolist()
            assert lines[1][1 + NT + ND:-1] == ['nan'] * NT
            for i, r in enumerate(lines[2:]):
                assert r[1 + NT + ND:-1] == torsions.format_torsions(relaxed[i]), (code, i)
            per_res = np.load(os.path.join(out, code + '_torsions_rows.npy'))
            want = runs[0][1][-1]['torsions_rows'].cpu().numpy()
            assert per_res.dtype == np.float64 and per_res.shape == (N, sc.Lab, 8) and np.array_equal(per_res, want, equal_nan=True)
