"""GPU checks of the secondary-structure analysis (abx_secondary_scores, csrc/secondary.hip; abx_amd.secondary.SecondaryScorer): the row,
the states and the per-residue table against the float64 host twin - equal, not close: every value is an integer count or an exactly
rounded fixed-point sum - on built chains and sheets, the tiny workload and the shipped complexes; the Lab edges of the bit words and
of the lane stride, the limits, the contracts of the entry (batch independence, an uninitialised workspace, a strided out, optional
outputs, a reused workspace), and the path through the sampler and the design driver."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from analysis_gpu_cases import (DEV, sample_tiny, sampler_pair, spy_on_sampler, table_lines, tiny_batch, ops, gpu_model)  # noqa: F401
import relax_cases as RC
import secondary_cases as SS
import shape_cases as SC

pytestmark = pytest.mark.gpu

GUARD = 64
NS = 22


def bits(t):
    return t.contiguous().view(torch.int64)


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
    x = torch.stack([torch.as_tensor(t[0])[:Lab] for t in triples]).float().to(DEV)
    sq = torch.stack([t[1][:Lab] for t in triples]).to(DEV)
    mask = torch.stack([torch.as_tensor(t[2]) for t in triples]).to(DEV)
    return x, sq, mask


def scored(sc, x, sq, mask=None, ws_fill=0xA5):
    """(row, rows, classes) on the host, every output and the workspace between guard values; the workspace starts as ws_fill bytes."""
    from abx_amd import ops as _ops
    B = x.shape[0]
    out, out_w = guarded((B, NS), torch.float64, -7.0)
    rows, rows_w = guarded((B, sc.Lab, 6), torch.int32, -7)
    cl, cl_w = guarded((B, sc.Lab), torch.int32, -7)
    ws, ws_w = guarded((_ops.secondary_workspace_bytes(B, sc.Lab),), torch.uint8, ws_fill)
    got = sc.score(x, sq, rows=rows, classes=cl, out=out, mask=mask, workspace=ws)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert guards_intact(out_w, -7.0) and guards_intact(rows_w, -7) and guards_intact(cl_w, -7) and guards_intact(ws_w, ws_fill)
    return out.cpu().clone(), rows.cpu().clone(), cl.cpu().clone()


def assert_equal_twin(row, rows, classes, h, what):
    """Every column, state and per-residue value equal (==): counts, and the fixed-point energy sum divided by 2^20."""
    row, rows, classes = row.numpy(), rows.numpy(), classes.numpy()
    print(what, 'device', row.tolist(), 'twin', h['row'].tolist())
    assert row.tolist() == h['row'].tolist(), (what, row.tolist(), h['row'].tolist())
    assert np.array_equal(classes, h['classes']), (what, np.argwhere(classes != h['classes'])[:8].tolist())
    assert np.array_equal(rows, h['rows']), (what, np.argwhere(rows != h['rows'])[:8].tolist())


def scorer_of(c, res_mask=None):
    from abx_amd import secondary
    return secondary.SecondaryScorer(SC.batch_of(c, DEV, res_mask=res_mask), region=c['mov'])


def test_built_chains_and_sheets_equal_the_twin(ops):
    """The five built chains in one batch (B = 5, Lab = 12) against the helix as wild type, and the two sheets (B = 2, Lab = 14)."""
    from abx_amd import secondary
    chains = SS.built_chains()
    c = SS.as_complex(chains[0]['x'], chains[0]['mask'])
    x, sq, mask = device_batch(c, [(o['x'], c['aa'], o['mask']) for o in chains])
    row, rows, cl = scored(scorer_of(c), x, sq, mask)
    for j, o in enumerate(chains):
        h = SS.twin(c, torch.from_numpy(o['x']))
        assert h['n_borderline'] == 0
        assert_equal_twin(row[j], rows[j], cl[j], h, ('chain', j))
        assert ''.join(secondary.LETTERS[v] for v in cl[j].tolist()) == o['letters'] and row[j, 0] == len(o['bonds'])
    sheets = [SS.sheet(False), SS.sheet(True)]
    c = SS.as_complex(sheets[0]['x'], sheets[0]['mask'], sheets[0]['chain'])
    x, sq, mask = device_batch(c, [(s['x'], c['aa'], s['mask']) for s in sheets])
    row, rows, cl = scored(scorer_of(c), x, sq, mask)
    for j, s in enumerate(sheets):
        h = SS.twin(c, torch.from_numpy(s['x']))
        assert_equal_twin(row[j], rows[j], cl[j], h, ('sheet', j))
        assert ''.join(secondary.LETTERS[v] for v in cl[j].tolist()) == s['letters'] and row[j, 6] == 5
    assert row[0, 8] == 5 and row[1, 8] == 0            # the parallel sheet keeps no bridge of the antiparallel wild type: another type


@pytest.fixture(scope='module')
def shipped(ops):
    """Per crystal: the complex, its seven structures, the device rows and the twin's - computed once, left unchanged."""
    out = {}
    for code, sel in RC.MOVABLE_SETS[:2]:
        c = RC.load_complex(code, sel)
        triples = SS.gpu_structures(c)
        sc = scorer_of(c)
        x, sq, mask = device_batch(c, triples)
        row, rows, cl = scored(sc, x, sq, mask)
        host = [SS.twin(c, t[0], mask=t[2], seq=t[1]) for t in triples]
        out[code] = dict(c=c, sc=sc, x=x, sq=sq, mask=mask, row=row, rows=rows, cl=cl, host=host)
    return out


@pytest.mark.parametrize('code', ['6qd7', '6ct7'])
def test_shipped_complexes_equal_the_twin(shipped, code):
    """The wild type, three seeded perturbations and their mutated versions (Ala / Gly / Pro: Pro removes donors) in one batch (B = 7;
    Lab = 227 and 221, ragged against the block of 256 and the words of 32; the H -> L boundary)."""
    from abx_amd import secondary
    s = shipped[code]
    c = s['c']
    assert s['row'].shape == (7, NS) and c['Lab'] in (221, 227)
    for k, h in enumerate(s['host']):
        assert h['n_borderline'] == 0
        assert_equal_twin(s['row'][k], s['rows'][k], s['cl'][k], h, (code, k))
    w = s['row'][0]
    assert w[3] == w[4] == w[1] and w[7] == w[8] == w[6] and w[17] == w[18] == w[19] == int(c['mov'].sum())
    assert w[0] == {'6qd7': 150, '6ct7': 144}[code] and secondary.ss_string(s['cl'][0], c['mov']) == {'6qd7': 'EEBSSSSS---B-E', '6ct7': 'ESSS'}[code]
    assert torch.equal(bits(s['sc'].wild().cpu()[0]), bits(w))
    assert len({tuple(r) for r in s['row'].tolist()}) >= 4
    print(code, [secondary.ss_string(s['cl'][k], c['mov']) for k in range(7)])


def test_tiny_workload_equals_the_twin(ops):
    from abx_amd import secondary
    cx, xh, region = SS.tiny_structures()
    Lab = cx['anchor_flag'].shape[0]
    assert Lab == 16
    sc = secondary.SecondaryScorer({k: v.to(DEV) for k, v in cx.items()}, region=region)
    row, rows, cl = scored(sc, xh.to(DEV), cx['seq'][None, :Lab].repeat(2, 1).to(DEV))
    for k in range(2):
        assert_equal_twin(row[k], rows[k], cl[k], SS.synthetic_twin(cx, xh[k], region), ('tiny', k))


@pytest.mark.parametrize('n', [1, 2, 4, 5, 31, 32, 33, 64, 65, 255, 256, 257])
def test_lab_edges(ops, n):
    """1, 2, 4, 5: no helix and no bridge is possible; 31 .. 65: the edges of the bit words; 255 .. 257: the lane stride.  Concatenated
    built chains and sheets with chain ids of their own; the second structure has the O of its middle row missing."""
    c = SS.concatenated(n)
    m2 = c['mask'].clone()
    m2[n // 2, 3] = False
    x, sq, mask = device_batch(c, [(c['x'], c['aa'], c['mask']), (c['x'], c['aa'], m2)])
    row, rows, cl = scored(scorer_of(c), x, sq, mask)
    for k, m in enumerate((c['mask'], m2)):
        h = SS.twin(c, mask=m)
        assert h['n_borderline'] == 0
        assert_equal_twin(row[k], rows[k], cl[k], h, (n, k))
    if n <= 5:                                          # at most one turn: no helix start, no bridge
        assert row[0, 6] == 0 and row[0, 20] == 0 and row[0, 21] == 0 and not {1, 2, 3, 4, 5} & set(cl[0].tolist())
    if n >= 31:
        assert row[0, 0] > 0 and row[0, 21] > 0
    if n >= 255:
        assert row[0, 6] > 0 and row[0, 20] > 0
    assert cl[1, n // 2] == 0 and row[1, 17] == n - 1


def test_limits(ops):
    """One launch at MAX_LAB equals the twin; MAX_LAB + 1, hb_energy >= 0, a non-unit bend and a null workspace are refused by name
    before any launch: out keeps its fill."""
    from abx_amd import _lib, secondary
    c = SS.concatenated(secondary.MAX_LAB)
    x, sq, mask = device_batch(c, [(c['x'], c['aa'], c['mask'])])
    row, rows, cl = scored(scorer_of(c), x, sq, mask)
    assert_equal_twin(row[0], rows[0], cl[0], SS.twin(c), 'MAX_LAB')
    assert row[0, 0] > 200 and row[0, 6] > 50
    big = SS.concatenated(secondary.MAX_LAB + 1)
    with pytest.raises(ValueError, match='at most 800'):
        scorer_of(big)
    sc = scorer_of(SS.concatenated(40))
    c40 = SS.concatenated(40)
    x, sq, mask = device_batch(c40, [(c40['x'], c40['aa'], c40['mask'])])
    out = torch.full((1, NS), -7.0, dtype=torch.float64, device=DEV)
    args = (x, sq, sc.gt_atom14, sc.gt_seq, sc.gt_exists, sc.chain_id, sc.residx)
    th = secondary.thresholds()
    for bad, text in ((dict(th, hb_energy=0.0), 'hb_energy'), (dict(th, hb_energy=0.5), 'hb_energy'), (dict(th, bend=(0.5, 0.5)), r'\(cos, sin\)')):
        with pytest.raises(Exception, match=text):
            ops.secondary_scores(*args, bad, Lab=40, region=sc.region, mask=mask, out=out)
    xb, sqb, mb = device_batch(big, [(big['x'], big['aa'], big['mask'])])
    d = lambda t, dt: t.to(dt).to(DEV)
    with pytest.raises(Exception, match='Lab <= 800'):
        ops.secondary_scores(xb, sqb, d(big['x'], torch.float32), d(big['aa'], torch.int64), d(big['mask'], torch.uint8), d(big['chain'], torch.int32),
                             d(big['residx'], torch.int32), th, Lab=801, mask=mb, out=out)
    # a null workspace: the descriptor is checked before anything is dereferenced
    a = _lib.AbxSecondaryArgs()
    for f in ('pred_atom14', 'pred_seq', 'gt_atom14', 'gt_exists', 'gt_seq', 'radius', 'chain_id'):
        setattr(a, f, x.data_ptr())
    a.out, a.out_stride = out.data_ptr(), NS
    a.B, a.L, a.Lab, a.Lpred, a.pred_sb, a.pred_seq_sb = 1, 40, 40, 40, 40 * 42, 40
    a.hb_energy, a.pro = th['hb_energy'], 14
    a.bend[0], a.bend[1] = th['bend']
    lib = _lib.load()
    assert lib.abx_secondary_scores(ctypes.byref(a), None, None) < 0 and b'abx_secondary_scores: null workspace' in lib.abx_last_error_string()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def test_contracts(shipped, ops):
    """Equal bits: a structure alone and inside its batch of 7; a workspace of 0xFF bytes; out as columns of a wider table between
    guard columns; rows / classes absent; a second call on the same workspace with a smaller Lab."""
    s = shipped['6ct7']
    c, sc, x, sq, mask = s['c'], s['sc'], s['x'], s['sq'], s['mask']
    B, Lab = x.shape[0], c['Lab']
    for k in (0, 3, 6):
        row, rows, cl = scored(sc, x[k:k + 1], sq[k:k + 1], mask[k:k + 1])
        assert torch.equal(bits(row[0]), bits(s['row'][k])) and torch.equal(rows[0], s['rows'][k]) and torch.equal(cl[0], s['cl'][k]), k
    row, rows, cl = scored(sc, x, sq, mask, ws_fill=0xFF)
    assert torch.equal(bits(row), bits(s['row'])) and torch.equal(rows, s['rows']) and torch.equal(cl, s['cl'])
    table = torch.full((B, NS + 5), -1.0, dtype=torch.float64, device=DEV)
    sc.score(x[:3], sq[:3], out=table[:3, 2:2 + NS], mask=mask[:3])     # no optional output
    sc.score(x[3:], sq[3:], out=table[3:, 2:2 + NS], mask=mask[3:], classes=sc.new_classes(B - 3))
    t = table.cpu()
    assert torch.equal(bits(t[:, 2:2 + NS]), bits(s['row'])) and bool((t[:, :2] == -1).all()) and bool((t[:, 2 + NS:] == -1).all())
    # the same workspace, first for this complex, then for a smaller one
    ws = torch.full((ops.secondary_workspace_bytes(B, Lab),), 0x5A, dtype=torch.uint8, device=DEV)
    assert torch.equal(bits(sc.score(x, sq, mask=mask, workspace=ws).cpu()), bits(s['row']))
    small = SS.concatenated(65)
    xs, sqs, ms = device_batch(small, [(small['x'], small['aa'], small['mask'])])
    rows1, cl1 = torch.empty(1, 65, 6, dtype=torch.int32, device=DEV), torch.empty(1, 65, dtype=torch.int32, device=DEV)
    got = scorer_of(small).score(xs, sqs, mask=ms, workspace=ws, rows=rows1, classes=cl1)
    assert_equal_twin(got.cpu()[0], rows1.cpu()[0], cl1.cpu()[0], SS.twin(small), 'reused workspace')
    # res_mask takes a row out of both structures
    r = int(torch.nonzero(c['mov'])[1, 0])
    keep = torch.ones(c['aa'].shape[0], dtype=torch.uint8)
    keep[r] = 0
    row, rows, cl = scored(scorer_of(c, res_mask=keep), x[:2], sq[:2], mask[:2])
    for k in range(2):
        t3 = SS.gpu_structures(c)[k]
        assert_equal_twin(row[k], rows[k], cl[k], SS.twin(c, t3[0], mask=t3[2], seq=t3[1], res_mask=keep), ('res_mask', k))
    assert cl[0, r] == 0 and row[0, 17] == int(c['mov'].sum()) - 1


def test_sampler_scores_the_last_record(gpu_model, cfg):
    """sample_fn(secondary=, relaxer=) on the tiny workload: the four keys sit on the last record only and equal a direct .score(); the
    plain records have today's keys and the shared tensors today's bits (sampler_pair)."""
    from abx_amd import relax, secondary
    b, sid = tiny_batch(gpu_model)
    B, Lab = sid.shape[0], b['anchor_flag'].shape[1]
    sc = secondary.SecondaryScorer(b)
    sc.want_rows = True
    _, got = sampler_pair(gpu_model, cfg, b, sid, ('secondary', 'secondary_classes', 'secondary_rows', 'secondary_relaxed'), secondary=sc,
                          relaxer=relax.ViolationRelaxer(b))
    last = got[-1]
    assert last['secondary'].shape == (B, NS) and last['secondary'].dtype == torch.float64
    assert last['secondary_classes'].shape == (B, Lab) and last['secondary_classes'].dtype == torch.int32
    assert last['secondary_rows'].shape == (B, Lab, 6) and last['secondary_rows'].dtype == torch.int32
    rows, cl = sc.new_rows(B), sc.new_classes(B)
    assert torch.equal(bits(sc.score(last['atom14_results'], last['seq'], rows=rows, classes=cl)), bits(last['secondary']))
    assert torch.equal(rows, last['secondary_rows']) and torch.equal(cl, last['secondary_classes'])
    assert torch.equal(bits(sc.score(last['atom14_relaxed'], last['seq'])), bits(last['secondary_relaxed']))
    print('tiny workload, secondary rows', last['secondary'].cpu().tolist(), 'wild', sc.wild().cpu().tolist())
    assert sc.wild().shape == (1, NS)


@pytest.mark.parametrize('relax', [False, True])
def test_design_driver_writes_the_secondary_table(tmp_path, monkeypatch, relax):
    """`abx_amd.design --workload tiny --secondary` with --secondary_rows, or with --relax: <complex>_secondary.tsv with the header, the
    wild line and one line per sample whose fields are the sampler's record at print precision, the state string last."""
    from abx_amd import design, secondary
    N = 3
    seen = spy_on_sampler(monkeypatch, lambda batch, k, traj: (k['secondary'], traj) if k.get('secondary') is not None else None)
    out = tmp_path / 'out'
    files = design.main(['--workload', 'tiny', '--num_samples', str(N), '--num_t', '3', '--secondary', '--output_dir', str(out)] +
                        (['--relax', '--relax_iters', '10'] if relax else ['--secondary_rows']))
    tsv = [f for f in files if f.endswith('_secondary.tsv')]
    assert len(tsv) == 1 and len(seen) == 1 and len(glob.glob(str(out / '*_secondary_rows.npy'))) == (0 if relax else 1)
    sc, traj = seen[0]
    lines = [ln.split('\t') for ln in open(tsv[0]).read().splitlines()]
    ND = len(secondary.DELTA_COLUMNS)
    head = ['sample'] + list(secondary.SECONDARY_COLUMNS) + ['delta_' + c for c in secondary.DELTA_COLUMNS]
    assert lines[0] == head + ([c + '_relaxed' for c in secondary.SECONDARY_COLUMNS] if relax else []) + ['dssp']
    assert len(lines) == 2 + N and all(len(r) == len(lines[0]) for r in lines)
    wcl = sc.new_classes(1)
    wild = sc.wild(classes=wcl).cpu()[0].tolist()
    region = sc.region.cpu().numpy()
    assert lines[1][:1 + NS] == ['wild'] + secondary.format_secondary(wild) and lines[1][1 + NS:1 + NS + ND] == secondary.format_delta(wild, wild)
    h = secondary.secondary_host(sc.gt_atom14, sc.gt_exists, sc.gt_seq, sc.gt_atom14, sc.gt_exists, sc.gt_seq, sc.Lab, sc.chain_id, sc.residx,
                                 region=sc.region, res_mask=sc.res_mask)
    assert lines[1][-1] == secondary.ss_string(h['classes'], region) == secondary.ss_string(wcl.cpu()[0], region) and len(lines[1][-1]) == int(region[:sc.Lab].sum()) > 0
    rows = traj[-1]['secondary'].cpu().tolist()
    classes = traj[-1]['secondary_classes'].cpu().numpy()
    for i, r in enumerate(lines[2:]):
        assert r[0] == str(i) and r[1:1 + NS] == secondary.format_secondary(rows[i]) and r[1 + NS:1 + NS + ND] == secondary.format_delta(rows[i], wild), (i, r)
        assert r[-1] == secondary.ss_string(classes[i], region), (i, r)
    if relax:
        relaxed = traj[-1]['secondary_relaxed'].cpu().tolist()
        assert lines[1][1 + NS + ND:-1] == ['nan'] * NS
        for i, r in enumerate(lines[2:]):
            assert r[1 + NS + ND:-1] == secondary.format_secondary(relaxed[i]), i
    else:
        per_res = np.load(glob.glob(str(out / '*_secondary_rows.npy'))[0])
        assert per_res.dtype == np.int32 and per_res.shape == (N, sc.Lab, 6) and np.array_equal(per_res, traj[-1]['secondary_rows'].cpu().numpy())
