"""GPU checks of the patch analysis (abx_patch_scores, csrc/patches.hip; abx_amd.patches.PatchScorer): every column of the row and the
per-residue table against the float64 / int64 host twin - equal, not close -, the edges of the pair kernel's tiles, residue types taken
from the tokens, the edge rows (no side chains, no antigen nearby, coincident atoms), batch independence, a reused workspace with guard
words behind it, the entry's refusals, and the path through the sampler and the design driver, where the surface kernel is shared with
the interface, polar, developability and shape analyses."""
import os

import numpy as np
import pytest
import torch

from analysis_gpu_cases import (ALONE, CODES, DEV, driver_pair, l352_designs, names, pdb_args, runs_of, sample_tiny, sampler_pair,
                                set_master_port, spy_on_sampler, table_lines, tiny_batch, typed_or_gt, ops, gpu_model)  # noqa: F401  (ops, gpu_model: set up once per importing module)
import patches_cases as PC
import relax_cases as RC
import shape_cases as SC

pytestmark = pytest.mark.gpu

GUARD = 256
NP = 18


def bits(t):
    return t.contiguous().view(torch.int64)


def batch_of(c, **kw):
    return SC.batch_of(c, DEV, **kw)


def device_args(c, xs):
    """Antibody coordinates, tokens and the ground truth's atom mask of structures xs (B,L,14,3) of complex c on the device."""
    B, Lab = xs.shape[0], c['Lab']
    return xs[:, :Lab].float().to(DEV), c['aa'][None, :Lab].repeat(B, 1).to(DEV), c['mask'][None].repeat(B, 1, 1).to(DEV)


def assert_equal_twin(row, rows, hrow, hrows, what):
    assert row.tolist() == hrow.tolist(), (what, row.tolist(), hrow.tolist())
    assert np.array_equal(rows.numpy(), hrows), (what, np.argwhere(rows.numpy() != hrows)[:8].tolist())


def scored(sc, x, sq, mask=None, points=None):
    """(row, rows, points) of structures x on the host; the point counts come from the scorer's own surface unless given."""
    B = x.shape[0]
    if points is None:
        points = sc.new_points(B)
        sc.interface.score(x, sq, points=points, mask=mask)
    rows = torch.full((B, sc.L, 4), -7.0, dtype=torch.float64, device=DEV)
    row = sc.score(x, sq, points=points, rows=rows, mask=mask)
    return row.cpu(), rows.cpu(), points.cpu()


@pytest.fixture(scope='module')
def crystal(ops):
    """Per shipped complex: the complex, its four structures (crystal + three seeded perturbations), the device rows of a scorer with its
    own surface and the twin's rows - computed once, shared by the tests below and left unchanged."""
    from abx_amd import patches
    out = {}
    for code in ('6ct7', '6qd7'):
        c = RC.load_complex(code, 'h3')
        xs = PC.structures(c)
        x, sq, gt = device_args(c, xs)
        sc = patches.PatchScorer(batch_of(c), region=c['mov'])
        row, rows, pts = scored(sc, x, sq, mask=gt)
        host = [PC.twin(c, xs[k], c['mask'], pts[k], details=True) for k in range(xs.shape[0])]
        out[code] = dict(c=c, xs=xs, x=x, sq=sq, gt=gt, sc=sc, row=row, rows=rows, pts=pts, host=host)
    return out


@pytest.mark.parametrize('code', ['6ct7', '6qd7'])
def test_rows_equal_the_host_twin(ops, crystal, code):
    """The crystal structure and three seeded perturbations in one batch (B = 4; L = 231, and L = 259, which crosses a 256-wide j-tile):
    all 18 columns and the (L, 4) table equal the host twin's bit for bit; the perturbations put atoms within 1 Angstrom of each other,
    so the floor of r2 is exercised.  `points` handed over from an InterfaceScorer call equals points=None; the crystal structure with
    the host's own point counts and the prototype's numbers; rows of a wider table."""
    from abx_amd import interface, patches
    s = crystal[code]
    c, sc, x, sq, gt = s['c'], s['sc'], s['x'], s['sq'], s['gt']
    B, L = x.shape[0], c['aa'].shape[0]
    assert s['row'].shape == (B, NP) and s['row'].dtype == torch.float64
    for k in range(B):
        assert_equal_twin(s['row'][k], s['rows'][k], s['host'][k][0], s['host'][k][1], (code, k))
    print(code, 'psh', s['row'][:, 0].tolist(), 'ppc', s['row'][:, 1].tolist(), 'pnc', s['row'][:, 2].tolist(), 'pairs', s['row'][:, 14].tolist())
    assert min(float(h[2]['D2'].min()) for h in s['host']) < 1.0
    want = PC.PROTOTYPE[code]
    assert tuple(int(v) for v in s['row'][0, 11:]) == want['counts'] and f'{s["row"][0, 0]:.3f}' == want['psh']
    hrow, hrows = PC.twin(c, s['xs'][0], c['mask'], None)                      # points by interface_host
    assert_equal_twin(s['row'][0], s['rows'][0], hrow, hrows, (code, 'host points'))
    # points=None runs the surface kernel inside; a shared InterfaceScorer hands its counts over
    it = interface.InterfaceScorer(batch_of(c), region=c['mov'])
    shared = patches.PatchScorer(batch_of(c), interface=it)
    assert shared.interface is it and sc.interface is not it and torch.equal(shared.region, sc.region)
    pts = shared.new_points(B)
    it.score(x, sq, points=pts, mask=gt)
    assert torch.equal(pts.cpu(), s['pts'])
    none = sc.score(x, sq, mask=gt).cpu()
    given = shared.score(x, sq, points=pts, mask=gt).cpu()
    assert torch.equal(bits(none), bits(s['row'])) and torch.equal(bits(given), bits(s['row']))
    w = sc.wild().cpu()[0]
    assert w.tolist() == s['row'][0].tolist() == shared.wild(points=pts[:1].contiguous()).cpu()[0].tolist()
    # rows of a wider table
    table = torch.full((B, NP + 5), -1.0, dtype=torch.float64, device=DEV)
    shared.score(x, sq, points=pts, out=table[:, 2:2 + NP], mask=gt)
    t = table.cpu()
    assert torch.equal(bits(t[:, 2:2 + NP]), bits(s['row'])) and bool((t[:, :2] == -1).all()) and bool((t[:, 2 + NP:] == -1).all())


def test_a_structure_alone_equals_itself_in_a_batch(ops, crystal):
    s = crystal['6qd7']
    sc = s['sc']
    for b in (0, 3):
        rows = sc.new_rows(1)
        alone = sc.score(s['x'][b:b + 1], s['sq'][b:b + 1], points=s['pts'][b:b + 1].to(DEV).contiguous(), rows=rows, mask=s['gt'][:1])
        assert torch.equal(bits(alone.cpu()[0]), bits(s['row'][b])) and torch.equal(bits(rows.cpu()[0]), bits(s['rows'][b])), b


@pytest.mark.parametrize('L', ['Lab+1', 256, 257])
def test_tile_edges(ops, L):
    """6qd7 cut to L = Lab + 1 (one antigen row), 256 (the j-tile exactly full) and 257 (one row in a second tile); and the whole complex
    with a res_mask that drops rows of both sides - a dropped row has no atoms, is in no pair and has flags 0."""
    from abx_amd import patches
    full = RC.load_complex('6qd7', 'h3')
    L = full['Lab'] + 1 if L == 'Lab+1' else L
    c = PC.cut_complex(full, L)
    assert c['aa'].shape[0] == L and c['x'].shape[0] == L and c['Lab'] == full['Lab']
    xs = torch.stack([c['x'].float().double(), RC.perturb(c, 6)])
    x, sq, gt = device_args(c, xs)
    sc = patches.PatchScorer(batch_of(c), region=c['mov'])
    row, rows, pts = scored(sc, x, sq, mask=gt)
    for k in range(2):
        hrow, hrows = PC.twin(c, xs[k], c['mask'], pts[k])
        assert_equal_twin(row[k], rows[k], hrow, hrows, (L, k))
    if L == 257:
        keep = torch.ones(L, dtype=torch.bool)
        drop = [3, 50, 100, c['Lab'] - 1, c['Lab'], 256]
        keep[drop] = False
        cut = patches.PatchScorer(batch_of(c, res_mask=keep), region=c['mov'])
        row, rows, pts = scored(cut, x, sq, mask=gt)
        for k in range(2):
            hrow, hrows = PC.twin(c, xs[k], c['mask'] & keep[:, None], pts[k])
            assert_equal_twin(row[k], rows[k], hrow, hrows, ('res_mask', k))
        assert not rows[:, drop].any()


@pytest.mark.parametrize('token', [PC.K, PC.D, PC.G, PC.X])
def test_types_from_tokens(ops, token):
    """The designed rows of 6ct7 retyped to all Lys, all Asp, all Gly and X with pred_mask NULL: a predicted row has the atoms of ITS
    token (the radius table), X has none.  Against the twin."""
    from abx_amd import patches, residue_constants as rc
    c = RC.load_complex('6ct7', 'h3')
    Lab = c['Lab']
    seq = c['aa'].clone()
    seq[c['mov']] = token
    xs = torch.stack([c['x'].float().double(), RC.perturb(c, 7)])
    x, sq = xs[:, :Lab].float().to(DEV), seq[None, :Lab].repeat(2, 1).to(DEV)
    typed = torch.cat([torch.as_tensor(rc.restype_atom14_mask)[seq[:Lab]].bool(), c['mask'][Lab:]])
    sc = patches.PatchScorer(batch_of(c), region=c['mov'])
    row, rows, pts = scored(sc, x, sq)
    for k in range(2):
        hrow, hrows = PC.twin(c, xs[k], typed, pts[k], seq=seq)
        assert_equal_twin(row[k], rows[k], hrow, hrows, (token, k))
    mov = c['mov']
    if token == PC.X:
        assert not rows[:, mov].any()
    if token == PC.G:
        assert bool((rows[:, mov, 3] == 33).all())           # present and region, never exposed
    print('token', token, 'row', row[0].tolist())


def test_edge_rows(ops, crystal):
    """An all-Gly antibody: nothing is exposed, every patch and cross column is 0.  The antigen 100 Angstrom away with the point counts
    held fixed: the cross columns are 0 and the columns of the free antibody keep their bits.  Two residues on top of each other: D2 = 0,
    the terms stay bounded, the row equals the twin."""
    from abx_amd import patches
    s = crystal['6ct7']
    c, xs = s['c'], s['xs']
    Lab = c['Lab']
    # all Gly
    sc = s['sc']
    x2, gly = s['x'][:2], torch.full_like(s['sq'][:2], PC.G)
    row, rows, pts = scored(sc, x2, gly)
    seq = c['aa'].clone()
    seq[:Lab] = PC.G
    gmask = torch.cat([torch.tensor([True] * 4 + [False] * 10)[None].repeat(Lab, 1), c['mask'][Lab:]])
    for k in range(2):
        hrow, hrows = PC.twin(c, xs[k], gmask, pts[k], seq=seq)
        assert_equal_twin(row[k], rows[k], hrow, hrows, ('all Gly', k))
    assert row[:, :11].eq(0).all() and row[:, 12:].eq(0).all() and bool((row[:, 11] == s['row'][0, 11]).all())
    # the antigen moved away
    moved = SC.antigen_moved(c)
    away = patches.PatchScorer(batch_of(c, x=moved), region=c['mov'])
    pts4 = s['pts'].to(DEV)
    rows_d = away.new_rows(4)
    got = away.score(s['x'], s['sq'], points=pts4, rows=rows_d, mask=s['gt']).cpu()
    free, cross = list(PC.FREE_COLUMNS), list(PC.CROSS_COLUMNS)
    assert got[:, cross].eq(0).all() and torch.equal(bits(got[:, free]), bits(s['row'][:, free])) and bool((s['row'][:, 16] > 0).all())
    rows_d = rows_d.cpu()
    assert not rows_d[:, :, 2].any() and torch.equal(bits(rows_d[:, :, [0, 1, 3]]), bits(s['rows'][:, :, [0, 1, 3]]))
    hrow, hrows = PC.twin(c, torch.cat([xs[1, :Lab], moved[Lab:]]), c['mask'], s['pts'][1])
    assert_equal_twin(got[1], rows_d[1], hrow, hrows, 'antigen moved')
    # coincident residues: two rows of the vicinity, and an antibody row on an antigen row
    vic = np.nonzero(s['host'][0][2]['vicinity'])[0]
    xc = xs[0].clone()
    xc[vic[1]] = xc[vic[0]]
    charged = [r for r in range(Lab) if int(c['aa'][r]) in (PC.K, PC.R, PC.D, PC.E)]
    target = [r for r in range(Lab, c['aa'].shape[0]) if int(c['aa'][r]) in (PC.K, PC.R, PC.D, PC.E)]
    xc[charged[0]] = c['x'][target[0]].float().double()
    row, rows, pts = scored(sc, xc[None, :Lab].float().to(DEV), s['sq'][:1], mask=s['gt'][:1])
    hrow, hrows, d = PC.twin(c, xc, c['mask'], pts[0], details=True)
    assert d['D2'][vic[0], vic[1]] == 0.0 and d['D2'][charged[0], target[0]] == 0.0 and np.isfinite(hrow).all()
    assert_equal_twin(row[0], rows[0], hrow, hrows, 'coincident')


def test_headline_size_and_batch_independence():
    """L = 352 synthetic workload, B = 100 perturbed copies (two j-tiles, eight i-tiles, 100 structures): the rows of structures 0, 57
    and 99 scored alone equal their rows in the batch bit for bit; a second call repeats the first; structure 57 equals the host twin."""
    from abx_amd import patches
    cx, xh, x, sq, _ = l352_designs()
    (B, Lab), L = sq.shape, cx['seq'].shape[0]
    sc = patches.PatchScorer({k: v.to(DEV) for k, v in cx.items()}, region=cx['cdr_def'] == 5)
    pts = sc.new_points(B)
    sc.interface.score(x, sq, points=pts)
    rows = torch.full((B, L, 4), -7.0, dtype=torch.float64, device=DEV)
    full = sc.score(x, sq, points=pts, rows=rows)
    again = sc.score(x, sq, points=pts)
    assert full.shape == (B, NP) and torch.equal(bits(full), bits(again))
    h = full.cpu()
    print('L352 B=100: psh', h[:, 0].min().item(), h[:, 0].max().item(), 'pairs', h[:, 14].min().item(), h[:, 14].max().item(), 'cross', h[:, 16].max().item())
    assert len({tuple(r) for r in h.tolist()}) > 50
    for b in ALONE:
        r1 = torch.full((1, L, 4), -7.0, dtype=torch.float64, device=DEV)
        alone = sc.score(x[b:b + 1], sq[b:b + 1], points=pts[b:b + 1].contiguous(), rows=r1)
        assert torch.equal(bits(alone[0]), bits(full[b])) and torch.equal(bits(r1[0]), bits(rows[b])), b
    xs = torch.cat([xh[57], cx['atom14_gt_positions'][Lab:].float()])
    hrow, hrows = patches.patches_host(xs, typed_or_gt(cx, Lab, typed=True), cx['seq'], Lab, cx['chain_id'], cx['residx'], cx['cdr_def'],
                                       region=cx['cdr_def'] == 5, points=pts[57].cpu())
    assert_equal_twin(h[57], rows[57].cpu(), hrow, hrows, 'L352 structure 57')


def test_workspace_is_reused_and_not_overrun(ops, crystal):
    """One workspace sized for B = 4, with guard bytes behind it, serves B = 4 and then B = 2: the rows are those of a fresh workspace and
    the guard is intact; so it is behind a workspace of exactly B = 1."""
    from abx_amd import ops as _ops
    s = crystal['6qd7']
    sc, L, Lab = s['sc'], s['sc'].L, s['sc'].Lab
    need = _ops.patch_workspace_bytes(4, L, Lab)
    assert need == 4 * _ops.patch_workspace_bytes(1, L, Lab) and need % 16 == 0
    ws = torch.zeros(need + GUARD, dtype=torch.uint8, device=DEV)
    ws[need:] = 0xA5
    pts = s['pts'].to(DEV)
    got4 = sc.score(s['x'], s['sq'], points=pts, mask=s['gt'], workspace=ws).cpu()
    got2 = sc.score(s['x'][2:], s['sq'][2:], points=pts[2:].contiguous(), mask=s['gt'][2:], workspace=ws).cpu()
    assert bool((ws[need:] == 0xA5).all()), 'the bytes behind the workspace were written'
    assert torch.equal(bits(got4), bits(s['row'])) and torch.equal(bits(got2), bits(s['row'][2:]))
    one = _ops.patch_workspace_bytes(1, L, Lab)
    ws = torch.zeros(one + GUARD, dtype=torch.uint8, device=DEV)
    ws[one:] = 0xA5
    got1 = sc.score(s['x'][3:], s['sq'][3:], points=pts[3:].contiguous(), mask=s['gt'][3:], workspace=ws).cpu()
    assert bool((ws[one:] == 0xA5).all()) and torch.equal(bits(got1), bits(s['row'][3:]))
    with pytest.raises(AssertionError, match='workspace'):
        sc.score(s['x'], s['sq'], points=pts, mask=s['gt'], workspace=ws)


def test_entry_refusals(ops, crystal):
    """Tables with which a sum could leave int64, and thresholds that are no distances, come back as an argument error with the entry's
    name; nothing is launched."""
    from abx_amd import ops as _ops
    from abx_amd._lib import AbxHipError
    s = crystal['6ct7']
    sc = s['sc']
    it = sc.interface
    pts = s['pts'].to(DEV)

    def call(**kw):
        k = dict(sc.kw, **kw)
        return _ops.patch_scores(s['x'], s['sq'], it.gt_atom14, it.gt_seq, it.gt_exists, sc.chain_id, sc.cdr_def, sc.tables, pts, Lab=sc.Lab,
                                 region=sc.region, mask=s['gt'], **k)

    assert torch.equal(bits(call().cpu()), bits(s['row']))
    for kw, text in ((dict(h_max=1e5), 'int64'), (dict(q_max=1 << 20), 'int64'), (dict(cutoff=0.0), 'cutoff2'), (dict(salt=float('nan')), 'salt2'),
                     (dict(exposed=1.5), 'exposed'), (dict(gly=21), 'gly')):
        with pytest.raises(AbxHipError) as e:
            call(**kw)
        assert 'abx_patch_scores' in str(e.value) and 'rc=-' in str(e.value) and text in str(e.value), (kw, str(e.value))


def test_sampler_scores_the_last_record(gpu_model, cfg):
    """sample_fn(patches=) on the tiny workload: with patches=None the records have today's keys and bits, with a scorer 'patches' sits
    on the last record only and equals a direct .score() of that record; with a relaxer also 'patches_relaxed', with want_rows
    'patches_rows'; sharing the interface scorer changes no table."""
    from abx_amd import interface, patches, relax
    b, sid = tiny_batch(gpu_model)
    B, L = sid.shape[0], b['seq'].shape[1]
    sc = patches.PatchScorer(b)
    _, got = sampler_pair(gpu_model, cfg, b, sid, ('patches',), patches=sc)
    last = got[-1]
    assert last['patches'].shape == (B, NP) and last['patches'].dtype == torch.float64
    assert not {'patches_relaxed', 'patches_rows', 'interface'} & set(last)
    assert torch.equal(bits(sc.score(last['atom14_results'], last['seq'])), bits(last['patches']))
    it = interface.InterfaceScorer(b)
    sh = patches.PatchScorer(b, interface=it)
    sh.want_rows = True
    full = sample_tiny(gpu_model, cfg, b, sid, mode='design', patches=sh, interface=it, relaxer=relax.ViolationRelaxer(b))
    assert len(full) == 1
    rec = full[0]
    assert torch.equal(bits(rec['patches']), bits(last['patches'])) and rec['patches_rows'].shape == (B, L, 4)
    rows = sh.new_rows(B)
    assert torch.equal(bits(sh.score(rec['atom14_results'], rec['seq'], rows=rows)), bits(rec['patches']))
    assert torch.equal(bits(rows), bits(rec['patches_rows']))
    assert torch.equal(bits(sh.score(rec['atom14_relaxed'], rec['seq'])), bits(rec['patches_relaxed']))
    assert torch.equal(bits(it.score(rec['atom14_results'], rec['seq'])), bits(rec['interface']))
    print('tiny workload, patch rows', rec['patches'].cpu().tolist(), 'wild', sc.wild().cpu().tolist())
    assert sc.wild().shape == (1, NP)


@pytest.mark.parametrize('collective', [False, True])
def test_design_driver_writes_the_patches_table(tmp_path, monkeypatch, collective):
    """`abx_amd.design --patches`: <complex>_patches.tsv with the header, the wild line and one line per sample whose fields are the
    sampler's records at print precision; every other file of the run is byte-identical to the run without the flag.
    collective = False: the shipped 6ct7 complex with --relax --patches_rows (the relaxed columns follow, the per-residue table is
    written).  collective = True: the 1-rank RCCL path on both shipped complexes, the table as further columns of the set-level gather."""
    from abx_amd import patches
    out, codes, N, seen = driver_pair(tmp_path, monkeypatch, 'patches', ['--patches'] + ([] if collective else ['--patches_rows']), collective,
                                      plain_extra=['--relax', '--relax_iters', '20'], extra_files=[] if collective else [CODES[0] + '_patches_rows.npy'])
    NDELTA = len(patches.DELTA_COLUMNS)
    for code in codes:
        lines = table_lines(out, code, 'patches')
        head = ['sample'] + list(patches.PATCHES_COLUMNS) + ['delta_' + c for c in patches.DELTA_COLUMNS]
        assert lines[0] == head + ([] if collective else [c + '_relaxed' for c in patches.PATCHES_COLUMNS])
        assert len(lines) == 1 + 1 + N and all(len(r) == len(lines[0]) for r in lines)
        runs = runs_of(seen, code, collective)
        wild = runs[0][0].wild().cpu()[0].tolist()
        assert lines[1][:1 + NP] == ['wild'] + patches.format_patches(wild)
        assert lines[1][1 + NP:1 + NP + NDELTA] == patches.format_delta(wild, wild)
        want = PC.PROTOTYPE[code[:4]]
        # (the driver's region is the rows the sampler diffuses, not the prototype's CDR-H3: the region columns are left out)
        assert tuple(int(v) for v in wild[11:17]) == want['counts'][:6] and lines[1][1] == want['psh'] and lines[1][2] == want['ppc']
        rows = torch.cat([tr[-1]['patches'] for _, tr in runs]).cpu().tolist()
        for i, r in enumerate(lines[2:]):
            assert r[0] == str(i) and r[1:1 + NP] == patches.format_patches(rows[i]), (code, i, r)
            assert r[1 + NP:1 + NP + NDELTA] == patches.format_delta(rows[i], wild), (code, i, r)
        if not collective:
            relaxed = runs[0][1][-1]['patches_relaxed'].cpu().tolist()
            assert lines[1][1 + NP + NDELTA:] == ['nan'] * NP
            for i, r in enumerate(lines[2:]):
                assert r[1 + NP + NDELTA:] == patches.format_patches(relaxed[i]) and 'nan' not in r, (code, i)
            per_res = np.load(os.path.join(out, code + '_patches_rows.npy'))
            want = runs[0][1][-1]['patches_rows'].cpu().numpy()
            assert per_res.dtype == np.float64 and per_res.shape == (N, 231, 4) and np.array_equal(per_res, want)
            assert [int(((per_res[i, :, 3].astype(np.int64) & 8) != 0).sum()) for i in range(N)] == [int(r[13]) for r in rows]


def test_set_level_and_sharded_runs_write_the_same_table(tmp_path, monkeypatch):
    """The set-level schedule (1-rank RCCL path, rows gathered) and the sample-sharded one write the same <complex>_patches.tsv."""
    from abx_amd import design
    set_master_port(monkeypatch)
    common = pdb_args(CODES[:1]) + ['--num_samples', '2', '--num_t', '3', '--patches']
    design.main(common + ['--force_collective', '--min_block', '1', '--output_dir', str(tmp_path / 'set')])
    design.main(common + ['--output_dir', str(tmp_path / 'sharded')])
    name = f'{CODES[0]}_patches.tsv'
    assert open(tmp_path / 'set' / name, 'rb').read() == open(tmp_path / 'sharded' / name, 'rb').read()


def test_one_surface_call_serves_five_tables(tmp_path, monkeypatch):
    """--interface --polar --developability --shape --patches: abx_interface_scores runs once per structure set (once inside the sampler
    call for the designs, once after it for the wild type), and the patches table is that of a run with --patches alone byte for byte."""
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
    flags = ['--interface', '--polar', '--developability', '--shape', '--patches']
    files = design.main(common + flags + ['--output_dir', str(tmp_path / 'all')])
    assert inside == [1] and calls == [2, 1], (inside, calls)
    assert [n for n in names(files) if n.endswith('.tsv')] == sorted(f'{CODES[0]}_{t}.tsv' for t in ('designs', 'developability', 'interface', 'patches', 'polar', 'shape'))
    del calls[:], inside[:]
    design.main(common + ['--patches', '--output_dir', str(tmp_path / 'patches')])
    assert inside == [1] and calls == [2, 1], (inside, calls)
    name = f'{CODES[0]}_patches.tsv'
    assert open(tmp_path / 'all' / name, 'rb').read() == open(tmp_path / 'patches' / name, 'rb').read()
    lines = table_lines(tmp_path / 'patches', CODES[0], 'patches')
    assert lines[1][0] == 'wild' and lines[1][12:18] == [str(v) for v in PC.PROTOTYPE['6ct7']['counts'][:6]]       # (all but the region's)
