"""GPU checks of the interface analysis (abx_interface_scores, csrc/interface.hip; abx_amd.interface.InterfaceScorer): the point counts
of every atom14 slot against the float64 host twin - equal, not close -, the input conventions shared with abx_design_scores, batch
independence at the headline size, and the path through the sampler and the design driver."""
import pytest
import torch

from analysis_gpu_cases import (ALONE, DEV, IDX13, assert_row as assert_columns, driver_pair, l352_designs, runs_of,
                                sample_tiny, sampler_pair, structure_inputs, table_lines, tiny_batch, typed_or_gt, ops, gpu_model)  # noqa: F401  (ops, gpu_model: set up once per importing module)
import relax_cases as RC

pytestmark = pytest.mark.gpu

AREA, COUNT = slice(0, 6), slice(6, 12)


_HOST = {}


def host(code, which, P, c=None):
    """Host twin (row, points) of one structure of a shipped complex, computed once per (complex, structure, P): which = 'wild' or
    (movable set, seed).  The region is always the movable set of `c` at the first request: the key carries it."""
    from abx_amd import interface
    key = (code, which, P)
    if key not in _HOST:
        x = c['x'] if which == 'wild' or which[1] is None else RC.perturb(c, which[1])
        _HOST[key] = interface.interface_host(x, c['mask'], c['aa'], c['Lab'], region=c['mov'], n_points=P)
    return _HOST[key]


def gpu_scores(ops, c, xs, P, Lp=None, mask='gt', points=True, **kw):
    """abx_interface_scores on structures xs (B,L,14,3) of complex c (rows >= Lp come from the crystal structure, which xs holds there)."""
    from abx_amd import interface
    x, sq, cplx, m, region = structure_inputs(c, xs, Lp, mask)
    pts = torch.full((xs.shape[0], c['aa'].shape[0], 14, 2), -7, dtype=torch.int32, device=DEV) if points else None
    kw.setdefault('region', region)
    row = ops.interface_scores(x, sq, *cplx, interface.sphere_points(P, DEV), Lab=c['Lab'], mask=m, points=pts, **kw)
    return row.cpu(), (pts.cpu() if points else None)


def assert_row(got, want, what):
    """integer columns equal; areas to 1e-10 relative (the order of the sums is the only freedom)."""
    assert_columns(got, want, COUNT, AREA, 1e-10, what)


@pytest.mark.parametrize('P', [128, 100, 960])
@pytest.mark.parametrize('code,sel', RC.MOVABLE_SETS)
def test_point_counts_equal_the_host_twin(ops, code, sel, P):
    """The wild type and the three seeded perturbations of every movable set in one batch: acc_alone / acc_cplx of EVERY slot of every
    structure equal the host twin's, so do the count columns; areas to 1e-10.  P = 100: a ragged last pass of the point loop."""
    c = RC.load_complex(code, sel)
    which = [(sel, None)] + [(sel, s) for s in RC.SEEDS]
    xs = torch.stack([c['x'].float().double()] + [RC.perturb(c, s) for s in RC.SEEDS])
    row, pts = gpu_scores(ops, c, xs, P)
    for b, w in enumerate(which):
        hrow, hpts = host(code, w, P, c)
        bad = torch.nonzero(pts[b] != torch.from_numpy(hpts))
        assert bad.shape[0] == 0, (code, sel, P, w, bad[:8].tolist(), pts[b][tuple(bad[0, :2])].tolist(), hpts[tuple(bad[0, :2].tolist())].tolist())
        assert torch.equal(pts[b], torch.from_numpy(hpts))
        assert_row(row[b], hrow, (code, sel, P, w))
        assert row[b, 11] == hrow[11] > 1000
    print(code, sel, P, 'dsasa_int', row[:, 3].tolist(), 'contacts', row[:, 9].tolist(), 'region', row[:, 5].tolist(), 'complex', row[:, 0].tolist())
    assert len({float(v) for v in row[:, 0]}) == 4                         # four different structures (6qd7's H3 is not at the interface)


def test_conventions_shared_with_design_scores(ops):
    """Lpred == Lab (antigen rows from the ground truth) and Lpred == L; pred_mask given and NULL; res_mask; out_stride > 12 and
    successive calls into one table."""
    from abx_amd import interface, residue_constants as rc
    c = RC.load_complex('6ct7', 'h3')
    L, Lab, P = c['aa'].shape[0], c['Lab'], 128
    xs = torch.stack([c['x'].float().double(), RC.perturb(c, 5)])
    full, pts_full = gpu_scores(ops, c, xs, P)
    ab, pts_ab = gpu_scores(ops, c, xs, P, Lp=Lab)
    assert torch.equal(full.view(torch.int64), ab.view(torch.int64)) and torch.equal(pts_full, pts_ab)
    # NULL pred_mask: predicted rows have the atoms of their residue type, the others those of the ground truth
    typed = torch.as_tensor(rc.restype_atom14_mask)[c['aa']].bool()
    for Lp in (Lab, L):
        m = torch.cat([typed[:Lp], c['mask'][Lp:]])[None].repeat(2, 1, 1)
        given, pts_g = gpu_scores(ops, c, xs, P, Lp=Lp, mask=m)
        null, pts_n = gpu_scores(ops, c, xs, P, Lp=Lp, mask=None)
        assert torch.equal(given.view(torch.int64), null.view(torch.int64)) and torch.equal(pts_g, pts_n), Lp
        hrow, hpts = interface.interface_host(xs[1], m[0], c['aa'], Lab, region=c['mov'], n_points=P)
        assert torch.equal(pts_n[1], torch.from_numpy(hpts))
        assert_row(null[1], hrow, ('NULL mask', Lp))
    # res_mask: a removed row is on neither side (an antibody and an antigen row of the interface)
    touched = (pts_full[0, ..., 0] > pts_full[0, ..., 1]).any(1)
    ra, rb = int(torch.nonzero(touched[:Lab])[0]), Lab + int(torch.nonzero(touched[Lab:])[0])
    keep = torch.ones(L, dtype=torch.bool)
    keep[[ra, rb]] = False
    cut, pts_cut = gpu_scores(ops, c, xs, P, res_mask=keep.to(DEV))
    assert not pts_cut[:, [ra, rb]].any() and bool((cut[:, 11] == full[:, 11] - float(c['mask'][[ra, rb]].sum())).all())
    hrow, hpts = interface.interface_host(xs[0], c['mask'] & keep[:, None], c['aa'], Lab, region=c['mov'], n_points=P)
    assert torch.equal(pts_cut[0], torch.from_numpy(hpts))
    assert_row(cut[0], hrow, 'res_mask')
    assert cut[0, 3] < full[0, 3]
    # rows of a wider table, and successive calls into one table
    table = torch.full((4, 16), -1.0, dtype=torch.float64, device=DEV)
    gpu_scores(ops, c, xs, P, points=False, out=table[:2, 2:14])
    gpu_scores(ops, c, xs[[1, 0]], P, points=False, out=table[2:, 2:14])
    t = table.cpu()
    assert torch.equal(t[:2, 2:14].view(torch.int64), full.view(torch.int64)) and torch.equal(t[[3, 2], 2:14].view(torch.int64), full.view(torch.int64))
    assert bool((t[:, :2] == -1).all()) and bool((t[:, 14:] == -1).all())
    # no region: its three columns are 0, the others do not change
    nore, _ = gpu_scores(ops, c, xs, P, points=False, region=None)
    assert nore[:, [5, 8, 10]].abs().max() == 0 and torch.equal(nore[:, [0, 1, 2, 3, 4, 6, 7, 9, 11]], full[:, [0, 1, 2, 3, 4, 6, 7, 9, 11]])
    assert full[0, 5] > 0 and full[0, 8] > 0 and full[0, 10] > 0


def test_a_structure_does_not_depend_on_its_batch():
    """L = 352 synthetic workload, B = 100 perturbed copies: rows 0, 57 and 99 are bit-identical alone, in a chunk of 13 and in the
    batch of 100; a second call repeats the first bit for bit; one structure against the host twin (compact random coordinates: far
    more neighbours per atom than a protein has, so the neighbour list is worked off several times per atom)."""
    from abx_amd import interface
    cx, xh, x, sq, _ = l352_designs()
    (B, Lab), L = sq.shape, cx['seq'].shape[0]
    sc = interface.InterfaceScorer({k: v.to(DEV) for k, v in cx.items()}, region=cx['cdr_def'] == 5)
    pts = torch.zeros(B, L, 14, 2, dtype=torch.int32, device=DEV)
    full = sc.score(x, sq, points=pts)
    again = sc.score(x, sq)
    assert full.shape == (B, len(interface.INTERFACE_COLUMNS)) and full.dtype == torch.float64
    assert torch.equal(full.view(torch.int64), again.view(torch.int64))
    h = full.cpu()
    print('L352 B=100: dsasa_int', h[:, 3].min().item(), h[:, 3].max().item(), 'contacts', h[:, 9].min().item(), h[:, 9].max().item(), 'atoms', h[0, 11].item())
    assert len({float(v) for v in h[:, 3]}) > 50 and bool((h[:, 11] == h[0, 11]).all())
    chunk = sc.score(x[IDX13], sq[IDX13])
    for j, b in enumerate(IDX13):
        assert torch.equal(chunk[j].view(torch.int64), full[b].view(torch.int64)), b
    for b in ALONE:
        alone = sc.score(x[b:b + 1], sq[b:b + 1])
        assert torch.equal(alone[0].view(torch.int64), full[b].view(torch.int64)), b
    xs = torch.cat([xh[57], cx['atom14_gt_positions'][Lab:].float()])
    hrow, hpts = interface.interface_host(xs, typed_or_gt(cx, Lab), cx['seq'], Lab, region=cx['cdr_def'] == 5, n_points=128)
    assert torch.equal(pts[57].cpu(), torch.from_numpy(hpts))
    assert_row(h[57], hrow, 'L352 structure 57')


def test_sampler_scores_the_last_record(gpu_model, cfg):
    """sample_fn(interface=) on the tiny workload: 'interface' sits on the last record only and equals a direct .score() of that
    record; with a relaxer also 'interface_relaxed'; with interface=None the records have exactly today's keys."""
    from abx_amd import interface, relax
    b, sid = tiny_batch(gpu_model)
    B = sid.shape[0]
    sc, relaxer = interface.InterfaceScorer(b), relax.ViolationRelaxer(b)
    dm = ((1 - b['fixed_mask'][0]) * b['atom14_gt_exists'][0, :, 0]) != 0
    assert torch.equal(sc.region.bool(), dm) and int(dm.sum()) > 0
    _, scored = sampler_pair(gpu_model, cfg, b, sid, ('interface', 'interface_relaxed'), interface=sc, relaxer=relaxer)
    last = scored[-1]
    NI = len(interface.INTERFACE_COLUMNS)
    assert last['interface'].shape == last['interface_relaxed'].shape == (B, NI) and last['interface'].dtype == torch.float64
    assert torch.equal(sc.score(last['atom14_results'], last['seq']).view(torch.int64), last['interface'].view(torch.int64))
    assert torch.equal(sc.score(last['atom14_relaxed'], last['seq']).view(torch.int64), last['interface_relaxed'].view(torch.int64))
    design = sample_tiny(gpu_model, cfg, b, sid, mode='design', interface=sc)
    assert len(design) == 1 and 'interface_relaxed' not in design[0]
    assert torch.equal(design[0]['interface'].view(torch.int64), last['interface'].view(torch.int64))
    row = last['interface'].cpu()
    print('tiny workload, interface rows', row.tolist(), 'wild', sc.wild().cpu().tolist())
    assert bool((row[:, 11] > 0).all()) and bool((row[:, 0] > 0).all()) and sc.wild().shape == (1, NI)


@pytest.mark.parametrize('collective', [False, True])
def test_design_driver_writes_the_interface_table(tmp_path, monkeypatch, collective):
    """`abx_amd.design --interface`: <complex>_interface.tsv with the header, the wild line and one line per sample whose fields are the
    sampler's records at print precision; every other file of the run is byte-identical to the run without the flag.  collective =
    False: the shipped 6ct7 complex with --relax --score (the relaxed columns follow).  collective = True: the 1-rank RCCL path on both
    shipped complexes, the table as further columns of the set-level gather."""
    from abx_amd import interface
    out, codes, N, seen = driver_pair(tmp_path, monkeypatch, 'interface', ['--interface'], collective, plain_extra=['--relax', '--score'])
    NI = len(interface.INTERFACE_COLUMNS)
    for code in codes:
        lines = table_lines(out, code, 'interface')
        head = ['sample'] + list(interface.INTERFACE_COLUMNS) + ['delta_' + c for c in interface.DELTA_COLUMNS]
        assert lines[0] == head + ([] if collective else [c + '_relaxed' for c in interface.INTERFACE_COLUMNS])
        assert len(lines) == 1 + 1 + N and all(len(r) == len(lines[0]) for r in lines)
        runs = runs_of(seen, code, collective)
        wild = runs[0][0].wild().cpu()[0].tolist()
        assert lines[1][:1 + NI] == ['wild'] + interface.format_interface(wild) and lines[1][1 + NI:1 + NI + 5] == ['+0.00', '+0.00', '+0.00', '+0', '+0']
        assert wild[9] == (119 if code.startswith('6ct7') else 1)            # the contacts of the crystal structure (any P)
        rows = torch.cat([tr[-1]['interface'] for _, tr in runs]).cpu().tolist()
        for i, r in enumerate(lines[2:]):
            assert r[0] == str(i) and r[1:1 + NI] == interface.format_interface(rows[i]), (code, i, r)
            assert r[1 + NI:1 + NI + 5] == interface.format_delta(rows[i], wild), (code, i, r)
        if not collective:
            relaxed = runs[0][1][-1]['interface_relaxed'].cpu().tolist()
            assert lines[1][1 + NI + 5:] == ['nan'] * NI
            for i, r in enumerate(lines[2:]):
                assert r[1 + NI + 5:] == interface.format_interface(relaxed[i]), (code, i)
