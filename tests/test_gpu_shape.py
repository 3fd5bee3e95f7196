"""GPU checks of the shape-complementarity analysis (abx_shape_scores, csrc/shape.hip; abx_amd.shape.ShapeScorer): the row against the
float64 host twin - the counts equal, the medians to 1e-12 -, the point densities, the LDS chunks of the match, the edge cases of the
trimming and of an interface that is not there, the capacity of the dot lists with guard words behind the workspace, batch independence
at the headline size, and the path through the sampler and the design driver, where the surface kernel is shared with the interface,
polar and developability analyses.

The bound of the float columns is derived, not measured: the selection of the dots and the tie-break of the match are exact, an order
statistic moves by at most the largest change of any of its inputs, and exp and sqrt differ by a few ulp (about 5e-16) between the
device and numpy."""
import numpy as np
import pytest
import torch

from analysis_gpu_cases import (ALONE, CODES, DEV, assert_row, driver_pair, l352_designs, names, pdb_args, runs_of, sample_tiny, sampler_pair,
                                set_master_port, spy_on_sampler, table_lines, tiny_batch, typed_or_gt, ops, gpu_model)  # noqa: F401  (ops, gpu_model: set up once per importing module)
import relax_cases as RC
import shape_cases as SC

pytestmark = pytest.mark.gpu

EQUAL, CLOSE, RTOL = list(range(6, 11)), list(range(6)), 1e-12
GUARD = 256


def bits(t):
    return t.contiguous().view(torch.int64)


def batch_of(c, **kw):
    return SC.batch_of(c, DEV, **kw)


def device_args(c, xs):
    """Antibody coordinates, tokens and the ground truth's atom mask of structures xs (B,L,14,3) of complex c on the device."""
    B, Lab = xs.shape[0], c['Lab']
    return xs[:, :Lab].float().to(DEV), c['aa'][None, :Lab].repeat(B, 1).to(DEV), c['mask'][None].repeat(B, 1, 1).to(DEV)


def guarded(sc, B, P, max_dots=None):
    """A workspace for B structures with GUARD bytes of 0xA5 behind it -> (tensor, bytes the entry may use)."""
    from abx_amd import ops as _ops
    need = _ops.shape_workspace_bytes(B, sc.L, P, sc.kw['max_dots'] if max_dots is None else max_dots)
    ws = torch.zeros(need + GUARD, dtype=torch.uint8, device=DEV)
    ws[need:] = 0xA5
    return ws, need


def assert_guard_intact(ws, need):
    assert bool((ws[need:] == 0xA5).all()), 'the words behind the workspace were written'


@pytest.mark.parametrize('code', ['6ct7', '6qd7'])
def test_rows_match_the_host_twin(ops, code):
    """The wild type and three seeded perturbations in one batch (B = 4, L = 231 / 259) against the host twin, with the scorer's own
    surface call and with the point counts handed over from InterfaceScorer.score; then with pred_mask NULL (the atoms of the residue
    types) and with a res_mask.  The host twin takes the device's point counts (their equality with interface_host is test_gpu_interface's
    subject); the wild type's are recomputed on the host as well."""
    from abx_amd import interface, residue_constants as rc, shape
    c = SC.complex_of(code)
    L, Lab = c['aa'].shape[0], c['Lab']
    xs = SC.structures(c)
    B = xs.shape[0]
    x, sq, gt = device_args(c, xs)
    batch = batch_of(c)
    it = interface.InterfaceScorer(batch, region=c['mov'])
    own, shared = shape.ShapeScorer(batch, region=c['mov']), shape.ShapeScorer(batch, interface=it)
    assert shared.interface is it and own.interface is not it and torch.equal(shared.region, own.region)
    pts = shared.new_points(B)
    it.score(x, sq, points=pts, mask=gt)
    a = own.score(x, sq, mask=gt)
    b = shared.score(x, sq, points=pts, mask=gt)
    assert a.shape == (B, 11) and a.dtype == torch.float64 and torch.equal(bits(a), bits(b))
    a, hp = a.cpu(), pts.cpu()
    for k in range(B):
        assert_row(a[k], SC.twin(c, xs[k], c['mask'], hp[k]), EQUAL, CLOSE, RTOL, (code, k))
    print(code, 'sc', a[:, 0].tolist(), 'sc_region', a[:, 3].tolist(), 'dots', a[:, 6:9].tolist(), 'trimmed', a[:, 9:].tolist())
    assert_row(a[0], SC.twin(c, xs[0], c['mask'], None), EQUAL, CLOSE, RTOL, (code, 'host points'))
    proto = SC.PROTOTYPE[code, 128]
    assert a[0, 6:9].tolist() == list(proto['kept']) + [proto['region']] and np.abs(a[0, :4].numpy() - np.array(proto['sc'])).max() <= 1e-3
    w = own.wild().cpu()[0]
    assert bits(w).tolist() == bits(a[0]).tolist() == bits(shared.wild(points=pts[:1].contiguous()).cpu()[0]).tolist()
    # pred_mask NULL: the predicted rows have the atoms of their residue type
    typed = torch.cat([torch.as_tensor(rc.restype_atom14_mask)[c['aa'][:Lab]].bool(), c['mask'][Lab:]])
    pts_n = own.new_points(2)
    it.score(x[:2], sq[:2], points=pts_n)
    null = own.score(x[:2], sq[:2]).cpu()
    for k in range(2):
        assert_row(null[k], SC.twin(c, xs[k], typed, pts_n[k].cpu()), EQUAL, CLOSE, RTOL, (code, 'NULL mask', k))
    # res_mask: a removed row has no atoms and no dots
    keep = torch.ones(L, dtype=torch.bool)
    keep[[3, 50, int(torch.nonzero(c['mov'])[0, 0])]] = False
    cut = shape.ShapeScorer(batch_of(c, res_mask=keep), region=c['mov'])
    pts_c = cut.new_points(1)
    cut.interface.score(x[1:2], sq[1:2], points=pts_c, mask=gt[:1])
    got = cut.score(x[1:2], sq[1:2], mask=gt[:1]).cpu()
    assert_row(got[0], SC.twin(c, xs[1], c['mask'] & keep[:, None], pts_c[0].cpu()), EQUAL, CLOSE, RTOL, (code, 'res_mask'))
    # rows of a wider table
    table = torch.full((B, 15), -7.0, dtype=torch.float64, device=DEV)
    shared.score(x, sq, points=pts, out=table[:, 2:13], mask=gt)
    t = table.cpu()
    assert torch.equal(bits(t[:, 2:13]), bits(a)) and bool((t[:, :2] == -7).all()) and bool((t[:, 13:] == -7).all())


@pytest.mark.parametrize('P', [32, 128, 512])
def test_point_densities(ops, P):
    """6ct7 and a perturbation at 32, 128 and 512 sphere points (one to eight passes of a wave over the points of an atom): the twin's
    row, the list sizes the issue's prototype printed, and Sc rising with the density as it found."""
    from abx_amd import shape
    c = SC.complex_of('6ct7')
    xs = torch.stack([c['x'].float().double(), RC.perturb(c, 6)])
    x, sq, gt = device_args(c, xs)
    sc = shape.ShapeScorer(batch_of(c), region=c['mov'], n_points=P)
    pts = sc.new_points(2)
    sc.interface.score(x, sq, points=pts, mask=gt)
    got = sc.score(x, sq, points=pts, mask=gt).cpu()
    for k in range(2):
        row, d = SC.twin(c, xs[k], c['mask'], pts[k].cpu(), n_points=P, details=True)
        assert_row(got[k], row, EQUAL, CLOSE, RTOL, (P, k))
        print('P', P, k, 'row', got[k].tolist(), 'buried', d['n_buried'], 'open', d['n_open'])
    assert bool((got[:, 6:8] > 0).all())
    if P in SC.DENSITY:
        assert abs(float(got[0, 0]) - SC.DENSITY[P]) <= 1e-3
    if P == 512:
        assert np.abs(got[0, 1:3].numpy() - np.array(SC.DENSITY_512)).max() <= 1e-3


@pytest.mark.parametrize('P,buried_atoms,kept,trimmed', [(65, 102, [39, 46], [144, 125]), (128, 115, [61, 48], [302, 309])])
def test_shared_point_test_at_its_edges(ops, P, buried_atoms, kept, trimmed):
    """The point test that iface_points_kernel and shape_dots_kernel share (csrc/surface_dev.h) at the smallest case that crosses its
    edges: 16 Trp rows (Lab = 8, all 14 slots) in a 7 A box.  Every one of the 224 atoms has 92 to 223 neighbours inside the prefilter,
    so its 192-entry list is worked off and refilled with a remainder, and the 224 atoms are three and a half 64-atom steps of the scan.
    P = 65: a second pass over the points with one live lane.  The point counts and the interface row equal interface_host's; the shape
    row on those counts equals shape_host's (a disagreement of the two kernels would make it eleven -1).  The literals are the host's."""
    from abx_amd import interface, shape
    L, Lab = 16, 8
    x = (torch.rand(L, 14, 3, generator=torch.Generator().manual_seed(5)) * 7.0).float()
    aa, mask = torch.full((L,), 17, dtype=torch.int64), torch.ones(L, 14, dtype=torch.bool)
    batch = {'seq': aa.to(DEV), 'atom14_gt_positions': x.to(DEV), 'atom14_gt_exists': mask.to(DEV), 'anchor_flag': torch.zeros(Lab)}
    it = interface.InterfaceScorer(batch, region=torch.zeros(L), n_points=P)
    sc = shape.ShapeScorer(batch, region=torch.zeros(L), n_points=P, interface=it)
    xa, sq = x[None, :Lab].to(DEV), aa[None, :Lab].to(DEV)
    pts = sc.new_points(1)
    irow = it.score(xa, sq, points=pts).cpu()[0]
    srow = sc.score(xa, sq, points=pts).cpu()[0]
    hrow, hpts = interface.interface_host(x, mask, aa, Lab, n_points=P)
    print('P', P, 'interface', irow.tolist(), 'shape', srow.tolist())
    assert torch.equal(pts.cpu()[0], torch.from_numpy(hpts))
    assert int((hpts[..., 0] > hpts[..., 1]).sum()) == buried_atoms
    assert_row(irow, hrow, list(range(6, 12)), list(range(6)), 1e-10, ('interface', P))
    assert irow[9] == 4349 and irow[11] == 224
    want = shape.shape_host(x, mask, aa, Lab, points=hpts, n_points=P)
    assert_row(srow, want, EQUAL, CLOSE, RTOL, ('shape', P))
    assert srow.tolist() != [-1.0] * 11 and srow[6:8].tolist() == kept and srow[9:].tolist() == trimmed


def test_lds_chunks_give_the_same_rows(ops):
    """j_chunk = 64 on 6ct7: nine chunks of the antigen's 532 kept dots with a ragged last one (and three tiles of 256 of them as the
    matched side, the last one ragged too) give the bits of the default chunk; so do 1 and 100."""
    from abx_amd import shape
    c = SC.complex_of('6ct7')
    xs = torch.stack([c['x'].float().double(), RC.perturb(c, 5)])
    x, sq, gt = device_args(c, xs)
    sc = shape.ShapeScorer(batch_of(c), region=c['mov'])
    pts = sc.new_points(2)
    sc.interface.score(x, sq, points=pts, mask=gt)
    base = sc.score(x, sq, points=pts, mask=gt)
    assert base[0, 6:8].cpu().tolist() == [347.0, 532.0]
    assert_row(base[0].cpu(), SC.twin(c, xs[0], c['mask'], pts[0].cpu()), EQUAL, CLOSE, RTOL, 'default chunk')
    for chunk in (64, 100, 1):
        assert torch.equal(bits(sc.score(x, sq, points=pts, mask=gt, j_chunk=chunk)), bits(base)), chunk


def test_trim_and_weight_edge_cases(ops):
    """trim = 0 keeps every buried dot; trim = 1e4 drops every dot of a side that has an open dot at all; weight = 0 leaves the plain
    median of -n.n.  On 6qd7 the default trim leaves 8 / 0 dots: every Sc column is 0 and the counts say why."""
    from abx_amd import shape
    for code in ('6ct7', '6qd7'):
        c = SC.complex_of(code)
        xs = torch.stack([c['x'].float().double(), RC.perturb(c, 7)])
        x, sq, gt = device_args(c, xs)
        for kw in (dict(trim=0.0), dict(trim=1e4), dict(weight=0.0), dict(trim=0.0, weight=0.0)):
            sc = shape.ShapeScorer(batch_of(c), region=c['mov'], **kw)
            pts = sc.new_points(2)
            sc.interface.score(x, sq, points=pts, mask=gt)
            got = sc.score(x, sq, points=pts, mask=gt).cpu()
            for k in range(2):
                row, d = SC.twin(c, xs[k], c['mask'], pts[k].cpu(), details=True, **kw)
                assert_row(got[k], row, EQUAL, CLOSE, RTOL, (code, kw, k))
                if kw.get('trim') == 0.0:
                    assert got[k, 6:8].tolist() == list(d['n_buried']) and got[k, 9:].tolist() == [0.0, 0.0]
                if kw.get('trim') == 1e4:
                    assert got[k].tolist() == [0.0] * 9 + [float(n) for n in d['n_buried']]
        sc = shape.ShapeScorer(batch_of(c), region=c['mov'])
        w = sc.wild().cpu()[0]
        proto = SC.PROTOTYPE[code, 128]
        assert w[6:8].tolist() == list(proto['kept']) and (w[6:8] + w[9:]).tolist() == list(proto['buried'])
    assert w[:6].tolist() == [0.0] * 6                                          # (6qd7: 8 / 0 dots)


def test_no_interface_and_glycines(ops):
    """The antigen moved 100 A away: no atom is named, the empty lists are never read and the row is zero.  All-Gly tokens: backbone
    atoms only, against the twin."""
    from abx_amd import shape
    c = SC.complex_of('6ct7')
    Lab = c['Lab']
    far = SC.antigen_moved(c)
    sc = shape.ShapeScorer(batch_of(c, x=far), region=c['mov'])
    xs = torch.stack([far, far])
    x, sq, gt = device_args(c, xs)
    ws, need = guarded(sc, 2, 128)
    got = sc.score(x, sq, mask=gt, workspace=ws).cpu()
    assert got.tolist() == [[0.0] * 11] * 2 and SC.twin(c, far, c['mask'], None).tolist() == [0.0] * 11
    assert_guard_intact(ws, need)
    sc = shape.ShapeScorer(batch_of(c), region=c['mov'])
    xs = torch.stack([c['x'].float().double(), RC.perturb(c, 6)])
    x, sq, _ = device_args(c, xs)
    gly = torch.full_like(sq, SC.G)
    pts = sc.new_points(2)
    sc.interface.score(x, gly, points=pts)
    got = sc.score(x, gly, points=pts).cpu()
    seq = c['aa'].clone()
    seq[:Lab] = SC.G
    gmask = torch.cat([torch.tensor([True] * 4 + [False] * 10)[None].repeat(Lab, 1), c['mask'][Lab:]])
    for k in range(2):
        assert_row(got[k], SC.twin(c, xs[k], gmask, pts[k].cpu(), seq=seq), EQUAL, CLOSE, RTOL, ('all Gly', k))
    assert bool((got[:, 6:8] > 0).all())


def test_capacity_and_foreign_points(ops):
    """max_dots = 64 on 6ct7 (701 / 881 buried dots): the row is eleven -1, the guard words behind the workspace are intact, and the other
    structure of the batch - the antibody moved 14 A off: 8 / 8 buried and 51 / 64 open dots, the largest list exactly at the capacity -
    has the row it has with the default capacity (trim = 0, so that its few dots are kept).  The point counts of ANOTHER structure: -1 as
    well, nothing written past a promised segment or the workspace."""
    from abx_amd import shape
    c = SC.complex_of('6ct7')
    small = SC.antibody_moved(c, SC.SMALL_SHIFT)
    xs = torch.stack([c['x'].float().double(), small, RC.perturb(c, 6)])
    x, sq, gt = device_args(c, xs)
    big, tight = shape.ShapeScorer(batch_of(c), region=c['mov'], trim=0.0), shape.ShapeScorer(batch_of(c), region=c['mov'], trim=0.0, max_dots=64)
    pts = big.new_points(3)
    big.interface.score(x, sq, points=pts, mask=gt)
    want = big.score(x, sq, points=pts, mask=gt).cpu()
    row, d = SC.twin(c, xs[1], c['mask'], pts[1].cpu(), details=True, trim=0.0, max_dots=64)
    assert (d['n_buried'], d['n_open'], d['n_kept']) == ((8, 8), (51, 64), (8, 8)), d
    assert_row(want[1], row, EQUAL, CLOSE, RTOL, 'small interface')
    ws, need = guarded(tight, 3, 128)
    got = tight.score(x, sq, points=pts, mask=gt, workspace=ws).cpu()
    assert_guard_intact(ws, need)
    assert got[0].tolist() == got[2].tolist() == [-1.0] * 11 and bits(got[1]).tolist() == bits(want[1]).tolist()
    assert SC.twin(c, xs[0], c['mask'], pts[0].cpu(), max_dots=64).tolist() == [-1.0] * 11
    # the counts of structure 2 handed in for structure 0 and the other way round; structure 1 keeps its own
    swapped = pts[[2, 1, 0]].contiguous()
    ws, need = guarded(big, 3, 128)
    got = big.score(x, sq, points=swapped, mask=gt, workspace=ws).cpu()
    assert_guard_intact(ws, need)
    assert got[0].tolist() == got[2].tolist() == [-1.0] * 11 and bits(got[1]).tolist() == bits(want[1]).tolist()
    assert SC.twin(c, xs[0], c['mask'], swapped[0].cpu()).tolist() == [-1.0] * 11
    # counts that cannot be: more buried points than the sphere has
    broken = pts.clone()
    broken[0, 5, 1, 0] = 129
    assert big.score(x, sq, points=broken, mask=gt).cpu()[0].tolist() == [-1.0] * 11


def test_a_structure_does_not_depend_on_its_batch():
    """L = 352 synthetic workload, B = 100 perturbed copies: the rows of structures 0, 57 and 99 scored alone equal their rows in the
    batch bit for bit; a second call repeats the first; structure 57 matches the host twin."""
    from abx_amd import shape
    cx, xh, x, sq, _ = l352_designs()
    (B, Lab), L = sq.shape, cx['seq'].shape[0]
    sc = shape.ShapeScorer({k: v.to(DEV) for k, v in cx.items()}, region=cx['cdr_def'] == 5)
    pts = sc.new_points(B)
    sc.interface.score(x, sq, points=pts)
    full = sc.score(x, sq, points=pts)
    again = sc.score(x, sq, points=pts)
    assert full.shape == (B, 11) and torch.equal(bits(full), bits(again))
    h = full.cpu()
    print('L352 B=100: sc', h[:, 0].min().item(), h[:, 0].max().item(), 'dots', h[:, 6].min().item(), h[:, 6].max().item(), h[:, 7].min().item(), h[:, 7].max().item())
    assert bool((h >= 0).all()) and len({tuple(r) for r in h.tolist()}) > 50
    for b in ALONE:
        alone = sc.score(x[b:b + 1], sq[b:b + 1], points=pts[b:b + 1].contiguous())
        assert torch.equal(bits(alone[0]), bits(full[b])), b
    xs = torch.cat([xh[57], cx['atom14_gt_positions'][Lab:].float()])
    row = shape.shape_host(xs, typed_or_gt(cx, Lab, typed=True), cx['seq'], Lab, region=cx['cdr_def'] == 5, points=pts[57].cpu())
    assert_row(h[57], row, EQUAL, CLOSE, RTOL, 'L352 structure 57')


def test_sampler_scores_the_last_record(gpu_model, cfg):
    """sample_fn(shape=) on the tiny workload: the plain trajectory is unchanged, 'shape' sits on the last record only and equals a direct
    .score() of that record; with a relaxer also 'shape_relaxed'; sharing the interface scorer changes no table."""
    from abx_amd import interface, relax, shape
    b, sid = tiny_batch(gpu_model)
    B = sid.shape[0]
    NS = len(shape.SHAPE_COLUMNS)
    sc = shape.ShapeScorer(b)
    _, scored = sampler_pair(gpu_model, cfg, b, sid, ('shape',), shape=sc)
    last = scored[-1]
    assert last['shape'].shape == (B, NS) and last['shape'].dtype == torch.float64
    assert not {'shape_relaxed', 'interface'} & set(last)
    assert torch.equal(bits(sc.score(last['atom14_results'], last['seq'])), bits(last['shape']))
    it = interface.InterfaceScorer(b)
    sh = shape.ShapeScorer(b, interface=it)
    full = sample_tiny(gpu_model, cfg, b, sid, mode='design', shape=sh, interface=it, relaxer=relax.ViolationRelaxer(b))
    assert len(full) == 1
    rec = full[0]
    assert torch.equal(bits(rec['shape']), bits(last['shape']))
    assert torch.equal(bits(sh.score(rec['atom14_results'], rec['seq'])), bits(rec['shape']))
    assert torch.equal(bits(sh.score(rec['atom14_relaxed'], rec['seq'])), bits(rec['shape_relaxed']))
    assert torch.equal(bits(it.score(rec['atom14_results'], rec['seq'])), bits(rec['interface']))
    print('tiny workload, shape rows', rec['shape'].cpu().tolist(), 'wild', sc.wild().cpu().tolist())
    assert bool((rec['shape'] >= 0).all()) and sc.wild().shape == (1, NS)


@pytest.mark.parametrize('collective', [False, True])
def test_design_driver_writes_the_shape_table(tmp_path, monkeypatch, collective):
    """`abx_amd.design --shape` alone: <complex>_shape.tsv with the header, the wild line and one line per sample whose fields are the
    sampler's records at print precision; every other file of the run is byte-identical to the run without the flag.
    collective = False: the shipped 6ct7 complex with --relax (the relaxed columns follow), sample-sharded.  collective = True: the
    1-rank RCCL path on both shipped complexes, the table as further columns of the set-level gather - the same wild lines."""
    from abx_amd import shape
    out, codes, N, seen = driver_pair(tmp_path, monkeypatch, 'shape', ['--shape'], collective, plain_extra=['--relax', '--relax_iters', '20'])
    NS, NDELTA = len(shape.SHAPE_COLUMNS), len(shape.DELTA_COLUMNS)
    for code in codes:
        lines = table_lines(out, code, 'shape')
        head = ['sample'] + list(shape.SHAPE_COLUMNS) + ['delta_' + c for c in shape.DELTA_COLUMNS]
        assert lines[0] == head + ([] if collective else [c + '_relaxed' for c in shape.SHAPE_COLUMNS])
        assert len(lines) == 1 + 1 + N and all(len(r) == len(lines[0]) for r in lines)
        runs = runs_of(seen, code, collective)
        wild = runs[0][0].wild().cpu()[0].tolist()
        assert lines[1][:1 + NS] == ['wild'] + shape.format_shape(wild)
        assert lines[1][1 + NS:1 + NS + NDELTA] == shape.format_delta(wild, wild) == ['+0.0000'] * 4 + ['+0'] * 3
        proto = SC.PROTOTYPE[code[:4], 128]
        assert wild[6:8] == list(proto['kept']) and abs(float(lines[1][1]) - proto['sc'][0]) <= 1e-3
        rows = torch.cat([tr[-1]['shape'] for _, tr in runs]).cpu().tolist()
        for i, r in enumerate(lines[2:]):
            assert r[0] == str(i) and r[1:1 + NS] == shape.format_shape(rows[i]), (code, i, r)
            assert r[1 + NS:1 + NS + NDELTA] == shape.format_delta(rows[i], wild), (code, i, r)
        if not collective:
            relaxed = runs[0][1][-1]['shape_relaxed'].cpu().tolist()
            assert lines[1][1 + NS + NDELTA:] == ['nan'] * NS
            for i, r in enumerate(lines[2:]):
                assert r[1 + NS + NDELTA:] == shape.format_shape(relaxed[i]) and 'nan' not in r, (code, i)


def test_set_level_and_sharded_runs_write_the_same_table(tmp_path, monkeypatch):
    """The set-level schedule (1-rank RCCL path, rows gathered) and the sample-sharded one write the same <complex>_shape.tsv."""
    from abx_amd import design
    set_master_port(monkeypatch)
    common = pdb_args(CODES[:1]) + ['--num_samples', '2', '--num_t', '3', '--shape']
    design.main(common + ['--force_collective', '--min_block', '1', '--output_dir', str(tmp_path / 'set')])
    design.main(common + ['--output_dir', str(tmp_path / 'sharded')])
    name = f'{CODES[0]}_shape.tsv'
    assert open(tmp_path / 'set' / name, 'rb').read() == open(tmp_path / 'sharded' / name, 'rb').read()


def test_one_surface_call_serves_four_tables(tmp_path, monkeypatch):
    """--interface --polar --developability --shape: abx_interface_scores runs once per structure set (once inside the sampler call for
    the designs, once after it for the wild type), and the shape table is that of a run with --shape alone byte for byte."""
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
    flags = ['--interface', '--polar', '--developability', '--shape']
    files = design.main(common + flags + ['--output_dir', str(tmp_path / 'all')])
    assert inside == [1] and calls == [2, 1], (inside, calls)
    assert [n for n in names(files) if n.endswith('.tsv')] == sorted(f'{CODES[0]}_{t}.tsv' for t in ('designs', 'developability', 'interface', 'polar', 'shape'))
    del calls[:], inside[:]
    design.main(common + ['--shape', '--output_dir', str(tmp_path / 'shape')])
    assert inside == [1] and calls == [2, 1], (inside, calls)
    for t in ('shape',):
        name = f'{CODES[0]}_{t}.tsv'
        assert open(tmp_path / 'all' / name, 'rb').read() == open(tmp_path / 'shape' / name, 'rb').read()
    lines = table_lines(tmp_path / 'shape', CODES[0], 'shape')
    assert lines[1][0] == 'wild' and lines[1][7:9] == ['347', '532']
