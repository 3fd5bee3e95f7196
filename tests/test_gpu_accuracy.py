"""GPU checks of the accuracy analysis (abx_accuracy_scores, csrc/accuracy.hip; abx_amd.accuracy.AccuracyScorer): the per-residue pair
counts and the residue-contact bits against the float64 host twin - equal, not close (tests/test_accuracy_host.py shows that no decision
of these structures is borderline) -, the input conventions shared with abx_design_scores, batch independence at the headline size, and
the path through the sampler and the design driver."""
import os

import numpy as np
import pytest
import torch

import accuracy_cases as AC
from analysis_gpu_cases import (ALONE, CODES, DEV, IDX13, assert_row as assert_columns, driver_pair, l352_designs, runs_of,
                                sample_tiny, sampler_pair, structure_inputs, table_lines, tiny_batch, typed_or_gt, ops, gpu_model)  # noqa: F401  (ops, gpu_model: set up once per importing module)
import relax_cases as RC

pytestmark = pytest.mark.gpu

GDT = [9, 10]
COUNT = [12, 13, 15, 16, 17, 19, 20]
FLOAT = [0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 14, 18]


def gpu_scores(ops, c, xs, aas=None, Lp=None, mask='gt', extras=True, **kw):
    """abx_accuracy_scores on structures xs (B,L,14,3) of complex c (rows >= Lp come from the crystal structure, which xs holds there).
    -> (table, rows, counts, contacts) on the host."""
    B, L, Lab = xs.shape[0], c['aa'].shape[0], c['Lab']
    x, sq, cplx, m, region = structure_inputs(c, xs, Lp, mask)
    sq = sq if aas is None else aas[:, :Lab].to(DEV)
    kw.setdefault('region', region)
    rows = torch.full((B, L, 4), -7.0, dtype=torch.float64, device=DEV) if extras else None
    counts = torch.full((B, L, 3, 5), -7, dtype=torch.int32, device=DEV) if extras else None
    contacts = torch.full((B, Lab, L - Lab), 77, dtype=torch.uint8, device=DEV) if extras else None
    table = ops.accuracy_scores(x, sq, *cplx, Lab=Lab, mask=m, rows=rows, counts=counts, contacts=contacts, **kw)
    cpu = lambda t: None if t is None else t.cpu()
    return table.cpu(), cpu(rows), cpu(counts), cpu(contacts)


def assert_row(got, want, what):
    """count and GDT columns equal; the other columns to 1e-9 relative (the order of the sums and the last bit of the square root are
    the only freedom); nan where the twin says nan."""
    assert_columns(got, want, COUNT + GDT, [], 0.0, what)
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    ok = ~np.isnan(want[FLOAT])
    err = np.abs(got[FLOAT][ok] - want[FLOAT][ok]) / np.maximum(np.abs(want[FLOAT][ok]), 1e-300)
    small = np.abs(want[FLOAT][ok]) < 1e-6                                   # rmsd_ca of an identical structure: 0 against ~1e-7
    assert float(np.where(small, 0.0, err).max()) <= 1e-9 and float(np.abs(got[FLOAT][ok] - want[FLOAT][ok])[small].max(initial=0.0)) <= 1e-6, \
        (what, got[FLOAT], want[FLOAT])


def assert_structure(got, b, h, what):
    table, rows, counts, contacts = got
    bad = torch.nonzero(counts[b] != torch.from_numpy(h['counts']))
    assert bad.shape[0] == 0, (what, bad[:8].tolist(), counts[b][tuple(bad[0, :2])].tolist(), h['counts'][tuple(bad[0, :2].tolist())].tolist())
    assert torch.equal(contacts[b], torch.from_numpy(h['contacts'])), (what, torch.nonzero(contacts[b] != torch.from_numpy(h['contacts']))[:8].tolist())
    assert_row(table[b], h['row'], what)
    assert np.array_equal(rows[b, :, 3].numpy(), h['rows'][:, 3]) and np.array_equal(np.isnan(rows[b].numpy()), np.isnan(h['rows'])), what
    assert np.allclose(rows[b].numpy(), h['rows'], rtol=1e-12, atol=0, equal_nan=True), what


@pytest.mark.parametrize('code,sel', RC.MOVABLE_SETS)
def test_counts_equal_the_host_twin(ops, code, sel):
    """The wild type, the three seeded perturbations and their mutated versions (new tokens, typed atoms) of every movable set in one
    batch, with a per-residue pLDDT: `counts` and `contacts` of EVERY row equal the host twin's, so do the count and GDT columns; the
    other columns to 1e-9.  L = 259 and 231: the last tile is ragged."""
    c = RC.load_complex(code, sel)
    L = c['aa'].shape[0]
    assert L % 16 != 0
    pert = [RC.perturb(c, s) for s in RC.SEEDS]
    mut = [AC.mutate(c, x, s) for x, s in zip(pert, RC.SEEDS)]
    xs = torch.stack([c['x'].float().double()] + pert + [m[0] for m in mut])
    aas = torch.stack([c['aa']] * 4 + [m[1] for m in mut])
    masks = torch.stack([c['mask']] * 4 + [m[2] for m in mut])
    pl = (40.0 + 55.0 * torch.rand(7, L, generator=torch.Generator().manual_seed(3))).float()
    got = gpu_scores(ops, c, xs, aas, mask=masks, plddt=pl.to(DEV))
    for b in range(7):
        h = AC.host(c, xs[b], aas[b], masks[b], plddt=pl[b])
        assert h['n_borderline'] == 0 and h['n_borderline_gdt'] == 0
        assert_structure(got, b, h, (code, sel, b))
    t = got[0]
    print(code, sel, 'lddt_region', t[:, 2].tolist(), 'fnat', t[:, 14].tolist(), 'tm', t[:, 8].tolist(), 'plddt_err', t[:, 7].tolist())
    assert t[0, :6].tolist() == [1.0] * 6 and t[0, 14] == 1.0 and t[0, 11] < 1e-6 and bool((t[1:, 2] < 0.9).all())
    assert bool((t[4:, 20] < t[0, 20]).all()) and bool((t[:, 7] > 0).all())


def test_conventions_shared_with_design_scores(ops):
    """Lpred == Lab (antigen rows from the ground truth) and Lpred == L; pred_mask given and NULL; res_mask; no region; no pLDDT;
    out_stride > 21 and successive calls into one table; the tiny workload (L below one tile); L == Lab."""
    from abx_amd import accuracy, residue_constants as rc, synthetic
    c = RC.load_complex('6ct7', 'h3')
    L, Lab = c['aa'].shape[0], c['Lab']
    xs = torch.stack([c['x'].float().double(), RC.perturb(c, 5)])
    bits = lambda t: t.view(torch.int64)
    full = gpu_scores(ops, c, xs)
    ab = gpu_scores(ops, c, xs, Lp=Lab)
    assert all(torch.equal(p, q) for p, q in zip((bits(full[0]), bits(full[1]), full[2], full[3]), (bits(ab[0]), bits(ab[1]), ab[2], ab[3])))
    # NULL pred_mask: predicted rows have the atoms of their residue type, the others those of the ground truth
    typed = torch.as_tensor(rc.restype_atom14_mask)[c['aa']].bool()
    for Lp in (Lab, L):
        m = torch.cat([typed[:Lp], c['mask'][Lp:]])[None].repeat(2, 1, 1)
        given = gpu_scores(ops, c, xs, Lp=Lp, mask=m)
        null = gpu_scores(ops, c, xs, Lp=Lp, mask=None)
        assert torch.equal(bits(given[0]), bits(null[0])) and torch.equal(given[2], null[2]) and torch.equal(given[3], null[3]), Lp
        assert_structure(null, 1, AC.host(c, xs[1], mask=m[0]), ('NULL mask', Lp))
    # res_mask: a removed row is in neither structure (an antibody and an antigen row in contact)
    ra, rb = (int(v) for v in torch.nonzero(full[3][0] == 3)[0])
    rb += Lab
    keep = torch.ones(L, dtype=torch.bool)
    keep[[ra, rb]] = False
    cut = gpu_scores(ops, c, xs, res_mask=keep.to(DEV))
    assert not cut[2][:, [ra, rb]].any() and not cut[3][:, ra].any() and not cut[3][:, :, rb - Lab].any()
    assert bool((cut[0][:, 20] == full[0][:, 20] - float(c['mask'][[ra, rb]].sum())).all()) and bool((cut[0][:, 12] < full[0][:, 12]).all())
    for b in (0, 1):
        assert_structure(cut, b, AC.host(c, xs[b], res_mask=keep), ('res_mask', b))
    # rows of a wider table, and successive calls into one table
    table = torch.full((4, 26), -1.0, dtype=torch.float64, device=DEV)
    gpu_scores(ops, c, xs, extras=False, out=table[:2, 2:23])
    gpu_scores(ops, c, xs[[1, 0]], extras=False, out=table[2:, 2:23])
    t = table.cpu()
    assert torch.equal(bits(t[:2, 2:23].contiguous()), bits(full[0])) and torch.equal(bits(t[[3, 2], 2:23].contiguous()), bits(full[0]))
    assert bool((t[:, :2] == -1).all()) and bool((t[:, 23:] == -1).all())
    # no region: its columns are nan / 0, the others do not change; no pLDDT: columns 6 and 7 are nan
    nore = gpu_scores(ops, c, xs, extras=False, region=None)[0]
    assert bool(torch.isnan(nore[:, [2, 3, 5, 6, 7, 18]]).all()) and bool((nore[:, [16, 17, 19]] == 0).all())
    same = [0, 1, 4, 8, 9, 10, 11, 12, 13, 14, 15, 20]
    assert torch.equal(bits(nore[:, same].contiguous()), bits(full[0][:, same].contiguous()))
    assert bool(torch.isnan(full[0][:, [6, 7]]).all()) and full[0][1, 19] > 0 and full[0][1, 16] == 9
    pl = torch.full((2, L), 80.0)
    with_pl = gpu_scores(ops, c, xs, extras=False, plddt=pl.to(DEV))[0]
    assert with_pl[:, 6].tolist() == [80.0, 80.0] and abs(float(with_pl[0, 7]) - 20.0) < 1e-12 and with_pl[1, 7] > 0
    assert torch.equal(bits(with_pl[:, 8:].contiguous()), bits(full[0][:, 8:].contiguous()))
    # the tiny workload: L = 20 in two tiles, Lab = 16; and the antibody alone, L == Lab: no contacts
    cx = synthetic.make_complex(seed=3, **synthetic.WORKLOADS['tiny'])
    Lt, Labt = cx['seq'].shape[0], cx['anchor_flag'].shape[0]
    g = torch.Generator().manual_seed(4)
    xt = (cx['atom14_gt_positions'][None] + 0.4 * torch.randn(3, Lt, 14, 3, generator=g)).float()
    xt[:, Labt:] = cx['atom14_gt_positions'][Labt:]
    tiny = dict(x=cx['atom14_gt_positions'].double(), mask=cx['atom14_gt_exists'].bool(), aa=cx['seq'].long(), Lab=Labt, mov=cx['cdr_def'] == 5)
    got = gpu_scores(ops, tiny, xt.double())
    for b in range(3):
        assert_structure(got, b, AC.host(tiny, xt[b].double()), ('tiny', b))
    alone = {k: (v[:Labt] if torch.is_tensor(v) else v) for k, v in tiny.items()}
    got = gpu_scores(ops, alone, xt[:, :Labt].double())
    assert got[3].shape == (3, Labt, 0) and bool((got[0][:, [12, 13, 15, 16, 17]] == 0).all()) and bool(torch.isnan(got[0][:, [14, 18]]).all())
    for b in range(3):
        h = accuracy.accuracy_host(xt[b, :Labt], alone['mask'], alone['aa'], alone['x'], alone['mask'], alone['aa'], Labt, region=alone['mov'])
        assert_structure(got, b, h, ('L == Lab', b))


def test_a_structure_does_not_depend_on_its_batch():
    """L = 352 synthetic workload, B = 100 perturbed copies: rows 0, 57 and 99 are bit-identical alone, in a chunk of 13 and in the
    batch of 100; a second call repeats the first bit for bit; structure 57 against the host twin."""
    from abx_amd import accuracy
    cx, xh, x, sq, g = l352_designs()
    (B, Lab), L = sq.shape, cx['seq'].shape[0]
    pl = (40.0 + 55.0 * torch.rand(B, L, generator=g)).float()
    sc = accuracy.AccuracyScorer({k: v.to(DEV) for k, v in cx.items()}, region=cx['cdr_def'] == 5)
    full, rows, counts, contacts = sc.score(x, sq, plddt=pl.to(DEV), rows=True, counts=True, contacts=True)
    again = sc.score(x, sq, plddt=pl.to(DEV), rows=True, counts=True, contacts=True)
    assert full.shape == (B, len(accuracy.ACCURACY_COLUMNS)) and full.dtype == torch.float64
    bits = lambda t: t.contiguous().view(torch.int64)
    assert torch.equal(bits(full), bits(again[0])) and torch.equal(bits(rows), bits(again[1])) and torch.equal(counts, again[2]) and torch.equal(contacts, again[3])
    h = full.cpu()
    print('L352 B=100: lddt_all', h[:, 0].min().item(), h[:, 0].max().item(), 'lddt_region', h[:, 2].min().item(), h[:, 2].max().item(),
          'tm', h[:, 8].min().item(), 'native', h[0, 12].item(), 'kept', h[:, 13].min().item(), h[:, 13].max().item(), 'scored atoms', h[0, 20].item())
    assert len({float(v) for v in h[:, 0]}) > 50 and bool((h[:, 20] == h[0, 20]).all()) and bool((h[:, 12] == h[0, 12]).all())
    chunk = sc.score(x[IDX13], sq[IDX13], plddt=pl[IDX13].to(DEV))
    for j, b in enumerate(IDX13):
        assert torch.equal(bits(chunk[j]), bits(full[b])), b
    for b in ALONE:
        alone = sc.score(x[b:b + 1], sq[b:b + 1], plddt=pl[b:b + 1].to(DEV))
        assert torch.equal(bits(alone[0]), bits(full[b])), b
    xs = torch.cat([xh[57], cx['atom14_gt_positions'][Lab:].float()])
    hh = accuracy.accuracy_host(xs, typed_or_gt(cx, Lab, typed=True), cx['seq'], cx['atom14_gt_positions'], cx['atom14_gt_exists'], cx['seq'], Lab,
                                region=cx['cdr_def'] == 5, res_mask=cx['mask'].bool(), plddt=pl[57])
    assert hh['n_borderline'] == 0 and hh['n_borderline_gdt'] == 0
    assert_structure((h, rows.cpu(), counts.cpu(), contacts.cpu()), 57, hh, 'L352 structure 57')


def test_sampler_scores_the_last_record(gpu_model, cfg, monkeypatch):
    """sample_fn(accuracy=) on the tiny workload: 'accuracy' and 'accuracy_rows' sit on the last record only and equal a direct .score()
    of that record with the per-residue pLDDT of that call; with a relaxer also 'accuracy_relaxed'; with accuracy=None the records have
    exactly today's keys and equal tensors."""
    from abx_amd import accuracy, relax
    b, sid = tiny_batch(gpu_model)
    B = sid.shape[0]
    sc, relaxer = accuracy.AccuracyScorer(b), relax.ViolationRelaxer(b)
    dm = ((1 - b['fixed_mask'][0]) * b['atom14_gt_exists'][0, :, 0]) != 0
    assert torch.equal(sc.region.bool(), dm) and int(dm.sum()) > 0
    seen = []
    real = sc.score
    monkeypatch.setattr(sc, 'score', lambda *a, **kw: (seen.append(kw['plddt'].clone()) if kw.get('plddt') is not None else None, real(*a, **kw))[1])
    _, scored = sampler_pair(gpu_model, cfg, b, sid, ('accuracy', 'accuracy_rows', 'accuracy_relaxed'), accuracy=sc, relaxer=relaxer)
    last = scored[-1]
    NA, L = len(accuracy.ACCURACY_COLUMNS), b['seq'].shape[1]
    assert last['accuracy'].shape == last['accuracy_relaxed'].shape == (B, NA) and last['accuracy'].dtype == torch.float64
    assert last['accuracy_rows'].shape == (B, L, 4) and len(seen) == 2 and seen[0].shape == (B, L) and torch.equal(seen[0], seen[1])
    # the per-residue pLDDT of the call: its mean over the diffused rows is the record's pLDDT
    dmf = dm.float()
    assert float(((seen[0] * dmf).sum(1) / dmf.sum() - last['pLDDT'][:, 0]).abs().max()) < 1e-4
    bits = lambda t: t.contiguous().view(torch.int64)
    direct = real(last['atom14_results'], last['seq'], plddt=seen[0], rows=True)
    assert torch.equal(bits(direct[0]), bits(last['accuracy'])) and torch.equal(bits(direct[1]), bits(last['accuracy_rows']))
    assert torch.equal(bits(real(last['atom14_relaxed'], last['seq'], plddt=seen[0])), bits(last['accuracy_relaxed']))
    design = sample_tiny(gpu_model, cfg, b, sid, mode='design', accuracy=sc)
    assert len(design) == 1 and 'accuracy_relaxed' not in design[0]
    assert torch.equal(bits(design[0]['accuracy']), bits(last['accuracy']))
    row, wild = last['accuracy'].cpu(), sc.wild().cpu()
    print('tiny workload, accuracy rows', row.tolist(), 'wild', wild.tolist())
    assert bool((row[:, 20] > 0).all()) and bool((row[:, 0] > 0).all()) and bool((row[:, 0] < 1).all()) and wild.shape == (1, NA)
    assert bool((row[:, 6] - last['pLDDT'][:, 0].cpu().double()).abs().max() < 1e-3) and bool((row[:, 7] >= 0).all())
    assert wild[0, :6].tolist() == [1.0] * 6 and wild[0, 11] < 1e-6 and bool(torch.isnan(wild[0, 6:8]).all())


@pytest.mark.parametrize('collective', [False, True])
def test_design_driver_writes_the_accuracy_table(tmp_path, monkeypatch, collective):
    """`abx_amd.design --accuracy`: <complex>_accuracy.tsv with the header, the wild line (every lDDT and fnat 1.0000) and one line per
    sample whose fields are the sampler's records at print precision; every other file of the run is byte-identical to the run without
    the flag.  collective = False: the shipped 6ct7 complex with --relax (the relaxed columns follow) and --accuracy_rows.
    collective = True: the 1-rank RCCL path on both shipped complexes, the table as further columns of the set-level gather."""
    from abx_amd import accuracy
    out, codes, N, seen = driver_pair(tmp_path, monkeypatch, 'accuracy', ['--accuracy'] + ([] if collective else ['--accuracy_rows']), collective,
                                        plain_extra=['--relax'], extra_files=[] if collective else [CODES[0] + '_accuracy_rows.npy'])
    NA, ND = len(accuracy.ACCURACY_COLUMNS), len(accuracy.DELTA_COLUMNS)
    for code in codes:
        lines = table_lines(out, code, 'accuracy')
        head = ['sample'] + list(accuracy.ACCURACY_COLUMNS)
        assert lines[0] == head + ([] if collective else [c + '_relaxed' for c in accuracy.ACCURACY_COLUMNS] + ['delta_' + c for c in accuracy.DELTA_COLUMNS])
        assert len(lines) == 1 + 1 + N and all(len(r) == len(lines[0]) for r in lines)
        runs = runs_of(seen, code, collective)
        wild = runs[0][0].wild().cpu()[0].tolist()
        assert lines[1][:1 + NA] == ['wild'] + accuracy.format_accuracy(wild)
        assert lines[1][1:7] == ['1.0000'] * 6 and lines[1][15] == '1.0000' and lines[1][12] == '0.000' and lines[1][7:9] == ['nan', 'nan']
        assert lines[1][13] == lines[1][14] == ('51' if code.startswith('6ct7') else '3')       # the native contacts of the crystal structure
        rows = torch.cat([tr[-1]['accuracy'] for _, tr in runs]).cpu().tolist()
        for i, r in enumerate(lines[2:]):
            assert r[0] == str(i) and r[1:1 + NA] == accuracy.format_accuracy(rows[i]), (code, i, r)
        if not collective:
            relaxed = runs[0][1][-1]['accuracy_relaxed'].cpu().tolist()
            assert lines[1][1 + NA:] == ['nan'] * (NA + ND)
            for i, r in enumerate(lines[2:]):
                assert r[1 + NA:1 + 2 * NA] == accuracy.format_accuracy(relaxed[i]) and r[1 + 2 * NA:] == accuracy.format_delta(relaxed[i], rows[i]), (code, i)
            per_res = np.load(os.path.join(out, code + '_accuracy_rows.npy'))
            assert per_res.shape == (N, 231, 4) and np.array_equal(per_res, runs[0][1][-1]['accuracy_rows'].cpu().numpy(), equal_nan=True)
