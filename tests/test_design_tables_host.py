"""Host checks of the design driver's table of analyses (abx_amd.analyses): the layout of the set-level rows, the zero-row blocks, the one
write path behind both schedules and the option checks.  No device: the scorers are stand-ins, the ensemble analysis its float64 twin."""
import itertools
import os

import numpy as np
import pytest
import torch

from abx_amd import accuracy, analyses, confidence, design, ensemble, interface, polar, sampler

FLAGS = [an.flag for an in analyses.ANALYSES[:7]]
L, LAB, N = 9, (5, 7), 3


PARSER = design.build_parser()


def parse(flags, *more):
    return PARSER.parse_args(['--' + f for f in flags] + list(more))


def fabricate(fields, n, Lab, base=0):
    """{field: (n, ...)} with a value of its own in every element: field index * 1000 + column, + 100000 per sample."""
    out = {}
    for k, f in enumerate(fields):
        shape = analyses.block_shape(f, L, Lab)
        cols = int(np.prod(shape))
        v = k * 1000 + torch.arange(cols, dtype=torch.float64)[None] + 100000.0 * (base + torch.arange(n, dtype=torch.float64))[:, None]
        out[f.name] = v.reshape(n, *shape).to(f.dtype)
    return out


def test_layout_round_trip_for_every_subset_of_the_analyses():
    assert FLAGS == ['score', 'relax', 'interface', 'confidence', 'accuracy', 'polar', 'ensemble']
    for r in range(len(FLAGS) + 1):
        for flags in itertools.combinations(FLAGS, r):
            for n_rec in (0, 3):
                a = parse(flags, *(['--mode', 'trajectory', '--num_t', '3'] if n_rec else []))
                fields = analyses.fields_of(analyses.check_options(a, set_level=True), a)
                layout = analyses.RowLayout(fields, max(LAB))
                spans = sorted(layout.spans.values())
                assert spans[0][0] == 4 and all(s[1] == t[0] for s, t in zip(spans, spans[1:])) and spans[-1][1] == layout.WIDTH, (flags, spans)
                assert layout.WIDTH == 4 + sum(e - s for s, e in spans) and set(layout.spans) == {f.name for f in fields if f.rows}
                assert ('traj_scores' in layout.spans) == ('score' in flags and n_rec == 3) and 'pLDDT' not in layout.spans
                # two jobs, the rows of each arriving out of sample order through the 1-rank gather
                local = {ji: fabricate(fields, N, Lab, base=10 * ji) for ji, Lab in enumerate(LAB)}
                order = [2, 0, 1]
                table = torch.cat([layout.pack(ji, order, {k: v[order] for k, v in local[ji].items()}) for ji in (1, 0)])
                assert table.shape == (2 * N, layout.WIDTH) and table.dtype == torch.float64
                full = sampler.gather_rows(table, [2 * N], 0, 1)
                for ji, Lab in enumerate(LAB):
                    mine = full[full[:, 0] == ji]
                    ids, F = layout.unpack(mine)
                    assert ids == [0, 1, 2] and set(F) == set(layout.spans) | {'mean_pLDDT'}
                    assert torch.equal(F['mean_pLDDT'], local[ji]['pLDDT'].float().mean(1).double())
                    for f in layout.fields:
                        assert F[f.name].dtype == f.dtype and torch.equal(F[f.name], local[ji][f.name]), (flags, n_rec, ji, f.name)
                        s, e = layout.spans[f.name]
                        used = int(np.prod(analyses.block_shape(f, L, Lab)))
                        assert not mine[:, s + used:e].any(), 'the columns beyond the job\'s own Lab stay zero'


class Wild:
    """A scorer as analyses.collect sees one: a wild row per complex, and for polar the buffer of point counts."""

    def __init__(self, columns, seen):
        self.columns, self.seen = columns, seen

    def new_points(self, B):
        return torch.empty(B, L, 14, 2, dtype=torch.int32)

    def wild(self, points=None):
        self.seen.append(points)
        return torch.full((1, len(self.columns)), 0.5, dtype=torch.float64)


def record(a, n, Lab, seed=0):
    """A last record as sampler.sample_fn leaves it with every scorer on, values from a seeded generator."""
    g = torch.Generator().manual_seed(seed)
    table = lambda cols: (torch.rand(n, len(cols), generator=g, dtype=torch.float64) * 50).round(decimals=3)
    from abx_amd import metrics, relax
    rec = {'seq': torch.randint(0, 20, (n, Lab), generator=g), 'pLDDT': (64.5 + 0.25 * torch.arange(n, dtype=torch.float32))[:, None].expand(n, Lab),
           'atom14_results': torch.randn(n, Lab, 14, 3, generator=g), 'time': 0.01, 'scores': table(metrics.SCORE_COLUMNS),
           'relax': table(relax.RELAX_COLUMNS), 'scores_relaxed': table(metrics.SCORE_COLUMNS),
           'confidence_wild': table(confidence.CONFIDENCE_COLUMNS), 'confidence_planes': (torch.rand(n, L, L, generator=g), None),
           'accuracy_rows': torch.rand(n, L, 4, generator=g, dtype=torch.float64), 'polar_rows': torch.randint(0, 9, (n, L, 4), generator=g, dtype=torch.int32)}
    for mod in (interface, confidence, accuracy, polar):
        kind = mod.__name__.rsplit('.', 1)[1]
        rec[kind], rec[kind + '_relaxed'] = table(getattr(mod, kind.upper() + '_COLUMNS')), table(getattr(mod, kind.upper() + '_COLUMNS'))
    return rec


def stand_ins(seen, flags=FLAGS):
    """The scorers of a batch that the collecting code calls, by flag."""
    columns = {'interface': interface.INTERFACE_COLUMNS, 'accuracy': accuracy.ACCURACY_COLUMNS, 'polar': polar.POLAR_COLUMNS}
    return {f: Wild(c, seen) for f, c in columns.items() if f in flags}


@pytest.mark.parametrize('flags', [[f] for f in FLAGS] + [FLAGS], ids=lambda f: '+'.join(f))
def test_zero_row_block_matches_the_filled_block(flags):
    extras = [an.extra for an in analyses.ANALYSES[:7] if an.flag in flags and an.extra]
    a = parse(flags + extras)
    active = analyses.check_options(a, set_level=False)
    assert [an.flag for an in active] == flags
    seen = []
    filled = analyses.collect(active, a, [record(a, 2, 7)], stand_ins(seen, flags))
    zero = analyses.zero_rows(active, a, L, 7, 'cpu')
    assert list(filled) == list(zero) == [f.name for f in analyses.fields_of(active, a)]
    assert {'seq', 'pLDDT'} < set(zero) and all(('confidence_contacts', 'accuracy_rows', 'polar_rows')[k] in zero
                                                 for k, f in enumerate(('confidence', 'accuracy', 'polar')) if f in flags)
    for k in filled:
        assert filled[k].dtype == zero[k].dtype and filled[k].shape[1:] == zero[k].shape[1:], k
        assert filled[k].shape[0] == 2 and zero[k].shape[0] == 0
    if flags == FLAGS:              # one buffer of point counts serves both wild rows; accuracy's takes none
        assert len(seen) == 3 and seen[0] is seen[2] and seen[0].shape == (1, L, 14, 2) and seen[1] is None
    elif flags in (['interface'], ['polar']):
        assert seen == [None]


class HostAnalyzer:
    """ensemble.EnsembleAnalyzer's float64 twin behind the same three attributes and analyze()."""

    def __init__(self, Lab):
        self.Lab, self.n_region = Lab, 3
        self.region = torch.zeros(Lab, dtype=torch.uint8)
        self.region[1:4] = 1

    def analyze(self, x, seq):
        return {k: torch.as_tensor(v) for k, v in ensemble.ensemble_host(x, seq, self.region, cutoff=2.0).items()}


def test_both_schedules_write_the_same_bytes(tmp_path):
    """Fabricated fields of two complexes with every analysis on: the tables written from sampler.gather_results' form and from the
    unpacked rows of sampler.gather_rows are the same bytes, and their lines are what the modules' own format functions give."""
    a = parse(FLAGS, '--ensemble_matrix')
    active = analyses.check_options(a, set_level=True)
    layout = analyses.RowLayout(analyses.fields_of(active, a), max(LAB))
    analyzers = {Lab: HostAnalyzer(Lab) for Lab in LAB}
    blocks, rows = {}, []
    os.makedirs(tmp_path / 'one')
    os.makedirs(tmp_path / 'set')
    for ji, Lab in enumerate(LAB):          # every job in two blocks, as two units of a plan: samples (0, 1) and (2)
        blocks[ji] = [analyses.collect(active, a, [record(a, len(ids), Lab, seed=10 * ji + ids[0])], stand_ins([])) for ids in ([0, 1], [2])]
        rows += [layout.pack(ji, ids, blk) for ids, blk in zip(([0, 1], [2]), blocks[ji])]
    full = sampler.gather_rows(torch.cat(rows[::-1]), [2 * N], 0, 1)
    for ji, Lab in enumerate(LAB):
        res = {k: torch.cat([blk[k] for blk in blocks[ji]]) for k in blocks[ji][0]}
        res['mean_pLDDT'] = [float(res['pLDDT'][i].float().mean()) for i in range(N)]
        one = analyses.write_job(active, a, str(tmp_path / 'one'), f'c{ji}_H_L_A', list(range(N)), res, lambda an: analyzers[Lab])
        two = analyses.write_job(active, a, str(tmp_path / 'set'), f'c{ji}_H_L_A', *layout.unpack(full[full[:, 0] == ji]), lambda an: analyzers[Lab])
        ends = ['designs.tsv', 'relax.tsv', 'interface.tsv', 'confidence.tsv', 'accuracy.tsv', 'polar.tsv', 'ensemble.tsv', 'ensemble_rmsd.npy']
        assert [os.path.basename(f) for f in one] == [os.path.basename(f) for f in two] == [f'c{ji}_H_L_A_{e}' for e in ends]
        for f, g in zip(one, two):
            assert open(f, 'rb').read() == open(g, 'rb').read(), f
        # the lines against the format functions: header, wild line and sample 1 (the second row of the first block)
        for mod, own_wild in ((interface, False), (polar, False), (confidence, True)):
            kind = mod.__name__.rsplit('.', 1)[1]
            cols, fmt = getattr(mod, kind.upper() + '_COLUMNS'), getattr(mod, 'format_' + kind)
            lines = [ln.split('\t') for ln in open(tmp_path / 'set' / f'c{ji}_H_L_A_{kind}.tsv').read().splitlines()]
            v = res[kind][1].tolist()
            C = len(cols)
            assert len(v) == 3 * C and len(lines) == 2 + N
            assert lines[0] == ['sample'] + list(cols) + ['delta_' + c for c in mod.DELTA_COLUMNS] + [c + '_relaxed' for c in cols]
            wild = [sum(r[2 * C + k] for r in res[kind].tolist()) / N for k in range(C)] if own_wild else [0.5] * C
            assert lines[1] == ['wild'] + fmt(wild) + mod.format_delta(wild, wild) + ['nan'] * C
            assert lines[3] == ['1'] + fmt(v[:C]) + mod.format_delta(v[:C], v[2 * C:]) + fmt(v[C:2 * C])
        lines = [ln.split('\t') for ln in open(tmp_path / 'set' / f'c{ji}_H_L_A_accuracy.tsv').read().splitlines()]
        v, C = res['accuracy'][1].tolist(), len(accuracy.ACCURACY_COLUMNS)
        assert lines[0] == ['sample'] + list(accuracy.ACCURACY_COLUMNS) + [c + '_relaxed' for c in accuracy.ACCURACY_COLUMNS] + \
            ['delta_' + c for c in accuracy.DELTA_COLUMNS]
        assert lines[1] == ['wild'] + accuracy.format_accuracy([0.5] * C) + ['nan'] * (C + len(accuracy.DELTA_COLUMNS))
        assert lines[3] == ['1'] + accuracy.format_accuracy(v[:C]) + accuracy.format_accuracy(v[C:2 * C]) + accuracy.format_delta(v[C:2 * C], v[:C])
        planes = np.load(tmp_path / 'set' / f'c{ji}_H_L_A_ensemble_rmsd.npy')
        assert planes.shape == (3, N, N) and (planes[1][~np.eye(N, dtype=bool)] > 0).all()


@pytest.mark.parametrize('argv, set_level, text', [
    (['--polar_rows'], False, '--polar_rows needs --polar'),
    (['--accuracy', '--accuracy_rows'], True,
     '--accuracy_rows needs the sample-sharded schedule (--shard_samples): a set-level run gathers one table only'),
    (['--polar', '--interface_points', '0'], False, '--interface_points must be in 1..1024, --interface_probe >= 0'),
    (['--ensemble', '--num_samples', '0'], False, '--ensemble compares 1..1024 samples of a complex, --ensemble_cutoff must be >= 0'),
    (['--interface', '--interface_points', '0'], False, '--interface_points must be in 1..1024, --interface_probe >= 0, --interface_cutoff > 0'),
    (['--confidence_planes'], False, '--confidence_planes needs --confidence'),
])
def test_option_checks_keep_their_texts(argv, set_level, text):
    with pytest.raises(SystemExit) as e:
        analyses.check_options(PARSER.parse_args(argv), set_level)
    assert e.value.code == text
    assert [an.flag for an in analyses.check_options(parse(['accuracy', 'accuracy_rows']), set_level=False)] == ['accuracy']
