"""CPU-only checks of the shape-complementarity analysis (abx_shape_scores, abx_amd.shape): C layout of the descriptor, argument checks
without a GPU, the float64 host twin against the numbers a prototype of the definition printed for the two shipped complexes - the
list sizes as integers, the Sc columns to 1e-3 (the prototype did not fix the order of the median's inputs) -, the edge cases of the
trimming, the weight and the capacity, and the wiring of the design driver."""
import ctypes

import numpy as np
import pytest
import torch

import host_cases as HC
import relax_cases as RC
import shape_cases as SC


@pytest.fixture(scope='module')
def lib():
    return HC.load_lib()


@pytest.fixture(scope='module')
def shipped():
    """Host rows of the two shipped crystal complexes (P = 128, region = CDR-H3, trim 1.5), computed once."""
    from abx_amd import interface, shape
    out = {}
    for code in ('6ct7', '6qd7'):
        c = SC.complex_of(code)
        irow, pts = interface.interface_host(c['x'], c['mask'], c['aa'], c['Lab'], region=c['mov'], n_points=128)
        row, d = shape.shape_host(c['x'], c['mask'], c['aa'], c['Lab'], region=c['mov'], points=pts, details=True)
        out[code] = dict(c=c, pts=pts, row=row, d=d)
    return out


def test_shape_args_match_c_layout():
    from abx_amd import _lib, shape
    c_layout = HC.assert_c_layout({'AbxShapeArgs': _lib.AbxShapeArgs}, ['ABX_SHAPE_COLS'])
    assert c_layout['ABX_SHAPE_COLS'] == _lib.SHAPE_COLS == len(shape.SHAPE_COLUMNS) == 11
    assert [shape.SHAPE_COLUMNS.index(c) for c in shape.DELTA_COLUMNS] == [0, 1, 2, 3, 6, 7, 8]
    assert shape.COUNT_COLUMNS == shape.SHAPE_COLUMNS[6:]
    assert 'abx_shape_scores' in _lib.EXPORTED and 'abx_shape_scores_workspace_bytes' in _lib.EXPORTED


def test_argument_checks_without_gpu(lib):
    """Every malformed descriptor comes back negative before any launch, with the entry's name in the error string."""
    from abx_amd._lib import AbxShapeArgs
    PTR = 0x1000                                    # any non-null "device pointer": nothing is dereferenced

    def good():
        a = AbxShapeArgs()
        a.pred_atom14 = a.pred_seq = a.gt_atom14 = a.gt_exists = a.gt_seq = a.radius = a.sphere = a.points = a.out = PTR
        a.B, a.L, a.Lab, a.Lpred, a.P = 4, 40, 30, 30, 128
        a.pred_sb, a.pred_seq_sb, a.out_stride = 30 * 42, 30, 11
        a.probe, a.trim, a.weight, a.max_dots = 1.4, 1.5, 0.5, 8192
        return a

    def bad(a, ws=PTR):
        rc = lib.abx_shape_scores(ctypes.byref(a) if a is not None else None, ws, None)
        msg = lib.abx_last_error_string()
        assert rc < 0 and b'abx_shape_scores' in msg, (rc, msg)
        return msg

    bad(None)
    bad(AbxShapeArgs())
    bad(good(), ws=None)
    for field in ('pred_atom14', 'pred_seq', 'gt_atom14', 'gt_exists', 'gt_seq', 'radius', 'sphere', 'points', 'out'):
        a = good()
        setattr(a, field, None)
        bad(a)
    nan = float('nan')
    for field, v in (('B', 0), ('B', 65536), ('L', 0), ('Lab', 41), ('Lab', 0), ('Lpred', 29), ('out_stride', 10), ('P', 0), ('P', 1025),
                     ('probe', -0.1), ('probe', nan), ('trim', -1.0), ('trim', nan), ('weight', -0.5), ('weight', nan), ('max_dots', 0),
                     ('max_dots', (1 << 20) + 1), ('j_chunk', -1), ('j_chunk', 1025)):
        a = good()
        setattr(a, field, v)
        bad(a)
    a = good()                                      # more atoms than the LDS of a CU holds
    a.L, a.Lab, a.Lpred = 600, 300, 300
    assert b'L <= 541' in bad(a)
    per = (64 + 504 * 352 + 144 * 8192 + 15) // 16 * 16
    assert lib.abx_shape_scores_workspace_bytes(100, 352, 128, 8192) == 100 * per
    assert lib.abx_shape_scores_workspace_bytes(1, 231, 128, 64) == (64 + 504 * 231 + 144 * 64 + 15) // 16 * 16
    assert lib.abx_shape_scores_workspace_bytes(0, 352, 128, 8192) == 0 and lib.abx_shape_scores_workspace_bytes(1, 352, 128, 0) == 0


def test_median_rule():
    from abx_amd.shape import median
    assert median([]) == 0.0 and median([3.0]) == 3.0 and median([4.0, 1.0]) == 2.5 and median([5.0, 1.0, 3.0]) == 3.0
    assert median([4.0, 1.0, 3.0, 2.0]) == 2.5 and median([-1.0, -1.0, 7.0, 8.0, 9.0]) == 7.0


@pytest.mark.parametrize('code', ['6ct7', '6qd7'])
def test_shipped_complexes_give_the_prototype_numbers(shipped, code):
    """The list sizes are integers of the definition: equal.  The buried dots per side are the interface analysis' buried points."""
    from abx_amd import shape
    s = shipped[code]
    row, d, c, pts = s['row'], s['d'], s['c'], s['pts']
    proto = SC.PROTOTYPE[code, 128]
    got = dict(zip(shape.SHAPE_COLUMNS, row.tolist()))
    print(code, got, d['n_buried'], d['n_open'])
    assert d['bad'] is None and d['n_buried'] == proto['buried'] and d['n_kept'] == proto['kept'] and int(d['region'].sum()) == proto['region']
    if proto['open']:
        assert d['n_open'] == proto['open']
    side = (np.arange(c['aa'].shape[0]) >= c['Lab'])[:, None]
    buried = (pts[..., 0] - pts[..., 1]).astype(np.int64)
    assert d['n_buried'] == (int(buried[~side[:, 0]].sum()), int(buried[side[:, 0]].sum()))
    assert np.abs(row[:4] - np.array(proto['sc'])).max() <= 1e-3
    assert row[6:].tolist() == [proto['kept'][0], proto['kept'][1], proto['region'], proto['buried'][0] - proto['kept'][0], proto['buried'][1] - proto['kept'][1]]
    assert row[0] == (row[1] + row[2]) * 0.5 and row[1] == shape.median(d['S'][0]) and row[4] == np.sqrt(shape.median(d['d2'][0]))
    assert len(d['S'][0]) == (row[6] if row[7] else 0) and row[3] == shape.median(d['S'][0][d['region']] if row[7] else [])
    # the points are computed by interface_host when none are given
    assert shape.shape_host(c['x'], c['mask'], c['aa'], c['Lab'], region=c['mov']).tolist() == row.tolist()


def test_6qd7_is_the_edge_case(shipped):
    """68 / 74 buried dots of which the default trim leaves 8 / 0: every Sc column is 0 and the counts say why; trim 0 gives about 0.172."""
    from abx_amd import shape
    s = shipped['6qd7']
    c = s['c']
    assert s['row'].tolist() == [0.0] * 6 + [8.0, 0.0, 0.0, 60.0, 74.0]
    row, d = shape.shape_host(c['x'], c['mask'], c['aa'], c['Lab'], region=c['mov'], points=s['pts'], trim=0.0, details=True)
    assert abs(row[0] - 0.172) <= 1e-3 and row[6:].tolist() == [68.0, 74.0, 0.0, 0.0, 0.0] and d['n_kept'] == (68, 74)


@pytest.mark.parametrize('seed', RC.SEEDS)
def test_perturbed_h3_lowers_its_own_value(seed):
    """The seeded perturbations of CDR-H3 of 6ct7 leave the whole interface near the crystal's 0.549 and drop the CDR-H3 dots' value."""
    from abx_amd import shape
    c = SC.complex_of('6ct7')
    row = shape.shape_host(RC.perturb(c, seed), c['mask'], c['aa'], c['Lab'], region=c['mov'])
    print(seed, row.tolist())
    assert abs(row[0] - SC.PERTURBED[seed][0]) <= 1e-3 and abs(row[3] - SC.PERTURBED[seed][1]) <= 1e-3


@pytest.mark.parametrize('P', [64, 256, 512])
def test_sc_rises_with_the_dot_density(P):
    from abx_amd import shape
    c = SC.complex_of('6ct7')
    row, d = shape.shape_host(c['x'], c['mask'], c['aa'], c['Lab'], region=c['mov'], n_points=P, details=True)
    print(P, row.tolist(), d['n_buried'], d['n_open'])
    assert abs(row[0] - SC.DENSITY[P]) <= 1e-3
    if P == 512:
        assert (d['n_buried'], d['n_open']) == ((2824, 3517), (1743, 1784)) and np.abs(row[1:3] - np.array(SC.DENSITY_512)).max() <= 1e-3


def test_weight_trim_and_capacity_edge_cases(shipped):
    from abx_amd import shape
    s = shipped['6ct7']
    c, pts, base = s['c'], s['pts'], s['d']
    args = (c['x'], c['mask'], c['aa'], c['Lab'])
    # weight 0: the plain median of -n.n; the match itself does not depend on the weight
    row, d = shape.shape_host(*args, region=c['mov'], points=pts, weight=0.0, details=True)
    for k in range(2):
        assert np.array_equal(d['d2'][k], base['d2'][k]) and np.abs(d['S'][k]).max() <= 1.0 + 1e-15
        assert np.array_equal(d['S'][k] * np.exp(-(0.5 * d['d2'][k])), base['S'][k])
    assert row[1] == shape.median(d['S'][0]) and row[1] > s['row'][1] and row[4:].tolist() == s['row'][4:].tolist()
    # trim 0 keeps everything, trim 1e4 nothing (both sides have open dots)
    row = shape.shape_host(*args, region=c['mov'], points=pts, trim=0.0)
    assert row[6:].tolist() == [701.0, 881.0, 99.0, 0.0, 0.0] and 0.3 < row[0] < s['row'][0]
    row = shape.shape_host(*args, region=c['mov'], points=pts, trim=1e4)
    assert row.tolist() == [0.0] * 9 + [701.0, 881.0]
    # without a region no dot is a region dot
    row = shape.shape_host(*args, points=pts)
    assert row[3] == 0.0 and row[8] == 0.0 and row[:3].tolist() == s['row'][:3].tolist()
    # capacity: the largest list has 881 dots
    assert shape.shape_host(*args, region=c['mov'], points=pts, max_dots=881).tolist() == s['row'].tolist()
    row, d = shape.shape_host(*args, region=c['mov'], points=pts, max_dots=880, details=True)
    assert row.tolist() == [-1.0] * 11 and d['bad'] == 'max_dots'
    # points of another structure, and points that cannot be
    other = shape.shape_host(RC.perturb(c, 6), c['mask'], c['aa'], c['Lab'], region=c['mov'], points=pts, details=True)
    assert other[0].tolist() == [-1.0] * 11 and other[1]['bad'] == 'points'
    broken = pts.copy()
    broken[5, 1, 0] = 129
    assert shape.shape_host(*args, region=c['mov'], points=broken).tolist() == [-1.0] * 11
    # no interface: the antigen 100 A away
    far = SC.antigen_moved(c)
    assert shape.shape_host(far, c['mask'], c['aa'], c['Lab'], region=c['mov']).tolist() == [0.0] * 11
    small, d = shape.shape_host(SC.antibody_moved(c, SC.SMALL_SHIFT), c['mask'], c['aa'], c['Lab'], region=c['mov'], trim=0.0, max_dots=64, details=True)
    assert (d['n_buried'], d['n_open'], d['n_kept']) == ((8, 8), (51, 64), (8, 8)) and small[0] > 0


def test_scorer_rejects_bad_options():
    from abx_amd import shape
    for kw in (dict(trim=-1.0), dict(weight=-0.1), dict(max_dots=0)):
        with pytest.raises(ValueError, match='shape: needs trim >= 0'):
            shape.ShapeScorer({}, **kw)


PARSER = None


def parser():
    global PARSER
    if PARSER is None:
        from abx_amd import design
        PARSER = design.build_parser()
    return PARSER


def test_driver_declares_a_later_analysis():
    """ANALYSES keeps its order; --shape is walked after the first eight."""
    from abx_amd import analyses, shape
    assert [an.flag for an in analyses.ANALYSES] == ['score', 'relax', 'interface', 'confidence', 'accuracy', 'polar', 'ensemble', 'developability', 'shape', 'patches', 'torsions', 'secondary']
    assert analyses.SHAPE.kw == 'shape' and analyses.SHAPE.extra is None
    a = parser().parse_args([])
    assert a.shape is False and (a.shape_trim, a.shape_weight, a.shape_max_dots) == (1.5, 0.5, 8192)
    assert analyses.check_options(a, False) == []
    every = ['--' + an.flag for an in analyses.ANALYSES[:8]]
    a = parser().parse_args(['--shape'] + every)
    assert [an.flag for an in analyses.check_options(a, True)] == [an.flag for an in analyses.ANALYSES[:8]] + ['shape']
    a = parser().parse_args(['--shape', '--shape_trim', '0', '--shape_weight', '0', '--shape_max_dots', '1'])
    assert [an.flag for an in analyses.check_options(a, False)] == ['shape']
    NS = len(shape.SHAPE_COLUMNS)
    shapes = lambda a: {f.name: (f.dtype, f.shape, f.rows) for f in analyses.fields_of(analyses.check_options(a, False), a)}
    assert shapes(a) == {'seq': (torch.int64, ('Lab',), True), 'pLDDT': (torch.float32, ('Lab',), False), 'shape': (torch.float64, (2 * NS,), True)}
    a = parser().parse_args(['--shape', '--relax'])
    assert shapes(a)['shape'] == (torch.float64, (3 * NS,), True)


@pytest.mark.parametrize('argv, text', [
    (['--shape', '--shape_trim', '-0.5'], '--shape_trim must be >= 0, --shape_weight >= 0, --shape_max_dots >= 1'),
    (['--shape', '--shape_weight', '-1'], '--shape_trim must be >= 0, --shape_weight >= 0, --shape_max_dots >= 1'),
    (['--shape', '--shape_max_dots', '0'], '--shape_trim must be >= 0, --shape_weight >= 0, --shape_max_dots >= 1'),
    (['--shape', '--interface_points', '0'], '--interface_points must be in 1..1024, --interface_probe >= 0'),
    (['--shape', '--interface_points', '1025'], '--interface_points must be in 1..1024, --interface_probe >= 0'),
    (['--shape', '--interface_probe', '-1'], '--interface_points must be in 1..1024, --interface_probe >= 0'),
])
def test_option_checks_exit_by_name(argv, text):
    from abx_amd import analyses
    with pytest.raises(SystemExit) as e:
        analyses.check_options(parser().parse_args(argv), False)
    assert e.value.code == text


class Wild:
    """A scorer as analyses.collect sees one: a wild row per complex and the buffer of point counts."""

    def __init__(self, columns, seen):
        self.columns, self.seen = columns, seen

    def new_points(self, B):
        return torch.empty(B, 9, 14, 2, dtype=torch.int32)

    def wild(self, points=None):
        self.seen.append(points)
        return torch.full((1, len(self.columns)), 0.5, dtype=torch.float64)


@pytest.mark.parametrize('with_all', [False, True])
def test_zero_row_block_matches_the_filled_block(with_all):
    from abx_amd import accuracy, analyses, confidence, developability as dv, interface, metrics, polar, relax, shape
    L, Lab, n = 9, 7, 2
    before = analyses.ANALYSES[:8]
    others = [an.flag for an in before] if with_all else []
    flags = others + ['shape'] + [an.extra for an in before if an.extra and with_all]
    a = parser().parse_args(['--' + f for f in flags])
    active = analyses.check_options(a, set_level=False)
    assert [an.flag for an in active] == others + ['shape']
    g = torch.Generator().manual_seed(3)
    table = lambda cols: (torch.rand(n, len(cols), generator=g, dtype=torch.float64) * 50).round(decimals=3)
    rec = {'seq': torch.randint(0, 20, (n, Lab), generator=g), 'pLDDT': torch.full((n, Lab), 70.0), 'atom14_results': torch.randn(n, Lab, 14, 3, generator=g),
           'time': 0.01, 'scores': table(metrics.SCORE_COLUMNS), 'relax': table(relax.RELAX_COLUMNS), 'scores_relaxed': table(metrics.SCORE_COLUMNS),
           'confidence_wild': table(confidence.CONFIDENCE_COLUMNS), 'confidence_planes': (torch.rand(n, L, L, generator=g), None),
           'accuracy_rows': torch.rand(n, L, 4, generator=g, dtype=torch.float64), 'polar_rows': torch.zeros(n, L, 4, dtype=torch.int32),
           'developability_rows': torch.rand(n, L, 4, generator=g, dtype=torch.float64)}
    for mod in (interface, confidence, accuracy, polar, dv, shape):
        kind = mod.__name__.rsplit('.', 1)[1]
        rec[kind], rec[kind + '_relaxed'] = table(getattr(mod, kind.upper() + '_COLUMNS')), table(getattr(mod, kind.upper() + '_COLUMNS'))
    seen = []
    columns = {'interface': interface.INTERFACE_COLUMNS, 'accuracy': accuracy.ACCURACY_COLUMNS, 'polar': polar.POLAR_COLUMNS,
               'developability': dv.DEVELOPABILITY_COLUMNS, 'shape': shape.SHAPE_COLUMNS}
    scorers = {f: Wild(c, seen) for f, c in columns.items() if f in flags}
    filled = analyses.collect(active, a, [rec], scorers)
    zero = analyses.zero_rows(active, a, L, Lab, 'cpu')
    assert list(filled) == list(zero) == [f.name for f in analyses.fields_of(active, a)] and list(zero)[-1] == 'shape'
    for k in filled:
        assert filled[k].dtype == zero[k].dtype and filled[k].shape[1:] == zero[k].shape[1:] and filled[k].shape[0] == n and zero[k].shape[0] == 0, k
    NS = len(shape.SHAPE_COLUMNS)
    assert filled['shape'].shape == (n, (3 if with_all else 2) * NS) and bool((filled['shape'][:, -NS:] == 0.5).all())
    assert torch.equal(filled['shape'][:, :NS], rec['shape'])
    if with_all:                    # one buffer of point counts serves the four wild rows; accuracy's takes none
        assert len(seen) == 5 and all(seen[k] is seen[0] for k in (2, 3, 4)) and seen[0].shape == (1, 9, 14, 2) and seen[1] is None
    else:
        assert seen == [None]


def test_table_format(tmp_path):
    """The writer round-trips a wild line and deltas: four decimals for Sc, three for the gaps, integers for the counts."""
    from abx_amd import design, shape
    NS = len(shape.SHAPE_COLUMNS)
    wild = [0.54921, 0.57414, 0.52441, 0.57252, 0.70147, 0.81700, 347, 532, 82, 354, 349]
    d0 = [0.5, 0.6, 0.4, 0.33852, 0.8153, 0.8558, 333, 489, 61, 365, 380]
    assert shape.format_shape(wild) == ['0.5492', '0.5741', '0.5244', '0.5725', '0.701', '0.817', '347', '532', '82', '354', '349']
    assert shape.format_delta(d0, wild) == ['-0.0492', '+0.0259', '-0.1244', '-0.2340', '-14', '-43', '-21']
    path = design._write_shape(str(tmp_path), '6ct7_H_L_S', wild, [(0, d0 + wild), (1, wild + wild)], False)
    lines = [ln.split('\t') for ln in open(path).read().splitlines()]
    assert path.endswith('6ct7_H_L_S_shape.tsv') and len(lines) == 4
    assert lines[0] == ['sample'] + list(shape.SHAPE_COLUMNS) + ['delta_' + c for c in shape.DELTA_COLUMNS]
    assert lines[1] == ['wild'] + shape.format_shape(wild) + ['+0.0000'] * 4 + ['+0'] * 3
    assert lines[2] == ['0'] + shape.format_shape(d0) + shape.format_delta(d0, wild) and lines[3][1 + NS:] == lines[1][1 + NS:]
    assert [float(v) for v in lines[2][1:1 + NS]] == pytest.approx(d0, abs=5e-4)
    path = design._write_shape(str(tmp_path), 'x_H_L_A', wild, [(5, d0 + wild + wild)], True)
    lines = [ln.split('\t') for ln in open(path).read().splitlines()]
    assert lines[0][1 + NS + 7:] == [c + '_relaxed' for c in shape.SHAPE_COLUMNS] and lines[1][1 + NS + 7:] == ['nan'] * NS
    assert lines[2] == ['5'] + shape.format_shape(d0) + shape.format_delta(d0, wild) + shape.format_shape(wild)


def test_a_row_of_minus_one_ends_the_run_by_name(tmp_path):
    from abx_amd import design
    wild = [0.5, 0.5, 0.5, 0.5, 0.7, 0.8, 347, 532, 82, 354, 349]
    minus = [-1.0] * 11
    for rows, relaxed in (([(0, minus + wild)], False), ([(0, wild + minus + wild)], True)):
        with pytest.raises(SystemExit) as e:
            design._write_shape(str(tmp_path), 'c', wild, rows, relaxed)
        assert '--shape_max_dots' in str(e.value.code)
    with pytest.raises(SystemExit):
        design._write_shape(str(tmp_path), 'c', minus, [(0, minus + minus)], False)
    negative_sc = [-0.2, -0.1, -0.3, -0.4, 0.7, 0.8, 5, 6, 1, 0, 0]            # anti-complementary surfaces are no error
    assert design._write_shape(str(tmp_path), 'c', wild, [(0, negative_sc + wild)], False).endswith('c_shape.tsv')


def test_sampler_signature_defaults_to_no_shape():
    import inspect
    from abx_amd import sampler
    assert inspect.signature(sampler.sample_fn).parameters['shape'].default is None
