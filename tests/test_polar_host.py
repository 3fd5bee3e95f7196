"""CPU-only checks of the polar-contact analysis (abx_polar_scores, abx_amd.polar): C layout of the descriptor, argument checks without a
GPU, the polar table against a literal expectation, exact hand-built cases of the float64 host twin, the two shipped complexes against
recorded numbers and against an independent restatement of the rule, and the formats of the design driver."""
import ctypes
import os

import numpy as np
import pytest

import host_cases as HC
import polar_cases as PC
import relax_cases as RC



@pytest.fixture(scope='module')
def lib():
    return HC.load_lib()


def test_polar_args_match_c_layout():
    """sizeof / offsetof of AbxPolarArgs as gcc lays it out, and the ABX_POLAR_* constants against the Python side."""
    from abx_amd import _lib, polar
    st = _lib.AbxPolarArgs
    BITS = ['ABX_POLAR_DONOR', 'ABX_POLAR_ACCEPTOR', 'ABX_POLAR_CATION', 'ABX_POLAR_ANION', 'ABX_POLAR_ELEMENT']
    c_layout = HC.assert_c_layout({'AbxPolarArgs': st}, ['ABX_POLAR_COLS'] + BITS)
    assert c_layout['ABX_POLAR_COLS'] == _lib.POLAR_COLS == len(polar.POLAR_COLUMNS) == 14
    bits = [c_layout[m] for m in BITS]
    assert bits == [_lib.POLAR_DONOR, _lib.POLAR_ACCEPTOR, _lib.POLAR_CATION, _lib.POLAR_ANION, _lib.POLAR_ELEMENT] == \
        [polar.DONOR, polar.ACCEPTOR, polar.CATION, polar.ANION, polar.ELEMENT] == [1, 2, 4, 8, 16]
    assert polar.COUNT_COLUMNS == polar.POLAR_COLUMNS[:10] + polar.POLAR_COLUMNS[12:]
    assert [polar.POLAR_COLUMNS.index(c) for c in polar.DELTA_COLUMNS] == [0, 2, 3, 4, 8, 9, 10, 11]


def test_polar_argument_checks_without_gpu(lib):
    """Every malformed descriptor comes back negative before any launch, with the entry's name in the error string."""
    from abx_amd import polar
    from abx_amd._lib import AbxPolarArgs
    P = 0x1000                                      # any non-null "device pointer": nothing is dereferenced

    def good():
        a = AbxPolarArgs()
        a.pred_atom14 = a.pred_seq = a.gt_atom14 = a.gt_exists = a.gt_seq = a.radius = a.table = a.out = a.points = P
        a.B, a.L, a.Lab, a.Lpred, a.P = 4, 40, 30, 30, 128
        a.pred_sb, a.pred_seq_sb, a.out_stride = 30 * 42, 30, 14
        a.probe, a.hb_min, a.hb_max, a.hb_angle, a.hb_cos2, a.salt = 1.4, 2.0, 3.5, 120.0, polar.cos2_of(120.0), 4.0
        return a

    def bad(a):
        rc = lib.abx_polar_scores(ctypes.byref(a) if a is not None else None, None, None)
        msg = lib.abx_last_error_string()
        assert rc < 0 and b'abx_polar_scores' in msg, (rc, msg)

    assert lib.abx_polar_scores_workspace_bytes(100, 352) == 0
    bad(None)
    bad(AbxPolarArgs())
    for field in ('pred_atom14', 'pred_seq', 'gt_atom14', 'gt_exists', 'gt_seq', 'radius', 'table', 'out'):
        a = good()
        setattr(a, field, None)
        bad(a)
    nan = float('nan')
    for field, v in (('B', 0), ('B', -3), ('B', 65536), ('L', 0), ('L', -1), ('Lab', 41), ('Lab', 0), ('Lpred', 29), ('Lpred', 41), ('out_stride', 13),
                     ('P', 0), ('P', 1025), ('probe', -0.1), ('probe', nan), ('hb_min', 3.6), ('hb_min', -1.0), ('hb_min', nan), ('hb_max', 1.9),
                     ('hb_max', nan), ('hb_max', float('inf')), ('hb_angle', 89.9), ('hb_angle', 180.0), ('hb_angle', 60.0), ('hb_angle', nan),
                     ('hb_cos2', 0.5), ('hb_cos2', nan), ('hb_cos2', -0.25), ('salt', -1.0), ('salt', nan)):
        a = good()
        setattr(a, field, v)
        bad(a)
    a = good()                                      # 80 degrees with ITS squared cosine: the angle is outside the range
    a.hb_angle, a.hb_cos2 = 80.0, np.cos(np.radians(80.0)) ** 2
    bad(a)
    a = good()                                      # a table beyond the LDS of a CU
    a.L, a.Lab, a.Lpred = 757, 300, 300
    bad(a)
    assert lib.abx_polar_scores_lds_bytes(756) == 216 * 756 + 512 <= 160 * 1024 < lib.abx_polar_scores_lds_bytes(757)
    assert polar.cos2_of(90.0) == 0.0 and abs(polar.cos2_of(120.0) - 0.25) < 1e-15


def test_polar_table_against_a_literal_expectation():
    """Donors, acceptors, cations and anions of every residue type and every antecedent slot; Pro N is no donor, His no cation, X empty;
    the element bit marks every N* and O* atom (Pro N included) and nothing else."""
    from abx_amd import polar, residue_constants as rc
    t = polar.polar_table()
    assert t.shape == (21, 14) and t.dtype == np.int32 and not t[20].any()
    assert list(rc.restypes) == list(PC.RESTYPES)
    for i, r in enumerate(PC.RESTYPES):
        counts = tuple(int(((t[i] & bit) != 0).sum()) for bit in (polar.DONOR, polar.ACCEPTOR, polar.CATION, polar.ANION))
        assert counts == PC.ROLE_COUNTS[r], (r, counts)
        want = dict(PC.SIDE_ANTECEDENTS.get(r, {}))
        want[3] = 2
        if r != 'P':
            want[0] = 1
        got = {s: int((t[i, s] >> 8) & 15) for s in range(14) if t[i, s] & (polar.DONOR | polar.ACCEPTOR)}
        assert got == want, (r, got)
        assert all((t[i, s] >> 8) == 0 for s in range(14) if not t[i, s] & (polar.DONOR | polar.ACCEPTOR)), r
        names = rc.restype_name_to_atom14_names[rc.restype_1to3[r]]
        assert [bool(t[i, s] & polar.ELEMENT) for s in range(14)] == [n[:1] in ('N', 'O') for n in names], r
        assert not (t[i] & ~(31 | (15 << 8))).any()
    pro, his = PC.RESTYPES.index('P'), PC.RESTYPES.index('H')
    assert t[pro, 0] == polar.ELEMENT and not (t[his] & polar.CATION).any()
    assert max(int(((t[i] & 3) != 0).sum()) for i in range(21)) == 5          # what the kernel's LDS table is sized for


def host(s, Lab, **kw):
    from abx_amd import polar
    kw.setdefault('use_points', False)
    return polar.polar_host(*s, Lab, details=True, **kw)


def test_host_twin_exact_cases():
    """Two residues, one polar atom and its antecedent each."""
    one = np.zeros((2, 14, 2), np.int32)
    row, bonds, d = host(PC.ser_asp(), 1)
    one[0, PC.SER_OG, 1] = one[1, PC.ASP_OD1, 1] = 1
    assert row.tolist() == [1, 0, 0, 0, 0, 0, -1, -1, -1, -1, -1, -1, 1, 2] and np.array_equal(bonds, one)
    assert d['pairs'] == [(0, PC.SER_OG, 1, PC.ASP_OD1)] and d['rows'].tolist() == [[1, 0, 0, -1], [1, 0, 0, -1]]
    # the distance window
    for dist, n in ((3.6, 0), (1.9, 0), (3.4, 1), (2.1, 1)):
        row, bonds, _ = host(PC.ser_asp(d=dist), 1)
        assert row[12] == row[0] == n and bonds.sum() == 2 * n and row[13] == 2, dist
    assert host(PC.ser_asp(d=3.6), 1, hb_max=3.7)[0][0] == 1 and host(PC.ser_asp(d=1.9), 1, hb_min=1.8)[0][0] == 1
    # either antecedent swung to 80 degrees
    assert host(PC.ser_asp(angle_a=80.0), 1)[0][12] == 0 and host(PC.ser_asp(angle_b=80.0), 1)[0][12] == 0
    assert host(PC.ser_asp(angle_a=100.0, angle_b=95.0), 1)[0][12] == 1
    # hb_angle = 120: 110 degrees fails on either atom, 130 passes
    for kw, n in ((dict(angle_a=110.0, angle_b=130.0), 0), (dict(angle_a=130.0, angle_b=110.0), 0), (dict(angle_a=130.0, angle_b=130.0), 1)):
        assert host(PC.ser_asp(**kw), 1, hb_angle=120.0)[0][12] == n, kw
        assert host(PC.ser_asp(**kw), 1)[0][12] == 1
    # one side against across sides, with and without a region
    reg = np.array([True, False])
    same, cross = host(PC.ser_asp(), 2, region=reg), host(PC.ser_asp(), 1, region=reg)
    assert same[0].tolist()[:6] + same[0].tolist()[12:] == [0, 0, 0, 1, 0, 0, 1, 2] and same[1][0, PC.SER_OG].tolist() == [1, 0]
    assert cross[0].tolist()[:6] + cross[0].tolist()[12:] == [1, 0, 1, 0, 0, 0, 1, 2] and cross[1][0, PC.SER_OG].tolist() == [0, 1]
    assert host(PC.ser_asp(), 2)[0][3] == 0 and host(PC.ser_asp(), 1)[0][2] == 0
    # a missing antecedent removes the atom
    x, m, aa = PC.ser_asp()
    m2 = m.copy()
    m2[0, PC.SER_CB] = False
    row, bonds, _ = host((x, m2, aa), 1)
    assert row[13] == 1 and row[12] == 0 and not bonds.any()
    # pair order: Asp first, Ser second gives the same row and the mirrored bonds
    row_s, bonds_s, _ = host(PC.ser_asp(swap=True), 1, region=reg[::-1].copy())
    assert row_s.tolist() == cross[0].tolist() and np.array_equal(bonds_s[1, PC.SER_OG], cross[1][0, PC.SER_OG]) and bonds_s[0, PC.ASP_OD1, 1] == 1
    for kw in (dict(d=3.6), dict(angle_a=80.0), dict(angle_b=80.0), dict(angle_a=100.0, angle_b=95.0)):
        assert host(PC.ser_asp(swap=True, **kw), 1)[0].tolist() == host(PC.ser_asp(**kw), 1)[0].tolist(), kw
    # residue type X has no polar atoms
    x, m, aa = PC.ser_asp()
    assert host((x, m, np.array([20, PC.ASP])), 1)[0][13] == 1


def test_salt_bridges_count_residue_pairs():
    """Lys NZ within 4 A of both Glu OE1 and OE2 is one salt bridge; beyond the cutoff none; on one side none (only the interface is
    counted); the backbone bit needs two backbone atoms."""
    row, bonds, d = host(PC.lys_glu(3.0, 3.6), 1, region=np.array([False, True]))
    assert row[4] == 1 and row[5] == 1 and d['salt'] == [(0, 1)] and d['rows'][:, 2].tolist() == [1, 1] and row[13] == 3
    assert row[1] == 0 and row[0] >= 1                                          # NZ ... OE1 is a hydrogen bond too, not a backbone one
    assert host(PC.lys_glu(3.0, 4.5), 1)[0][4] == 1 and host(PC.lys_glu(4.2, 3.9), 1)[0][4] == 1
    assert host(PC.lys_glu(4.1, 4.6), 1)[0][4] == 0 and host(PC.lys_glu(4.1, 4.6), 1, salt=4.2)[0][4] == 1
    assert host(PC.lys_glu(3.0, 3.6), 2)[0][4] == 0 and host(PC.lys_glu(3.0, 3.6), 1)[0][5] == 0


def test_burial_columns_from_point_counts():
    """acc_alone > acc_cplx: at the interface; acc_alone > 0 and acc_cplx == 0: buried; buried without a bond: unsatisfied."""
    from abx_amd import polar
    x, m, aa = PC.ser_asp(d=3.6)                                                # no bond
    pts = np.zeros((2, 14, 2), np.int32)
    pts[0, PC.SER_OG] = [40, 0]                                                 # buried, no partner: unsatisfied
    pts[1, PC.ASP_OD1] = [50, 20]                                               # at the interface, not buried
    pts[0, PC.SER_CB] = [30, 10]
    reg = np.array([True, False])
    row, _, d = polar.polar_host(x, m, aa, 1, region=reg, points=pts, details=True)
    assert row[6:10].tolist() == [2, 1, 1, 1] and d['rows'][:, 3].tolist() == [1, 0]
    R_o, R_c = float(np.float32(1.52)) + 1.4, float(np.float32(1.7)) + 1.4
    assert abs(row[10] - 4 * np.pi * R_o * R_o * 70 / 128) < 1e-9 and abs(row[11] - 4 * np.pi * R_c * R_c * 20 / 128) < 1e-9
    x, m, aa = PC.ser_asp()                                                     # the same atom with its bond: satisfied
    row, _, d = polar.polar_host(x, m, aa, 1, region=reg, points=pts, details=True)
    assert row[6:10].tolist() == [2, 1, 0, 0] and d['rows'][:, 3].tolist() == [0, 0]
    row = polar.polar_host(x, m, aa, 1, points=pts)[0]
    assert row[9] == 0 and row[2] == 0 and row[0] == 1


RECORDED = {                                         # a scratch restatement of the rule, region = CDR-H3, P = 128
    '6ct7': dict(n_polar=629, n_hbond_total=234, n_hbond_int=9, n_hbond_region=2, n_hbond_intra_region=5, n_salt_int=1, n_polar_int=47,
                 n_polar_buried=17, n_unsat=3, n_unsat_region=1, dsasa_polar=574.31, dsasa_apolar=851.03),
    '6qd7': dict(n_polar=709, n_hbond_total=234, n_hbond_int=0, n_hbond_region=0, n_hbond_intra_region=18, n_salt_int=0, n_polar_int=7,
                 n_polar_buried=0, n_unsat=0, n_unsat_region=0, dsasa_polar=73.04, dsasa_apolar=52.83),
}


@pytest.fixture(scope='module')
def shipped():
    """Host rows of the two shipped complexes (ground truth, P = 128, region = CDR-H3), computed once."""
    from abx_amd import interface, polar
    out = {}
    for code in ('6ct7', '6qd7'):
        c = RC.load_complex(code, 'h3')
        irow, pts = interface.interface_host(c['x'], c['mask'], c['aa'], c['Lab'], region=c['mov'], n_points=128)
        row, bonds, d = polar.polar_host(c['x'], c['mask'], c['aa'], c['Lab'], region=c['mov'], points=pts, details=True)
        out[code] = dict(c=c, irow=irow, pts=pts, row=row, bonds=bonds, d=d)
    return out


@pytest.mark.parametrize('code', ['6ct7', '6qd7'])
def test_shipped_complexes_give_the_recorded_numbers(shipped, code):
    from abx_amd import polar
    s = shipped[code]
    row, bonds, d, c = s['row'], s['bonds'], s['d'], s['c']
    got = dict(zip(polar.POLAR_COLUMNS, row.tolist()))
    print(code, got)
    for k, v in RECORDED[code].items():
        assert (got[k] == v) if k.startswith('n_') else (abs(got[k] - v) <= 0.005), (k, got[k], v)
    assert row[2] <= row[0] and row[1] <= row[0] and row[9] <= row[8] <= row[7] <= row[6] <= row[13] and row[5] <= row[4]
    assert abs((row[10] + row[11]) - s['irow'][3]) <= 1e-9
    assert int(bonds.sum()) == 2 * int(row[12]) == 2 * len(d['pairs']) and int(bonds[..., 1].sum()) == 2 * int(row[0])
    # the per-residue table of --polar_rows from the per-slot bonds, the salt pairs and the point counts
    L, Lab = c['aa'].shape[0], c['Lab']
    rows = d['rows']
    assert rows.shape == (L, 4) and np.array_equal(rows[:, 0], bonds[..., 1].sum(1)) and np.array_equal(rows[:, 1], bonds[..., 0].sum(1))
    assert int(rows[:, 2].sum()) == 2 * int(row[4]) and int(rows[:, 3].sum()) == int(row[8]) and int(rows[c['mov'].numpy(), 3].sum()) == int(row[9])
    t = polar.polar_table()[c['aa'].numpy()]
    is_polar = ((t & 3) != 0) & c['mask'].numpy() & np.take_along_axis(c['mask'].numpy(), (t >> 8) & 15, 1)
    unsat = is_polar & (s['pts'][..., 0] > 0) & (s['pts'][..., 1] == 0) & (bonds.sum(2) == 0)
    assert np.array_equal(rows[:, 3], unsat.sum(1)) and int(is_polar.sum()) == int(row[13])
    assert not bonds[~is_polar].any()
    for r, q in d['salt']:
        assert r < Lab <= q
    # without point counts: the burial columns are -1, everything else is unchanged
    bare = polar.polar_host(c['x'], c['mask'], c['aa'], Lab, region=c['mov'], use_points=False)[0]
    assert bare[6:12].tolist() == [-1.0] * 6 and bare[:6].tolist() == row[:6].tolist() and bare[12:].tolist() == row[12:].tolist()
    # neighbouring backbone groups: C-O ... N(i+1) never passes the angle test
    assert not any(ra + 1 == rb and sa == 3 and sb == 0 for ra, sa, rb, sb in d['pairs'])


@pytest.mark.parametrize('code', ['6ct7', '6qd7'])
@pytest.mark.parametrize('kw', [dict(), dict(hb_angle=120.0, hb_max=3.2)])
def test_an_independent_restatement_finds_the_same_bonds(shipped, code, kw):
    """Plain loops over atom names with arccos and sqrt against the twin's squared-cosine test: the same set of bonds; no compatible
    pair lies within 1e-6 A / 1e-6 degrees of a threshold on these fixtures, so nothing is left out of the comparison."""
    from abx_amd import polar
    c = shipped[code]['c']
    x, m, aa = c['x'].numpy(), c['mask'].numpy(), c['aa'].numpy()
    want, near = PC.naive_hbonds(x, m, aa, **kw)
    d = shipped[code]['d'] if not kw else polar.polar_host(x, m, aa, c['Lab'], use_points=False, details=True, **kw)[2]
    got = PC.named_pairs(d['pairs'], aa)
    print(code, kw, len(want), 'bonds,', near, 'near a threshold')
    assert near == 0 and got == want and len(got) == len(d['pairs']) > 0


def test_driver_formats(tmp_path):
    from abx_amd import design, polar
    NP = len(polar.POLAR_COLUMNS)
    row = [9.0, 2.0, 2.0, 5.0, 1.0, 0.0, 47.0, 17.0, 3.0, 1.0, 574.3099, 851.031, 234.0, 629.0]
    assert polar.format_polar(row) == ['9', '2', '2', '5', '1', '0', '47', '17', '3', '1', '574.31', '851.03', '234', '629']
    wild = [9.0, 2.0, 2.0, 5.0, 1.0, 0.0, 47.0, 17.0, 3.0, 1.0, 574.25, 851.0, 234.0, 629.0]
    d0 = [11.0, 2.0, 1.0, 5.0, 0.0, 0.0, 50.0, 19.0, 5.0, 3.0, 600.0, 840.5, 236.0, 631.0]
    d1 = [0.0] * 14
    path = design._write_polar(str(tmp_path), '6ct7_H_L_S', wild, [(0, d0), (1, d1)], False)
    assert os.path.basename(path) == '6ct7_H_L_S_polar.tsv'
    lines = [ln.split('\t') for ln in open(path).read().splitlines()]
    assert lines[0] == ['sample'] + list(polar.POLAR_COLUMNS) + ['delta_' + c for c in polar.DELTA_COLUMNS] and len(lines) == 4
    assert lines[1] == ['wild'] + polar.format_polar(wild) + ['+0', '+0', '+0', '+0', '+0', '+0', '+0.00', '+0.00']
    assert lines[2] == ['0'] + polar.format_polar(d0) + ['+2', '-1', '+0', '-1', '+2', '+2', '+25.75', '-10.50']
    assert lines[3] == ['1'] + polar.format_polar(d1) + ['-9', '-2', '-5', '-1', '-3', '-1', '-574.25', '-851.00']
    path = design._write_polar(str(tmp_path), 'x_H_L_A', wild, [(5, d0 + d1)], True)
    lines = [ln.split('\t') for ln in open(path).read().splitlines()]
    assert lines[0][1 + NP + 8:] == [c + '_relaxed' for c in polar.POLAR_COLUMNS] and len(lines) == 3
    assert lines[1][0] == 'wild' and lines[1][1 + NP + 8:] == ['nan'] * NP
    assert lines[2] == ['5'] + polar.format_polar(d0) + ['+2', '-1', '+0', '-1', '+2', '+2', '+25.75', '-10.50'] + polar.format_polar(d1)
    ap = design.build_parser()
    a = ap.parse_args([])
    assert a.polar is False and a.polar_rows is False and (a.polar_hb_max, a.polar_hb_angle, a.polar_salt) == (3.5, 90.0, 4.0)
    a = ap.parse_args(['--polar', '--polar_hb_max', '3.2', '--polar_hb_angle', '120', '--polar_salt', '4.5', '--polar_rows'])
    assert a.polar is True and a.polar_rows is True and (a.polar_hb_max, a.polar_hb_angle, a.polar_salt) == (3.2, 120.0, 4.5)


def test_sampler_signature_defaults_to_no_polar():
    import inspect
    from abx_amd import sampler
    assert inspect.signature(sampler.sample_fn).parameters['polar'].default is None
