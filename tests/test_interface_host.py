"""CPU-only checks of the interface analysis (abx_interface_scores, abx_amd.interface): C layout of the descriptor, argument checks
without a GPU, exact cases of the float64 host twin, its discretisation error against the spherical-cap closed form, the two shipped
complexes, and the formats of the design driver."""
import ctypes
import os

import numpy as np
import pytest

import host_cases as HC
import relax_cases as RC

R_C, R_N = float(np.float32(1.7)) + 1.4, float(np.float32(1.55)) + 1.4      # inflated radii of a carbon (slot 1) and a nitrogen (slot 0)


@pytest.fixture(scope='module')
def lib():
    return HC.load_lib()


def test_interface_args_match_c_layout():
    """sizeof / offsetof of AbxInterfaceArgs as gcc lays it out, and ABX_IFACE_COLS against the Python side."""
    from abx_amd import _lib, interface
    st = _lib.AbxInterfaceArgs
    c_layout = HC.assert_c_layout({'AbxInterfaceArgs': st}, ['ABX_IFACE_COLS'])
    assert c_layout['ABX_IFACE_COLS'] == _lib.IFACE_COLS == len(interface.INTERFACE_COLUMNS) == 12
    assert interface.COUNT_COLUMNS == interface.INTERFACE_COLUMNS[6:]
    assert [interface.INTERFACE_COLUMNS.index(c) for c in interface.DELTA_COLUMNS] == [3, 4, 5, 9, 10]


def test_interface_argument_checks_without_gpu(lib):
    """Every malformed descriptor comes back negative before any launch, with the entry's name in the error string."""
    from abx_amd._lib import AbxInterfaceArgs
    P = 0x1000                                      # any non-null "device pointer": nothing is dereferenced

    def good():
        a = AbxInterfaceArgs()
        a.pred_atom14 = a.pred_seq = a.gt_atom14 = a.gt_exists = a.gt_seq = a.radius = a.sphere = a.out = P
        a.B, a.L, a.Lab, a.Lpred, a.P = 4, 40, 30, 30, 128
        a.pred_sb, a.pred_seq_sb, a.out_stride = 30 * 42, 30, 12
        a.probe, a.cutoff = 1.4, 4.0
        return a

    def bad(a, ws=P):
        rc = lib.abx_interface_scores(ctypes.byref(a) if a is not None else None, ws, None)
        msg = lib.abx_last_error_string()
        assert rc < 0 and b'abx_interface_scores' in msg, (rc, msg)

    assert lib.abx_interface_scores_workspace_bytes(4, 40, 128) >= 4 * (16 + 40 * 14 * 36)
    assert lib.abx_interface_scores_workspace_bytes(100, 352, 128) == lib.abx_interface_scores_workspace_bytes(100, 352, 960) < 20 << 20
    bad(None)
    bad(AbxInterfaceArgs())
    for field in ('pred_atom14', 'pred_seq', 'gt_atom14', 'gt_exists', 'gt_seq', 'radius', 'sphere', 'out'):
        a = good()
        setattr(a, field, None)
        bad(a)
    for field, v in (('B', 0), ('B', -3), ('L', 0), ('L', -1), ('Lab', 41), ('Lab', 0), ('Lpred', 29), ('Lpred', 41), ('out_stride', 11),
                     ('P', 0), ('P', -1), ('P', 1025), ('probe', -0.1), ('probe', float('nan')), ('cutoff', 0.0), ('cutoff', -4.0),
                     ('cutoff', float('nan'))):
        a = good()
        setattr(a, field, v)
        bad(a)
    a = good()                                      # an atom table beyond the LDS of a CU
    a.L, a.Lab, a.Lpred = 542, 300, 300
    bad(a)
    assert 20 * 14 * 541 + 12288 <= 160 * 1024 < 20 * 14 * 542 + 12288
    bad(good(), ws=None)


def atoms(*specs):
    """A structure of len(specs) residues (alanine) with ONE atom each: specs = (slot, xyz).  Slot 0 is a nitrogen, slot 1 a carbon."""
    n = len(specs)
    x, m = np.zeros((n, 14, 3), np.float32), np.zeros((n, 14), bool)
    for i, (slot, pos) in enumerate(specs):
        x[i, slot] = pos
        m[i, slot] = True
    return x, m, np.zeros(n, np.int64)


@pytest.mark.parametrize('P', [1, 64, 100, 128, 960])
def test_host_twin_exact_cases(P):
    from abx_amd import interface
    host = lambda s, Lab, **kw: interface.interface_host(*s, Lab, n_points=P, **kw)
    # an isolated atom: every point free, the area of its inflated sphere
    row, pts = host(atoms((1, [3.0, -2.0, 7.5])), 1)
    assert pts[0, 1].tolist() == [P, P] and int(pts.sum()) == 2 * P
    want = 4 * np.pi * R_C * R_C
    assert abs(row[0] - want) <= 1e-14 * want and row[1] == row[0] and row[11] == 1 and row[2:11].tolist() == [0.0] * 9
    # a nitrogen 0.1 A from a carbon: wholly inside the carbon's sphere (2.95 + 0.1 < 3.1), the carbon untouched (3.1 - 0.1 > 2.95)
    pair = atoms((1, [1.0, 2.0, 3.0]), (0, [1.0, 2.1, 3.0]))
    row, pts = host(pair, 2)
    assert pts[0, 1].tolist() == [P, P] and pts[1, 0].tolist() == [0, 0]
    assert row[3:11].tolist() == [0.0] * 8 and row[0] == row[1] and abs(row[0] - want) <= 1e-14 * want
    # the same pair on different sides: the nitrogen is free alone and lost in the complex; one contact, counted once
    row, pts = host(pair, 1, region=np.array([True, False]))
    assert pts[0, 1].tolist() == [P, P] and pts[1, 0].tolist() == [P, 0]
    buried = 4 * np.pi * R_N * R_N
    assert abs(row[3] - buried) <= 1e-14 * buried and abs(row[2] - buried) <= 1e-14 * buried and row[4] == row[5] == 0.0
    assert row[6:12].tolist() == [0.0, 1.0, 0.0, 1.0, 1.0, 2.0]
    row, _ = host(pair, 1, region=np.array([False, True]))
    assert abs(row[5] - buried) <= 1e-14 * buried and row[6:12].tolist() == [0.0, 1.0, 1.0, 1.0, 0.0, 2.0]
    # beyond the contact cutoff but with overlapping probe spheres: surface is buried, no contact
    far = atoms((1, [0.0, 0.0, 0.0]), (0, [0.0, 0.0, 4.5]))
    row, pts = host(far, 1)
    assert row[9] == 0 and (P < 64 or (row[3] > 0 and row[6:8].tolist() == [1.0, 1.0] and pts[0, 1, 0] == P > pts[0, 1, 1]))
    assert host(far, 1, cutoff=4.6)[0][9] == 1
    # an empty side B: columns 2-10 are 0 and the complex is the antibody
    row, pts = host(far, 2)
    assert row[2:11].tolist() == [0.0] * 9 and row[0] == row[1] and np.array_equal(pts[..., 0], pts[..., 1])
    # a masked slot and a slot without a radius (alanine has no slot 7) are no atoms
    x, m, aa = far
    m2 = m.copy()
    m2[1, 0] = False
    m2[0, 7] = True
    row, pts = host((x, m2, aa), 1)
    assert row[11] == 1 and pts[0, 1].tolist() == [P, P] and int(pts.sum()) == 2 * P


def cap_error(P):
    """Worst relative error of the host twin's exposed areas of two overlapping spheres (R = 3.1 and 2.95 A: a carbon and a nitrogen
    with the 1.4 A probe) against A_i = 4 pi R_i^2 - 2 pi R_i h_i, h_i = R_i - (d^2 + R_i^2 - R_j^2) / (2 d), over five separations
    along a generic direction."""
    from abx_amd import interface
    direction = np.array([0.36, 0.48, 0.8])
    origin = np.array([1.5, -2.25, 0.75])
    worst = 0.0
    for d in (1.0, 2.0, 3.0, 4.5, 5.5):
        _, pts = interface.interface_host(*atoms((1, origin), (0, origin + d * direction)), 2, n_points=P)
        for R, Ro, n in ((3.1, 2.95, pts[0, 1, 0]), (2.95, 3.1, pts[1, 0, 0])):
            h = R - (d * d + R * R - Ro * Ro) / (2 * d)
            exact = 4 * np.pi * R * R - 2 * np.pi * R * h
            worst = max(worst, abs(4 * np.pi * R * R * n / P - exact) / exact)
    return worst


def test_two_spheres_against_the_spherical_cap_closed_form():
    """The discretisation error has no closed form: measured on this point set it is 1.947e-2 at P = 128 and 7.92e-3 at P = 960 (worst of
    the ten areas, relative to the exact exposed area); the bounds are twice that, and more points must do better."""
    e128, e960 = cap_error(128), cap_error(960)
    print(f'spherical caps: worst relative error {e128:.4e} at P = 128, {e960:.4e} at P = 960')
    assert e128 <= 2 * 1.947e-2 and e960 <= 2 * 7.92e-3 and e960 < e128


@pytest.fixture(scope='module')
def shipped():
    """Host rows and point counts of the two shipped complexes (ground truth, P = 128, region = CDR-H3), computed once."""
    from abx_amd import interface
    out = {}
    for code in ('6ct7', '6qd7'):
        c = RC.load_complex(code, 'h3')
        row, pts = interface.interface_host(c['x'], c['mask'], c['aa'], c['Lab'], region=c['mov'], n_points=128)
        out[code] = (c, row, pts)
    return out


@pytest.mark.parametrize('code', ['6ct7', '6qd7'])
def test_shipped_complex_identities(shipped, code):
    from abx_amd import ops
    c, row, pts = shipped[code]
    print(code, row.tolist())
    L, Lab = c['aa'].shape[0], c['Lab']
    # complex = antibody + antigen - buried (sums of <= 5 000 terms of one sign: N eps sum)
    assert abs(row[0] - (row[1] + row[2] - row[3])) <= 1e-9 * row[0]
    assert row[3] >= row[4] >= 0 and row[4] >= row[5] >= 0            # H3 lies on side A
    exists = c['mask'].numpy() & (ops.vdw_radius_table('cpu').numpy()[c['aa'].numpy()] > 0)
    assert row[11] == exists.sum() == {'6ct7': 1741, '6qd7': 1967}[code]
    assert not pts[~exists].any() and pts.min() >= 0 and pts.max() <= 128 and (pts[..., 1] <= pts[..., 0]).all()
    touched = (pts[..., 0] > pts[..., 1]).any(1)
    assert row[6] == touched[:Lab].sum() and row[7] == touched[Lab:].sum() and row[8] == touched[c['mov'].numpy()].sum()
    assert row[6] + row[7] <= L and row[9] >= row[10] >= 0
    # the areas from the counts, atom by atom
    R = ops.vdw_radius_table('cpu').numpy()[c['aa'].numpy()].astype(np.float64) + 1.4
    area = lambda n: (4 * np.pi * R * R * n / 128)[exists].sum()
    assert abs(area(pts[..., 1]) - row[0]) <= 1e-9 * row[0] and abs(area(pts[..., 0] - pts[..., 1]) - row[3]) <= 1e-9 * row[0]


def test_shipped_complexes_are_plausible(shipped):
    """6ct7's CDR-H3 sits on the antigen, the cropped 6qd7 patch barely touches the antibody (and not with H3)."""
    _, ct7, _ = shipped['6ct7']
    _, qd7, _ = shipped['6qd7']
    assert ct7[5] > 0 and ct7[9] > 50 and ct7[3] > 10 * qd7[3] > 0 and ct7[8] >= 1
    assert qd7[8] == 0 and qd7[5] == 0 and qd7[10] == 0


def test_sphere_points_are_the_golden_spiral():
    import torch
    from abx_amd import interface
    for P in (1, 100, 128, 1024):
        u = interface.sphere_points(P)
        assert u.dtype == torch.float64 and tuple(u.shape) == (P, 3) and interface.sphere_points(P) is u
        assert float((u.norm(dim=1) - 1).abs().max()) <= 4e-16
        k = np.arange(P)
        assert np.array_equal(u[:, 2].numpy(), 1.0 - (2.0 * k + 1.0) / P)
    for P in (0, 1025):
        with pytest.raises(ValueError):
            interface.sphere_points(P)


def test_driver_formats(tmp_path):
    from abx_amd import design, interface
    NI = len(interface.INTERFACE_COLUMNS)
    row = [10391.536, 10363.164, 1450.8, 1422.424, 633.79, 84.0049, 30.0, 10.0, 3.0, 119.0, 18.0, 1741.0]
    assert interface.format_interface(row) == ['10391.54', '10363.16', '1450.80', '1422.42', '633.79', '84.00', '30', '10', '3', '119', '18', '1741']
    wild = [100.0, 80.0, 40.0, 20.0, 11.0, 5.25, 4.0, 3.0, 2.0, 17.0, 6.0, 900.0]
    d0 = [99.0, 80.5, 40.0, 21.5, 11.0, 3.0, 5.0, 3.0, 1.0, 15.0, 9.0, 901.0]
    d1 = [140.0, 100.0, 40.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 899.0]
    path = design._write_interface(str(tmp_path), '6ct7_H_L_S', wild, [(0, d0), (1, d1)], False)
    assert os.path.basename(path) == '6ct7_H_L_S_interface.tsv'
    lines = [ln.split('\t') for ln in open(path).read().splitlines()]
    assert lines[0] == ['sample'] + list(interface.INTERFACE_COLUMNS) + ['delta_' + c for c in interface.DELTA_COLUMNS] and len(lines) == 4
    assert lines[1] == ['wild'] + interface.format_interface(wild) + ['+0.00', '+0.00', '+0.00', '+0', '+0']
    assert lines[2] == ['0'] + interface.format_interface(d0) + ['+1.50', '+0.00', '-2.25', '-2', '+3']
    assert lines[3] == ['1'] + interface.format_interface(d1) + ['-20.00', '-11.00', '-5.25', '-17', '-6']
    # with --relax: the relaxed structure's columns follow, suffixed _relaxed; the wild type has none
    path = design._write_interface(str(tmp_path), 'x_H_L_A', wild, [(5, d0 + d1)], True)
    lines = [ln.split('\t') for ln in open(path).read().splitlines()]
    assert lines[0][1 + NI + 5:] == [c + '_relaxed' for c in interface.INTERFACE_COLUMNS] and len(lines) == 3
    assert lines[1][0] == 'wild' and lines[1][1 + NI + 5:] == ['nan'] * NI
    assert lines[2] == ['5'] + interface.format_interface(d0) + ['+1.50', '+0.00', '-2.25', '-2', '+3'] + interface.format_interface(d1)
    ap = design.build_parser()
    a = ap.parse_args([])
    assert a.interface is False and (a.interface_points, a.interface_probe, a.interface_cutoff) == (128, 1.4, 4.0)
    a = ap.parse_args(['--interface', '--interface_points', '960', '--interface_probe', '1.2', '--interface_cutoff', '4.5'])
    assert a.interface is True and (a.interface_points, a.interface_probe, a.interface_cutoff) == (960, 1.2, 4.5)


def test_sampler_signature_defaults_to_no_interface():
    import inspect
    from abx_amd import sampler
    assert inspect.signature(sampler.sample_fn).parameters['interface'].default is None
