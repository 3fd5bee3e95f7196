"""Polar interface contacts of designs: the chemical columns upstream takes from PyRosetta's InterfaceAnalyzerMover beside dG and dSASA
(hbonds_int, delta_unsatHbonds; abx/metric.py:28-59, eval/traj_evaluate.py:233-261, abx/common/energy.py) that need no force field:
hydrogen bonds and salt bridges between the antibody (rows < Lab) and the featurised antigen, and the polar atoms that binding buries
without giving them a partner.  Heavy atoms only: a donor - acceptor pair is a hydrogen bond when its distance lies in [hb_min, hb_max]
and both angles antecedent - atom ... partner are at least hb_angle (90 degrees: the HBPLUS heavy-atom rule); no hydrogens, no energies,
no His protonation (both ring nitrogens are donor and acceptor, neither a cation), no water, no cation-pi.

Every decision in float64 from the float32 coordinates in a fixed IEEE operation order (include/abx_hip.h, AbxPolarArgs): the counts of
the device (`PolarScorer`, abx_polar_scores, csrc/polar.hip) and of the host twin (`polar_host`, numpy) are equal integers.  Burial comes
from the point counts of the interface analysis (abx_amd.interface: acc_alone / acc_cplx of every atom14 slot)."""
import functools
import math

import numpy as np

from . import complex_view
from .complex_view import to_np
from .interface import FOUR_PI, SurfaceScorer

# The row of abx_polar_scores (include/abx_hip.h, ABX_POLAR_COLS)
POLAR_COLUMNS = ('n_hbond_int', 'n_hbond_int_bb', 'n_hbond_region', 'n_hbond_intra_region', 'n_salt_int', 'n_salt_region', 'n_polar_int',
                 'n_polar_buried', 'n_unsat', 'n_unsat_region', 'dsasa_polar', 'dsasa_apolar', 'n_hbond_total', 'n_polar')
COUNT_COLUMNS = tuple(c for c in POLAR_COLUMNS if c.startswith('n_'))
# design minus wild type: the columns the driver writes a difference for
DELTA_COLUMNS = ('n_hbond_int', 'n_hbond_region', 'n_hbond_intra_region', 'n_salt_int', 'n_unsat', 'n_unsat_region', 'dsasa_polar', 'dsasa_apolar')
# the per-residue table of --polar_rows (AbxPolarArgs.rows)
ROW_COLUMNS = ('n_hbond_cross', 'n_hbond_same', 'n_salt', 'n_unsat')
DONOR, ACCEPTOR, CATION, ANION, ELEMENT = 1, 2, 4, 8, 16          # ABX_POLAR_*; the antecedent's atom14 slot sits in bits 8-11

# side-chain polar atoms: residue -> {atom: (roles, antecedent)}; the backbone N (donor, CA; not Pro) and O (acceptor, C) are added to all
_SIDE_CHAINS = {
    'ARG': {'NE': (DONOR | CATION, 'CD'), 'NH1': (DONOR | CATION, 'CZ'), 'NH2': (DONOR | CATION, 'CZ')},
    'LYS': {'NZ': (DONOR | CATION, 'CE')},
    'ASN': {'ND2': (DONOR, 'CG'), 'OD1': (ACCEPTOR, 'CG')},
    'GLN': {'NE2': (DONOR, 'CD'), 'OE1': (ACCEPTOR, 'CD')},
    'TRP': {'NE1': (DONOR, 'CD1')},
    'ASP': {'OD1': (ACCEPTOR | ANION, 'CG'), 'OD2': (ACCEPTOR | ANION, 'CG')},
    'GLU': {'OE1': (ACCEPTOR | ANION, 'CD'), 'OE2': (ACCEPTOR | ANION, 'CD')},
    'HIS': {'ND1': (DONOR | ACCEPTOR, 'CG'), 'NE2': (DONOR | ACCEPTOR, 'CE1')},
    'SER': {'OG': (DONOR | ACCEPTOR, 'CB')},
    'THR': {'OG1': (DONOR | ACCEPTOR, 'CB')},
    'TYR': {'OH': (DONOR | ACCEPTOR, 'CZ')},
}


def polar_table():
    """(21,14) int32 per (residue type, atom14 slot): DONOR | ACCEPTOR | CATION | ANION role bits, ELEMENT (the atom's name starts with N
    or O), and the atom14 slot of the antecedent in bits 8-11 - from the atom14 names; residue type X (row 20) has no atoms."""
    from . import residue_constants as rc
    t = np.zeros((21, 14), np.int32)
    for i, r in enumerate(rc.restypes):
        res = rc.restype_1to3[r]
        names = rc.restype_name_to_atom14_names[res]
        roles = dict(_SIDE_CHAINS.get(res, {}), O=(ACCEPTOR, 'C'))
        if res != 'PRO':
            roles['N'] = (DONOR, 'CA')
        for slot, name in enumerate(names):
            if name[:1] in ('N', 'O'):
                t[i, slot] |= ELEMENT
            if name in roles:
                t[i, slot] |= roles[name][0] | (names.index(roles[name][1]) << 8)
    return t


_TABLE = {}


def polar_table_on(device):
    """polar_table() as an int32 tensor on `device` (cached per device)."""
    import torch
    key = str(device)
    if key not in _TABLE:
        _TABLE[key] = torch.from_numpy(polar_table()).to(device).contiguous()
    return _TABLE[key]


def cos2_of(hb_angle):
    """cos^2 of an angle in degrees as the kernel and the host twin use it: exactly 0.0 at 90 degrees."""
    hb_angle = float(hb_angle)
    return 0.0 if hb_angle == 90.0 else math.cos(math.radians(hb_angle)) ** 2


# format_polar(row): %.2f for the areas (square Angstrom), integers for the counts; format_delta(row, wild): design minus wild type for
# DELTA_COLUMNS, signed
format_polar = functools.partial(complex_view.format_row, POLAR_COLUMNS, COUNT_COLUMNS, 2)
format_delta = functools.partial(complex_view.format_delta, POLAR_COLUMNS, COUNT_COLUMNS, DELTA_COLUMNS, 2)


class PolarScorer(SurfaceScorer):
    """Polar rows of batches of designs of ONE complex on the device.  Built once per complex from its featurised batch (or the
    un-batched complex) like interface.InterfaceScorer, and holds one for the point counts (interface.SurfaceScorer: region, n_points /
    probe of the surface, interface).  hb_min / hb_max: donor - acceptor distance range (Angstrom); hb_angle: smallest antecedent - atom
    ... partner angle (degrees, [90, 180)); salt: cation - anion distance."""

    COLUMNS = POLAR_COLUMNS

    def __init__(self, batch, region=None, hb_min=2.0, hb_max=3.5, hb_angle=90.0, salt=4.0, n_points=128, probe=1.4, interface=None):
        if not (0 <= hb_min <= hb_max and 90.0 <= hb_angle < 180.0 and salt >= 0):
            raise ValueError(f'polar: needs 0 <= hb_min <= hb_max, 90 <= hb_angle < 180, salt >= 0 (got {hb_min}, {hb_max}, {hb_angle}, {salt})')
        super().__init__(batch, region, n_points, probe, interface)
        it = self.interface
        self.table = polar_table_on(self.device)
        self.kw = dict(hb_min=float(hb_min), hb_max=float(hb_max), hb_angle=float(hb_angle), salt=float(salt),
                       n_points=int(it.sphere.shape[0]), probe=it.kw['probe'])

    def score(self, atom14, seq, out=None, bonds=None, points=None, rows=None, mask=None):
        """atom14 (B, Lab or L, 14, 3) f32 predicted coordinates, seq (B, Lab) tokens -> (B, len(POLAR_COLUMNS)) float64 on the device;
        out: rows to write into (any row stride); bonds: (B,L,14,2) int32 to receive the same-side / cross-side bonds of every slot;
        rows: (B,L,4) int32 to receive ROW_COLUMNS of every residue; points: the (B,L,14,2) int32 acc_alone / acc_cplx that the
        interface scorer returned for THESE structures (None: its kernel runs here).  No host synchronisation."""
        from abx_amd import ops
        points = self.points_of(atom14, seq, points, mask)
        return ops.polar_scores(atom14, seq, self.gt_atom14, self.gt_seq, self.gt_exists, self.table, Lab=self.Lab, region=self.region, mask=mask,
                                res_mask=self.res_mask, points=points, out=out, bonds=bonds, rows=rows, **self.kw)

    def side_outputs(self, B):
        """want_rows: the record of the designs also carries 'polar_bonds' (B, L, 14, 2) and 'polar_rows' (B, L, 4) int32."""
        import torch
        if not self.want_rows:
            return {}
        return dict(bonds=torch.empty(B, self.L, 14, 2, dtype=torch.int32, device=self.device),
                    rows=torch.empty(B, self.L, 4, dtype=torch.int32, device=self.device))

    # record(): 'polar' - hydrogen bonds and salt bridges across the interface, polar atoms buried without a partner - and, with a
    # relaxer, 'polar_relaxed'; one launch per table


# -------------------------------------------------------------------------------------------------------------------
# host twin (float64, numpy)
# -------------------------------------------------------------------------------------------------------------------
def polar_atoms(x, mask, aa):
    """The polar atoms of one structure in the kernel's (row, slot) order: (rows, slots, flags, c (N,3) float64, u (N,3) float64 =
    antecedent minus atom).  x (L,14,3) float32, mask (L,14) bool, aa (L) tokens in 0..20."""
    t = polar_table()[aa]                                                       # (L,14)
    ante = (t >> 8) & 15
    ok = ((t & (DONOR | ACCEPTOR)) != 0) & mask & np.take_along_axis(mask, ante, 1)
    rows, slots = np.nonzero(ok)
    c = x[rows, slots].astype(np.float64)
    u = x[rows, ante[rows, slots]].astype(np.float64) - c
    return rows, slots, t[rows, slots], c, u


def residue_rows(rows, L, bonds, salt_pairs, unsat=None):
    """(L,4) int32 ROW_COLUMNS from the per-slot bonds (L,14,2), the salt-bridged row pairs [(r, s), ...] and the unsatisfied atoms'
    rows (None: -1)."""
    out = np.zeros((L, 4), np.int32)
    out[:, 0] = bonds[..., 1].sum(1)
    out[:, 1] = bonds[..., 0].sum(1)
    for r, s in salt_pairs:
        out[r, 2] += 1
        out[s, 2] += 1
    if unsat is None:
        out[:, 3] = -1
    else:
        np.add.at(out[:, 3], unsat, 1)
    return out


def polar_host(x, mask, aa, Lab, region=None, points=None, hb_min=2.0, hb_max=3.5, hb_angle=90.0, salt=4.0, n_points=128, probe=1.4,
               use_points=True, details=False):
    """The row of abx_polar_scores for ONE structure on the host, with the same IEEE operations in the same order (no fused
    multiply-add: numpy multiplies and adds in separate passes).  x (L,14,3) coordinates (rounded to float32 first: what the kernel
    reads), mask (L,14) which slots exist, aa (L) residue tokens, Lab = rows of side A, region (L) or None, points (L,14,2) acc_alone /
    acc_cplx of every slot (None: interface.interface_host computes them with n_points and probe; use_points=False: no burial, columns
    6-11 are -1 as with AbxPolarArgs.points == NULL).
    -> (row (len(POLAR_COLUMNS),) float64, bonds (L,14,2) int32: same-side, cross-side bonds of every slot); details=True adds a dict:
    'pairs' [(row_a, slot_a, row_b, slot_b), ...] the bonds, 'salt' [(row, row), ...], 'rows' (L,4) int32 ROW_COLUMNS."""
    from .interface import _radius_table, interface_host
    x = to_np(x).astype(np.float32)
    L = x.shape[0]
    aa = np.clip(to_np(aa).astype(np.int64), 0, 20)
    mask = to_np(mask) != 0
    reg_row = np.zeros(L, bool) if region is None else (to_np(region) != 0)
    hb_min, hb_max, salt, probe = float(hb_min), float(hb_max), float(salt), float(probe)
    if not 90.0 <= float(hb_angle) < 180.0:
        raise ValueError(f'polar: hb_angle = {hb_angle} outside [90, 180)')
    cos2 = cos2_of(hb_angle)
    rows, slots, fl, c, u = polar_atoms(x, mask, aa)
    N = rows.shape[0]
    side = rows >= Lab
    reg = reg_row[rows]
    bonds = np.zeros((L, 14, 2), np.int32)
    cnt = np.zeros(len(POLAR_COLUMNS), np.float64)
    pairs, salt_pairs = [], []
    if N:
        # a = the first index, b = the second: d = b - a, upper triangle of different rows
        dx, dy, dz = (c[None, :, k] - c[:, None, k] for k in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        upper = (rows[:, None] != rows[None]) & (np.arange(N)[:, None] < np.arange(N)[None])
        don, acc = (fl & DONOR) != 0, (fl & ACCEPTOR) != 0
        roles = (don[:, None] & acc[None]) | (acc[:, None] & don[None])
        cand = upper & roles & (d2 >= hb_min * hb_min) & (d2 <= hb_max * hb_max)
        ia, ib = np.nonzero(cand)
        ex, ey, ez, e2 = dx[ia, ib], dy[ia, ib], dz[ia, ib], d2[ia, ib]
        ua, ub = u[ia], u[ib]
        ta = (ua[:, 0] * ex + ua[:, 1] * ey) + ua[:, 2] * ez
        uu = (ua[:, 0] * ua[:, 0] + ua[:, 1] * ua[:, 1]) + ua[:, 2] * ua[:, 2]
        tb = (ub[:, 0] * ex + ub[:, 1] * ey) + ub[:, 2] * ez
        vv = (ub[:, 0] * ub[:, 0] + ub[:, 1] * ub[:, 1]) + ub[:, 2] * ub[:, 2]
        hb = (ta <= 0.0) & (ta * ta >= cos2 * (uu * e2)) & (tb >= 0.0) & (tb * tb >= cos2 * (vv * e2))
        ia, ib = ia[hb], ib[hb]
        cross = side[ia] != side[ib]
        either = reg[ia] | reg[ib]
        np.add.at(bonds, (rows[ia], slots[ia], cross.astype(np.int64)), 1)
        np.add.at(bonds, (rows[ib], slots[ib], cross.astype(np.int64)), 1)
        cnt[0] = cross.sum()
        cnt[1] = (cross & (slots[ia] < 4) & (slots[ib] < 4)).sum()
        cnt[2] = (cross & either).sum()
        cnt[3] = (~cross & either).sum()
        cnt[12] = ia.shape[0]
        pairs = list(zip(rows[ia].tolist(), slots[ia].tolist(), rows[ib].tolist(), slots[ib].tolist()))
        # salt bridges: residue pairs across the interface, once each
        cat, ani = (fl & CATION) != 0, (fl & ANION) != 0
        sb = upper & (side[:, None] != side[None]) & ((cat[:, None] & ani[None]) | (ani[:, None] & cat[None])) & (d2 <= salt * salt)
        sa, sb_ = np.nonzero(sb)
        salt_pairs = sorted(set(zip(rows[sa].tolist(), rows[sb_].tolist())))
        cnt[4] = len(salt_pairs)
        cnt[5] = sum(1 for r, s in salt_pairs if reg_row[r] or reg_row[s])
    cnt[13] = N
    unsat_rows = None
    if use_points:
        if points is None:
            points = interface_host(x, mask, aa, Lab, region=region, n_points=n_points, probe=probe)[1]
        points = to_np(points).astype(np.int64)
        alone, cplx = points[rows, slots, 0], points[rows, slots, 1]
        buried = (alone > 0) & (cplx == 0)
        unsat = buried & (bonds[rows, slots].sum(1) == 0)
        cnt[6], cnt[7], cnt[8], cnt[9] = (alone > cplx).sum(), buried.sum(), unsat.sum(), (unsat & reg).sum()
        unsat_rows = rows[unsat]
        rad = _radius_table()[aa]                                               # (L,14) float32
        ok = mask & (rad > 0)
        R = rad.astype(np.float64) + probe
        area = FOUR_PI * (R * R) * (points[..., 0] - points[..., 1]).astype(np.float64) / float(n_points)
        elem = (polar_table()[aa] & ELEMENT) != 0
        cnt[10], cnt[11] = area[ok & elem].sum(), area[ok & ~elem].sum()
    else:
        cnt[6:12] = -1.0
    if details:
        return cnt, bonds, dict(pairs=pairs, salt=salt_pairs, rows=residue_rows(rows, L, bonds, salt_pairs, unsat_rows))
    return cnt, bonds
