"""Torsion analysis of designs: are the angles BETWEEN the residues, and the chi angles of the side chains, those of a protein - and those
of the crystal structure?  The frame-based generator builds every residue with ideal internal geometry; phi, psi and omega come from two
independent frames, chi from the torsion head.

  omega     of the link (i-1, i): cis (|omega| < 30), twisted (30 <= |omega| < 150), cis before a non-proline.
  phi       residues other than Gly with phi >= 0.
  ABEGO     the five coarse boxes of the Ramachandran plane (A helical, B extended, G and E their mirror images at phi >= 0, O a cis
            peptide) of the designed residues, as counts, as agreement with the crystal structure and as the string of `abego_string`.
  backbone  mean and largest circular difference of phi, psi, omega to the crystal structure over the designed residues.
  chi       chi1 / chi1+2 recovery within `chi_tol` and the mean |delta chi| over the designed residues that kept their type; a chi
            with a symmetric end (Asp chi2, Glu chi3, Phe / Tyr chi2) is compared modulo 180 degrees.

A link is topological - same chain, consecutive residue numbers, N, CA and C present in both residues (the rule of metrics'
linked neighbours) -, not a distance: a broken bond still has an omega.  No Ramachandran probability surface, ABEGO is five boxes, no
hydrogens, the chi of a mutated residue is not compared, chirality is not checked (the atom builder cannot make a D-residue).

Every decision is taken on the pair (x, y) = (n1.n2, |b2| b1.n2) of a dihedral - products, a square root and a comparison in float64
from the float32 coordinates in a fixed IEEE operation order against (cos, sin) pairs computed once on the host (`thresholds`) - so the
counts, codes and flags of the device (`TorsionScorer`, abx_torsion_scores, csrc/torsions.hip) and of the host twin (`torsions_host`,
numpy) are equal; atan2 only reports, and the angle columns agree to its last bits.  The definitions, operation by operation:
include/abx_hip.h, AbxTorsionArgs."""
import functools

import numpy as np

from . import complex_view
from .complex_view import Borderline as _Borderline, to_np, type_index

# The row of abx_torsion_scores (include/abx_hip.h, ABX_TORSION_COLS)
TORSIONS_COLUMNS = ('n_links', 'cis', 'cis_nonpro', 'twisted', 'n_links_region', 'cis_region', 'twisted_region', 'phi_pos', 'phi_pos_region',
                    'abego_A', 'abego_B', 'abego_G', 'abego_E', 'abego_O', 'n_abego', 'abego_same', 'dphi_region', 'dpsi_region',
                    'domega_region', 'dbb_max_region', 'n_chi1', 'chi1_ok', 'n_chi12', 'chi12_ok', 'chi_mae_region')
MEAN_COLUMNS = ('dphi_region', 'dpsi_region', 'domega_region', 'dbb_max_region', 'chi_mae_region')
COUNT_COLUMNS = tuple(c for c in TORSIONS_COLUMNS if c not in MEAN_COLUMNS)
# design minus wild type: the columns the driver writes a difference for
DELTA_COLUMNS = ('cis', 'cis_nonpro', 'twisted', 'cis_region', 'twisted_region', 'phi_pos', 'phi_pos_region', 'abego_A', 'abego_B', 'abego_G',
                 'abego_E', 'abego_O')
# the per-residue table of --torsions_rows (AbxTorsionArgs.rows); angles in degrees, nan where undefined
ROW_COLUMNS = ('phi', 'psi', 'omega', 'chi1', 'chi2', 'chi3', 'chi4', 'flags')
ABEGO = '-ABGEO'                                        # the letter of a code; 0: undefined
F_CODE, F_CIS, F_TWISTED, F_PHI_POS, F_REGION, F_CHI1, F_CHI1_OK = 7, 8, 16, 32, 64, 128, 256     # the flag word of ROW_COLUMNS
MAX_LAB = 800                                           # ABX_TORSION_MAX_LAB
# the thresholds of AbxTorsionArgs in degrees, but the chi tolerance
ANGLES = dict(cis=30.0, trans=150.0, o=90.0, a_mid=-12.5, a_half=62.5, g_half=100.0)
DEG = 57.29577951308232                                 # 180 / pi, the constant of csrc/torsions.hip
_PLACES = 2

format_torsions = functools.partial(complex_view.format_row, TORSIONS_COLUMNS, COUNT_COLUMNS, _PLACES)
format_delta = functools.partial(complex_view.format_delta, TORSIONS_COLUMNS, COUNT_COLUMNS, DELTA_COLUMNS, _PLACES)


def thresholds(chi_tol=40.0):
    """{name: (cos, sin)} of AbxTorsionArgs' threshold pairs, float64: computed HERE for the device and for the twin."""
    if not 0.0 < float(chi_tol) <= 180.0:
        raise ValueError(f'torsions: chi_tol must be in (0, 180] degrees (got {chi_tol})')
    out = {}
    for k, deg in dict(ANGLES, chi_tol=float(chi_tol)).items():
        r = np.deg2rad(np.float64(deg))
        out[k] = (float(np.cos(r)), float(np.sin(r)))
    return out


@functools.lru_cache(maxsize=None)
def chi_table():
    """(chi_atoms (21,4,4) int32: the atom14 slots of chi_k of a residue type, -1 where it has none; chi_pi (21,4) uint8: chi_k is
    compared modulo 180 degrees) from residue_constants.chi_angles_atom_indices (atom37), chi_angles_mask and chi_pi_periodic."""
    from . import residue_constants as rc
    idx37 = np.asarray(rc.chi_angles_atom_indices).astype(np.int64)                             # (21,4,4)
    a14 = np.asarray(rc.restype_atom37_to_atom14).astype(np.int64)                              # (21,37)
    has = np.asarray(rc.chi_angles_mask) > 0
    typed = np.asarray(rc.restype_atom14_mask) > 0
    slots = np.take_along_axis(a14[:, None, :].repeat(4, 1), idx37, 2)
    for t in range(21):
        for k in range(4):
            assert not has[t, k] or typed[t, slots[t, k]].all(), (t, k)
    atoms = np.where(has[:, :, None], slots, -1).astype(np.int32)
    pi = (np.asarray(rc.chi_pi_periodic) > 0) & has
    atoms.setflags(write=False)
    return atoms, pi.astype(np.uint8)


def abego_string(classes, region):
    """The ABEGO letters of the rows of `region` (a mask over the rows of `classes`, or longer), '-' where the code is 0."""
    cl = np.asarray(classes).astype(np.int64)
    reg = np.asarray(region)[:cl.shape[0]] != 0
    return ''.join(ABEGO[int(v)] for v in cl[reg])


class TorsionScorer(complex_view.ComplexView):
    """Torsion rows of batches of designs of ONE complex on the device.  Built once per complex from its featurised batch (or the
    un-batched complex) like accuracy.AccuracyScorer.  region: (L) mask of the designed rows the `*_region` columns describe (default: the
    rows the sampler diffuses).  chi_tol: the largest |delta chi| of a recovered chi angle, in (0, 180] degrees."""

    COLUMNS = TORSIONS_COLUMNS

    def __init__(self, batch, region=None, chi_tol=40.0):
        import torch
        super().__init__(batch, chains=True)
        if self.Lab > MAX_LAB:
            raise ValueError(f'torsions: the antibody has {self.Lab} rows, abx_torsion_scores takes at most {MAX_LAB}')
        dev = self.gt_atom14.device
        self.region = complex_view.region_mask(batch, region, dev)
        atoms, pi = chi_table()
        self.tables = (torch.from_numpy(np.array(atoms)).to(dev), torch.from_numpy(np.array(pi)).to(dev))
        self.kw = dict(thresholds=thresholds(chi_tol), gly=type_index('G'), pro=type_index('P'))

    def new_rows(self, B):
        """An uninitialised (B, Lab, 8) float64 tensor for ROW_COLUMNS of B structures."""
        import torch
        return torch.empty(B, self.Lab, 8, dtype=torch.float64, device=self.region.device)

    def new_classes(self, B):
        """An uninitialised (B, Lab) int32 tensor for the ABEGO codes of B structures."""
        import torch
        return torch.empty(B, self.Lab, dtype=torch.int32, device=self.region.device)

    def score(self, atom14, seq, rows=None, classes=None, out=None, mask=None, workspace=None):
        """atom14 (B, Lab or L, 14, 3) f32 predicted coordinates (only the antibody rows are read), seq (B, Lab) tokens ->
        (B, len(TORSIONS_COLUMNS)) float64 on the device; out: rows to write into (any row stride); rows: (B,Lab,8) float64 to receive
        ROW_COLUMNS; classes: (B,Lab) int32 to receive the ABEGO codes; mask: (B,L,14) or None (the atoms of the tokens); workspace: a
        uint8 tensor of at least ops.torsion_workspace_bytes(B, Lab) bytes (None: allocated here).  One launch, no host synchronisation."""
        from abx_amd import ops
        return ops.torsion_scores(atom14, seq, self.gt_atom14, self.gt_seq, self.gt_exists, self.chain_id, self.residx, self.tables, Lab=self.Lab,
                                  region=self.region, mask=mask, res_mask=self.res_mask, out=out, rows=rows, classes=classes,
                                  workspace=workspace, **self.kw)

    def side_outputs(self, B):
        """The record of the designs also carries 'torsions_classes' (B, Lab) int32, the ABEGO codes, and with want_rows 'torsions_rows'
        (B, Lab, 8) float64."""
        return dict({'rows': self.new_rows(B)} if self.want_rows else {}, classes=self.new_classes(B))

    # wild(**kw): the crystal structure against itself - abego_same == n_abego, every difference 0, every compared chi ok: the first line
    # of the driver's table
    # record(): 'torsions' - cis and twisted peptides, phi >= 0, the ABEGO classes, the backbone dihedrals and the chi angles against the
    # crystal structure - and, with a relaxer, 'torsions_relaxed'; one launch per table


# -------------------------------------------------------------------------------------------------------------------
# host twin (float64, numpy)
# -------------------------------------------------------------------------------------------------------------------
def dihedral_xy(a, b, c, d):
    """csrc/torsions.hip::dihedral, operation for operation, over leading axes: (x, y) with angle = atan2(y, x)."""
    b1, b2, b3 = b - a, c - b, d - c
    cross = lambda u, v: (u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                          u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0])
    n1, n2 = cross(b1, b2), cross(b2, b3)
    x = (n1[0] * n2[0] + n1[1] * n2[1]) + n1[2] * n2[2]
    y = np.sqrt((b2[..., 0] * b2[..., 0] + b2[..., 1] * b2[..., 1]) + b2[..., 2] * b2[..., 2]) * \
        ((b1[..., 0] * n2[0] + b1[..., 1] * n2[1]) + b1[..., 2] * n2[2])
    return x, y


def _measure(x, mask, aa, chain, residx, th, chi_atoms, near):
    """The seven (x, y) pairs of every row of ONE structure, which of them are defined, and its ABEGO codes.  x (Lab,14,3) float64, mask
    (Lab,14) bool -> X, Y (Lab,7) float64, has (Lab,7) bool, code (Lab) int64."""
    Lab = x.shape[0]
    have = mask[:, 0] & mask[:, 1] & mask[:, 2]
    link = np.zeros(Lab + 1, bool)                                              # link[i]: the link (i-1, i)
    if Lab > 1:
        link[1:Lab] = have[:-1] & have[1:] & (chain[1:] == chain[:-1]) & (True if residx is None else residx[1:] == residx[:-1] + 1)
    X, Y, has = np.zeros((Lab, 7)), np.zeros((Lab, 7)), np.zeros((Lab, 7), bool)
    N, CA, C = x[:, 0], x[:, 1], x[:, 2]
    prev = lambda v: np.concatenate([v[:1], v[:-1]])
    nxt = lambda v: np.concatenate([v[1:], v[-1:]])
    for k, quad in enumerate(((prev(C), N, CA, C), (N, CA, C, nxt(N)), (prev(CA), prev(C), N, CA))):
        ok = link[1:] if k == 1 else link[:-1]
        xv, yv = dihedral_xy(*quad)
        X[:, k], Y[:, k], has[:, k] = np.where(ok, xv, 0.0), np.where(ok, yv, 0.0), ok
    for k in range(4):
        sl = chi_atoms[aa, k]                                                   # (Lab,4)
        ok = (sl >= 0).all(1)
        q = np.where(sl >= 0, sl, 0)
        ok &= np.take_along_axis(mask, q, 1).all(1)
        p = [x[np.arange(Lab), q[:, j]] for j in range(4)]
        xv, yv = dihedral_xy(*p)
        X[:, 3 + k], Y[:, 3 + k], has[:, 3 + k] = np.where(ok, xv, 0.0), np.where(ok, yv, 0.0), ok
    code = _classify(X, Y, has, th, near)
    return X, Y, has, code


def torsions_host(x, mask, aa, gt_x, gt_mask, gt_aa, Lab, chain_id, residx=None, region=None, res_mask=None, chi_tol=40.0, mistake=None):
    """abx_torsion_scores for ONE structure on the host, with the same IEEE operations in the same order (numpy multiplies and adds in
    separate passes) and the (cos, sin) pairs of `thresholds`.  x (>=Lab,14,3) the design's coordinates (rounded to float32 first: what
    the kernel reads), mask (>=Lab,14) its atoms, aa (>=Lab) its tokens; gt_x, gt_mask, gt_aa the same of the wild type; chain_id,
    residx, region, res_mask (>=Lab) or None.  Only the first Lab rows are read.
    -> dict(row (len(TORSIONS_COLUMNS),) float64, rows (Lab,8) float64 ROW_COLUMNS, classes (Lab) int32, wild_classes (Lab) int32,
            n_borderline: the decisions whose two sides differ by less than 1e-9 relative - those a device evaluation could take
            differently).
    mistake: None, or the name of a deliberate error the tests show a column for - 'atan2_swapped', 'phi_next', 'omega_following',
    'chain_linked', 'chi_unfolded', 'gly_phi_pos'."""
    Lab = int(Lab)
    keep = np.ones(Lab, bool) if res_mask is None else (to_np(res_mask)[:Lab] != 0)
    xd = to_np(x)[:Lab].astype(np.float32).astype(np.float64)
    xw = to_np(gt_x)[:Lab].astype(np.float32).astype(np.float64)
    md, mw = (to_np(mask)[:Lab] != 0) & keep[:, None], (to_np(gt_mask)[:Lab] != 0) & keep[:, None]
    aa_d, aa_w = (np.where((t < 0) | (t > 20), 20, t) for t in (to_np(aa)[:Lab].astype(np.int64), to_np(gt_aa)[:Lab].astype(np.int64)))
    chain = to_np(chain_id)[:Lab].astype(np.int64)
    if mistake == 'chain_linked':
        chain = np.zeros_like(chain)
    rsx = None if residx is None else to_np(residx)[:Lab].astype(np.int64)
    if mistake == 'chain_linked' and rsx is not None:
        rsx = np.arange(Lab)
    reg = np.zeros(Lab, bool) if region is None else ((to_np(region)[:Lab] != 0) & keep)
    th = thresholds(chi_tol)
    chi_atoms, chi_pi = chi_table()
    gly, pro = type_index('G'), type_index('P')
    near = _Borderline()
    Xw, Yw, hw, cw = _measure(xw, mw, aa_w, chain, rsx, th, chi_atoms, near)
    Xd, Yd, hd, cd = _measure(xd, md, aa_d, chain, rsx, th, chi_atoms, near)
    if mistake == 'atan2_swapped':
        (Xw, Yw), (Xd, Yd) = (Yw, Xw), (Yd, Xd)
        cw, cd = (_classify(X, Y, h, th) for X, Y, h in ((Xw, Yw, hw), (Xd, Yd, hd)))
    if mistake == 'phi_next':                           # phi of row i taken from row i + 1
        shift = lambda v: np.concatenate([v[1:, 0], v[-1:, 0]])
        for X, Y, h in ((Xw, Yw, hw), (Xd, Yd, hd)):
            X[:, 0], Y[:, 0], h[:, 0] = shift(X), shift(Y), shift(h)
        cw, cd = (_classify(X, Y, h, th) for X, Y, h in ((Xw, Yw, hw), (Xd, Yd, hd)))
    if mistake == 'omega_following':                    # omega of row i taken from the link (i, i + 1)
        shift = lambda v: np.concatenate([v[1:, 2], np.zeros(1, v.dtype)])
        for X, Y, h in ((Xw, Yw, hw), (Xd, Yd, hd)):
            X[:, 2], Y[:, 2], h[:, 2] = shift(X), shift(Y), shift(h)
        cw, cd = (_classify(X, Y, h, th) for X, Y, h in ((Xw, Yw, hw), (Xd, Yd, hd)))
    R = np.sqrt(Xd * Xd + Yd * Yd)
    # omega
    has_o = hd[:, 2]
    wide = Xd[:, 2] <= th['cis'][0] * R[:, 2]
    wider = Xd[:, 2] <= th['trans'][0] * R[:, 2]
    cis, tw = has_o & ~wide, has_o & wide & ~wider
    near(Xd[:, 2], th['cis'][0] * R[:, 2], R[:, 2], has_o)
    near(Xd[:, 2], th['trans'][0] * R[:, 2], R[:, 2], has_o & wide)
    reg_link = reg | np.concatenate([[False], reg[:-1]])
    # phi
    phi_pos = hd[:, 0] & ~(Yd[:, 0] < 0.0) & ((aa_d != gly) | (mistake == 'gly_phi_pos'))
    near(Yd[:, 0], 0.0, R[:, 0], hd[:, 0] & ((aa_d != gly) | (mistake == 'gly_phi_pos')))
    # differences
    both = hd & hw
    cc = Xd * Xw + Yd * Yw
    ss = Yd * Xw - Xd * Yw
    fold = np.zeros((Lab, 7), bool)
    if mistake != 'chi_unfolded':
        fold[:, 3:] = chi_pi[aa_d] != 0
    cc = np.where(fold, np.abs(cc), cc)
    rr = np.sqrt(cc * cc + ss * ss)
    ok = cc >= th['chi_tol'][0] * rr
    delta = np.arctan2(np.abs(ss), cc) * DEG
    same = reg & (aa_d == aa_w)
    cmp_bb = both[:, :3] & reg[:, None]
    cmp_chi = both[:, 3:] & same[:, None]
    near(cc[:, 3:5], (th['chi_tol'][0] * rr)[:, 3:5], rr[:, 3:5], cmp_chi[:, :2])
    ok1, ok2 = cmp_chi[:, 0] & ok[:, 3], cmp_chi[:, 1] & ok[:, 4]
    mean = lambda v, m: float(v[m].sum()) / float(m.sum()) if m.any() else np.nan
    row = np.full(len(TORSIONS_COLUMNS), np.nan)
    row[0:4] = has_o.sum(), cis.sum(), (cis & (aa_d != pro)).sum(), tw.sum()
    row[4:7] = (has_o & reg_link).sum(), (cis & reg_link).sum(), (tw & reg_link).sum()
    row[7:9] = phi_pos.sum(), (phi_pos & reg).sum()
    for k in range(5):
        row[9 + k] = ((cd == 1 + k) & reg).sum()
    defined = reg & (cd != 0) & (cw != 0)
    row[14], row[15] = defined.sum(), (defined & (cd == cw)).sum()
    row[16], row[17], row[18] = (mean(delta[:, k], cmp_bb[:, k]) for k in range(3))
    bb2 = cmp_bb[:, :2]
    row[19] = float(delta[:, :2][bb2].max()) if bb2.any() else np.nan
    row[20], row[21] = cmp_chi[:, 0].sum(), ok1.sum()
    c12 = cmp_chi[:, 0] & cmp_chi[:, 1]
    row[22], row[23] = c12.sum(), (c12 & ok1 & ok2).sum()
    row[24] = mean(delta[:, 3:], cmp_chi)
    rows = np.full((Lab, 8), np.nan)
    ang = np.arctan2(Yd, Xd) * DEG
    rows[:, :7] = np.where(hd, ang, np.nan)
    flags = cd | np.where(cis, F_CIS, 0) | np.where(tw, F_TWISTED, 0) | np.where(phi_pos, F_PHI_POS, 0) | np.where(reg, F_REGION, 0) | \
        np.where(cmp_chi[:, 0], F_CHI1, 0) | np.where(ok1, F_CHI1_OK, 0)
    rows[:, 7] = flags
    return dict(row=row, rows=rows, classes=cd.astype(np.int32), wild_classes=cw.astype(np.int32), n_borderline=near.n)


def _classify(X, Y, has, th, near=None):
    """The ABEGO codes of measured pairs, csrc/torsions.hip::code_of operation for operation; near: a _Borderline that counts the
    decisions taken here (None for the deliberate mistakes of torsions_host, which re-classify after moving a column)."""
    R = np.sqrt(X * X + Y * Y)
    full = has[:, 0] & has[:, 1] & has[:, 2]
    o_lhs, o_rhs = X[:, 2], th['o'][0] * R[:, 2]
    a_lhs, a_rhs = X[:, 1] * th['a_mid'][0] + Y[:, 1] * th['a_mid'][1], th['a_half'][0] * R[:, 1]
    g_lhs, g_rhs = X[:, 1], th['g_half'][0] * R[:, 1]
    is_o = ~(o_lhs <= o_rhs)
    neg = Y[:, 0] < 0.0
    if near is not None:
        near(o_lhs, o_rhs, R[:, 2], full)
        near(Y[:, 0], 0.0, R[:, 0], full & ~is_o)
        near(a_lhs, a_rhs, R[:, 1], full & ~is_o & neg)
        near(g_lhs, g_rhs, R[:, 1], full & ~is_o & ~neg)
    return np.where(full, np.where(is_o, 5, np.where(neg, np.where(a_lhs >= a_rhs, 1, 2), np.where(g_lhs >= g_rhs, 3, 4))), 0).astype(np.int64)
