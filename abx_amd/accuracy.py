"""Accuracy of designs against the crystal structure of the complex: how close a design is to the structure it was made from, beyond
the per-CDR C-alpha RMSD of abx_amd.metrics.

  lDDT       upstream's `lddt` (abx/model/utils.py:102-155; Mariani et al. 2013), the training target of predicted_lddt_loss: the
             quantity the reported pLDDT predicts.  Three classes in one walk over the atom pairs: all scored atoms, backbone + CB, and
             the C-alpha (class `ca` IS upstream's lddt on the C-alpha atoms), per residue and pair-pooled over row sets, plus the
             calibration of the per-residue pLDDT against 100 * lDDT-C-alpha.
  TM block   upstream's TMscoreHead (abx/model/head.py:116-141: Kabsch, TMscore, GDT of abx/utils.py:562-578, 525-560, 703-763), the
             head the network build loads around and never evaluates: TM-score, GDT-TS, GDT-HA and RMSD of the C-alpha after the
             optimal proper rotation.
  contacts   the native antibody-antigen residue contacts that survive in the design (DockQ's Fnat), and the new ones.

Scored atoms: a slot that exists in the wild type and in the design; a mutated residue is compared on N, CA, C, O, CB only.  Atoms
related by a side-chain symmetry (Asp OD1 / OD2, Glu OE1 / OE2, the Phe / Tyr ring, Arg NH1 / NH2, ...) are NOT renamed: a flipped
ring counts as a deviation.  The definitions, operation by operation: include/abx_hip.h, AbxAccuracyArgs.

Every decision is taken in float64 from the float32 coordinates in a fixed IEEE operation order, so the counts of the device
(`AccuracyScorer`, abx_accuracy_scores, csrc/accuracy.hip) and of the host twin (`accuracy_host`, numpy) are equal integers unless a
pair sits on a threshold, which the twin counts (`n_borderline`, `n_borderline_gdt`)."""
import functools

import numpy as np

from . import complex_view
from .complex_view import to_np

# The row of abx_accuracy_scores (include/abx_hip.h, ABX_ACC_COLS)
ACCURACY_COLUMNS = ('lddt_all', 'lddt_antibody', 'lddt_region', 'lddt_bb_region', 'lddt_ca_all', 'lddt_ca_region', 'plddt_region',
                    'plddt_err_region', 'tm_score', 'gdt_ts', 'gdt_ha', 'rmsd_ca', 'n_native', 'n_kept', 'fnat', 'n_new',
                    'n_native_region', 'n_kept_region', 'fnat_region', 'n_pairs_region', 'n_atoms_scored')
COUNT_COLUMNS = tuple(c for c in ACCURACY_COLUMNS if c.startswith('n_'))
# relaxed structure minus design: the columns the driver writes a difference for under --relax
DELTA_COLUMNS = ('lddt_region', 'lddt_bb_region', 'rmsd_ca', 'n_kept')
# the optional per-residue output `rows`
ROW_COLUMNS = ('lddt_all', 'lddt_bb', 'lddt_ca', 'n_pairs')
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
GDT_CUTOFFS = (0.5, 1.0, 2.0, 4.0, 8.0)
_PLACES = {'plddt_region': 2, 'plddt_err_region': 2, 'rmsd_ca': 3, None: 4}


# format_accuracy(row): integers for the counts, %.2f for the pLDDT columns, %.3f for the RMSD (Angstrom), %.4f for the scores;
# format_delta(row, base): row minus base for DELTA_COLUMNS, signed, at the same precision
format_accuracy = functools.partial(complex_view.format_row, ACCURACY_COLUMNS, COUNT_COLUMNS, _PLACES)
format_delta = functools.partial(complex_view.format_delta, ACCURACY_COLUMNS, COUNT_COLUMNS, DELTA_COLUMNS, _PLACES)


class AccuracyScorer(complex_view.ComplexView):
    """Accuracy rows of batches of designs of ONE complex on the device.  Built once per complex from its featurised batch (or the
    un-batched complex) like interface.InterfaceScorer.  region: (L) mask of the designed rows the `*_region` columns describe
    (default: the rows the sampler diffuses, sample 0's (1 - fixed_mask) * backbone mask).  radius: lDDT inclusion radius; contact:
    heavy-atom distance of a residue contact (Angstrom)."""

    COLUMNS = ACCURACY_COLUMNS

    def __init__(self, batch, region=None, radius=15.0, contact=5.0):
        super().__init__(batch)
        self.region = complex_view.region_mask(batch, region, self.gt_atom14.device)
        self.kw = dict(radius=float(radius), contact=float(contact))

    def score(self, atom14, seq, plddt=None, out=None, rows=False, counts=False, contacts=False, mask=None):
        """atom14 (B, Lab or L, 14, 3) f32 predicted coordinates (antibody only: the antigen is the ground truth's), seq (B, Lab) tokens,
        plddt (B, L) per-residue pLDDT of the call that produced them or None -> (B, len(ACCURACY_COLUMNS)) float64 on the device; out:
        rows to write into (any row stride).  With any of rows / counts / contacts: a tuple (table, rows (B,L,4) float64, counts
        (B,L,3,5) int32, contacts (B,Lab,L-Lab) uint8) with None for what was not asked for.  One call of abx_accuracy_scores, no host
        synchronisation."""
        import torch
        from abx_amd import ops
        B, dev = atom14.shape[0], atom14.device
        r = torch.empty(B, self.L, 4, dtype=torch.float64, device=dev) if rows else None
        c = torch.empty(B, self.L, 3, 5, dtype=torch.int32, device=dev) if counts else None
        k = torch.empty(B, self.Lab, self.L - self.Lab, dtype=torch.uint8, device=dev) if contacts else None
        table = ops.accuracy_scores(atom14, seq, self.gt_atom14, self.gt_seq, self.gt_exists, Lab=self.Lab, region=self.region, mask=mask,
                                    res_mask=self.res_mask, plddt=plddt, out=out, rows=r, counts=c, contacts=k, **self.kw)
        return (table, r, c, k) if (rows or counts or contacts) else table

    def record(self, rec, key, atom14, seq, design=True, plddt=None, **context):
        """ComplexView.record: 'accuracy' - lDDT, TM-score / GDT and native-contact recovery against the crystal structure, and the
        calibration of the per-residue pLDDT of the last network call (before it is averaged into the record's 'pLDDT') -, for the designs
        'accuracy_rows' (B, L, 4) per residue, and with a relaxer 'accuracy_relaxed'.  Two launches per table."""
        if design:
            rec[key], rec[key + '_rows'] = self.score(atom14, seq, plddt=plddt, rows=True)[:2]
        else:
            rec[key] = self.score(atom14, seq, plddt=plddt)

    # wild(**kw): the crystal structure against itself - every lDDT 1, fnat 1, rmsd_ca 0, the pLDDT columns nan: the first line of the
    # driver's table and the check that the conventions line up


# -------------------------------------------------------------------------------------------------------------------
# host twin (float64, numpy)
# -------------------------------------------------------------------------------------------------------------------
def _jacobi4(A):
    """csrc/accuracy.hip::jacobi4, operation for operation: eigen-decomposition of a symmetric 4x4 matrix by cyclic Jacobi rotations.
    -> (A rotated to diagonal form, V eigenvectors in columns)."""
    A = [[float(A[i][j]) for j in range(4)] for i in range(4)]
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(24):
        off = al = 0.0
        for i in range(4):
            for j in range(4):
                al += A[i][j] * A[i][j]
                if i < j:
                    off += A[i][j] * A[i][j]
        if off <= 1e-36 * al:
            break
        for p in range(3):
            for q in range(p + 1, 4):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                sn = t * c
                for k in range(4):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p] = c * akp - sn * akq
                    A[k][q] = sn * akp + c * akq
                for k in range(4):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k] = c * apk - sn * aqk
                    A[q][k] = sn * apk + c * aqk
                A[p][q] = A[q][p] = 0.0
                for k in range(4):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - sn * vkq
                    V[k][q] = sn * vkp + c * vkq
    return A, V


def tm_block_host(g, p):
    """The TM block of the kernel for the C-alpha sets g (wild type) and p (design), (N,3) float64 in row order.
    -> (tm_score, gdt_ts, gdt_ha, rmsd_ca, d (N) distances after the superposition); nan without points."""
    N = g.shape[0]
    if N == 0:
        return np.nan, np.nan, np.nan, np.nan, np.zeros(0)
    g = g - g.sum(0) / float(N)
    p = p - p.sum(0) / float(N)
    S = g.T @ p                                                                 # S[j][k] = sum g_j p_k
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S.tolist()
    Nm = [[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx], [0, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
          [0, 0, -Sxx + Syy - Szz, Syz + Szy], [0, 0, 0, -Sxx - Syy + Szz]]
    for i in range(1, 4):
        for j in range(i):
            Nm[i][j] = Nm[j][i]
    A, V = _jacobi4(Nm)
    im = 0
    for i in range(1, 4):
        if A[i][i] > A[im][im]:
            im = i
    q = np.array([V[k][im] for k in range(4)])
    qw, qx, qy, qz = (q / np.sqrt((q * q).sum())).tolist()
    R = np.array([[1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)],
                  [2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx)],
                  [2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)]])
    e = g @ R.T - p
    d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    d = np.sqrt(d2)
    d0 = 1.24 * np.cbrt(float(max(21, N)) - 15.0) - 1.8
    tm = (1.0 / (1.0 + (d / d0) * (d / d0))).sum() / float(N)
    n = [float((d <= c).sum()) for c in GDT_CUTOFFS]
    ts = ((n[1] + n[2]) + (n[3] + n[4])) / (4.0 * N)
    ha = ((n[0] + n[1]) + (n[2] + n[3])) / (4.0 * N)
    return tm, ts, ha, float(np.sqrt(d2.sum() / float(N))), d


def accuracy_host(x, mask, aa, gt_x, gt_mask, gt_aa, Lab, region=None, res_mask=None, plddt=None, radius=15.0, contact=5.0, chunk=32):
    """abx_accuracy_scores for ONE structure on the host, with the same IEEE operations in the same order (no fused multiply-add: numpy
    multiplies and adds in separate passes).  x (L,14,3) the design's coordinates with the antigen rows filled in (rounded to float32
    first: what the kernel reads), mask (L,14) its atoms, aa (L) its tokens; gt_x, gt_mask, gt_aa the same of the wild type; Lab =
    antibody rows; region (L) / res_mask (L) / plddt (L) or None.
    -> dict(row (len(ACCURACY_COLUMNS),) float64, rows (L,4) float64, counts (L,3,5) int32, contacts (Lab,L-Lab) uint8,
            n_borderline: atom pairs whose |d_wild - radius|, ||d_wild - d_design| - t| or |d^2 - contact^2| is <= 1e-9,
            n_borderline_gdt: C-alpha whose distance after the superposition lies within 1e-6 of a GDT cutoff)
    - the decisions a device evaluation may legitimately take differently.  The pair walk runs over `chunk` row residues at a time."""
    xd = to_np(x).astype(np.float32).astype(np.float64)
    xw = to_np(gt_x).astype(np.float32).astype(np.float64)
    L = xd.shape[0]
    Lab = int(Lab)
    keep = np.ones(L, bool) if res_mask is None else (to_np(res_mask) != 0)
    we = (to_np(gt_mask) != 0) & keep[:, None]
    de = (to_np(mask) != 0) & keep[:, None]
    aa_d, aa_w = (np.where((t < 0) | (t > 20), 20, t) for t in (to_np(aa).astype(np.int64), to_np(gt_aa).astype(np.int64)))
    sc = we & de & ((aa_d == aa_w)[:, None] | (np.arange(14) <= 4)[None])
    region = np.zeros(L, bool) if region is None else ((to_np(region) != 0) & keep)
    radius, contact = float(radius), float(contact)
    r2, c2 = radius * radius, contact * contact
    res, slot = np.repeat(np.arange(L), 14), np.tile(np.arange(14), L)
    XW, XD, scf, wef, def_ = xw.reshape(-1, 3), xd.reshape(-1, 3), sc.reshape(-1), we.reshape(-1), de.reshape(-1)
    counts = np.zeros((L, 3, 5), np.int64)
    cw, cd = np.zeros((Lab, L - Lab), bool), np.zeros((Lab, L - Lab), bool)
    nb = 0
    T = np.array(THRESHOLDS)

    def dist2(X, rows, cols):
        dx, dy, dz = (X[rows, None, k] - X[None, cols, k] for k in range(3))
        return (dx * dx + dy * dy) + dz * dz

    everyone, antigen = slice(None), slice(Lab * 14, None)
    for r0 in range(0, L, int(chunk)):
        rows = np.arange(r0 * 14, min(L, r0 + int(chunk)) * 14)
        rres, rslot = res[rows], slot[rows]
        d2w = dist2(XW, rows, everyone)
        cand = scf[rows, None] & scf[None] & (rres[:, None] != res[None])
        near = cand & (np.abs(d2w - r2) <= 4e-9 * (radius + 1.0))
        nb += int((np.abs(np.sqrt(d2w[near]) - radius) <= 1e-9).sum())
        ia, ib = np.nonzero(cand & (d2w < r2))
        ex, ey, ez = (XD[rows[ia], k] - XD[ib, k] for k in range(3))              # the design's distance of the included pairs only
        diff = np.abs(np.sqrt(d2w[ia, ib]) - np.sqrt((ex * ex + ey * ey) + ez * ez))
        nb += int((np.abs(diff[:, None] - T[None]) <= 1e-9).any(1).sum())
        pr, sa, sb = rres[ia], rslot[ia], slot[ib]
        for q, m in enumerate((np.ones(len(ia), bool), (sa <= 4) & (sb <= 4), (sa == 1) & (sb == 1))):
            counts[:, q, 0] += np.bincount(pr[m], minlength=L)
            for k, t in enumerate(THRESHOLDS):
                counts[:, q, 1 + k] += np.bincount(pr[m & (diff < t)], minlength=L)
        if r0 < Lab < L:
            side_a = (rres < Lab)[:, None]
            for has, d2, plane in ((wef, d2w[:, antigen], cw), (def_, dist2(XD, rows, antigen), cd)):
                both = side_a & has[rows, None] & has[None, antigen]
                nb += int((both & (np.abs(d2 - c2) <= 1e-9)).sum())
                ia, ib = np.nonzero(both & (d2 < c2))
                plane[rres[ia], res[antigen][ib] - Lab] = True
    pres = counts[:, :, 1:].sum(2).astype(np.float64)
    npairs = counts[:, :, 0].astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        per_res = np.where(npairs > 0, pres / (4.0 * npairs), np.nan)              # (L,3)
    ratio = lambda num, den: float(num) / float(den) if den > 0 else np.nan
    pooled = lambda rows_, q: ratio(pres[rows_, q].sum(), 4.0 * npairs[rows_, q].sum())
    everything, antibody = np.ones(L, bool), np.arange(L) < Lab
    row = np.full(len(ACCURACY_COLUMNS), np.nan)
    row[0], row[1], row[2], row[3] = pooled(everything, 0), pooled(antibody, 0), pooled(region, 0), pooled(region, 1)
    row[4], row[5] = pooled(everything, 2), pooled(region, 2)
    if plddt is not None:
        pl = to_np(plddt).astype(np.float32).astype(np.float64)
        row[6] = ratio(pl[region].sum(), region.sum())
        has = region & (counts[:, 2, 0] > 0)
        row[7] = ratio(np.abs(pl[has] - 100.0 * per_res[has, 2]).sum(), has.sum())
    ca = we[:, 1]
    tm, ts, ha, rmsd, d = tm_block_host(xw[ca, 1], xd[ca, 1])
    row[8], row[9], row[10], row[11] = tm, ts, ha, rmsd
    native, kept, new = cw.sum(1), (cw & cd).sum(1), (cd & ~cw).sum(1)
    reg_ab = region[:Lab]
    row[12], row[13], row[14], row[15] = native.sum(), kept.sum(), ratio(kept.sum(), native.sum()), new.sum()
    row[16], row[17], row[18] = native[reg_ab].sum(), kept[reg_ab].sum(), ratio(kept[reg_ab].sum(), native[reg_ab].sum())
    row[19], row[20] = npairs[region, 0].sum(), sc.sum()
    rows_out = np.concatenate([per_res, npairs[:, :1]], axis=1)
    nb_gdt = int((np.abs(d[:, None] - np.array(GDT_CUTOFFS)[None]) <= 1e-6).any(1).sum()) if d.size else 0
    return dict(row=row, rows=rows_out, counts=counts.astype(np.int32), contacts=(cw.astype(np.uint8) | (cd.astype(np.uint8) << 1)),
                n_borderline=nb, n_borderline_gdt=nb_gdt)
