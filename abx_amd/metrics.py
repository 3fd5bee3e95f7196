"""Design-quality metrics of the reference's offline evaluation (abx/common/ab_utils.py:124-167 `calc_ab_metrics`,
abx/utils.py:444-465 `kabsch_numpy`): Kabsch-aligned C-alpha RMSD and amino-acid recovery per CDR.  numpy, host side.

On the device: `DesignScorer` (abx_design_scores, csrc/metrics.hip) scores a whole batch of designs of one complex where the sampler
left them - the columns of `calc_ab_metrics` plus the violation counts of eval/metric_scripts/cal_vio.py:29-110 and the number of
clashing atom pairs (`SCORE_COLUMNS`).  `violation_counts` / `clash_counts` are the host twins of the count columns (plain torch)."""
import functools
from collections import OrderedDict

import numpy as np

from . import complex_view

_SCHEMA = {'cdr1': 1, 'cdr2': 3, 'cdr3': 5}


def kabsch(X, Y):
    """Kabsch alignment of X onto Y, both (3, N): returns the centred + rotated X and the centred Y (abx/utils.py:444-465)."""
    X_ = X - X.mean(axis=-1, keepdims=True)
    Y_ = Y - Y.mean(axis=-1, keepdims=True)
    C = np.dot(X_, Y_.transpose())
    V, S, W = np.linalg.svd(C)
    if (np.linalg.det(V) * np.linalg.det(W)) < 0.0:
        S[-1] = -S[-1]
        V[:, -1] = -V[:, -1]
    U = np.dot(V, W)
    return np.dot(X_.T, U).T, Y_


def _rmsd(A, B):
    return float(np.sqrt(np.mean(np.sum(np.square(A - B), axis=0))))


def calc_ab_metrics(gt_coord, pred_coord, cdr_def, gt_str_seq=None, pred_str_seq=None):
    """gt_coord / pred_coord (N, 3) C-alpha coordinates of the antibody, cdr_def (N,) IMGT region codes (H: 0..6, L: 7..13).
    -> OrderedDict {heavy|light}_cdr{1,2,3}_{AAR,RMSD} (+ *_cdr3_Loop_* on residues [4:-2] of CDR-H3), as ab_utils.py:124-167."""
    gt_al, pred_al = kabsch(np.transpose(gt_coord, [1, 0]), np.transpose(pred_coord, [1, 0]))
    cdr_def = np.asarray(cdr_def)
    names = {v: 'heavy_' + k for k, v in _SCHEMA.items()}
    names.update({v + 7: 'light_' + k for k, v in _SCHEMA.items()})
    ret = OrderedDict()
    for k, v in names.items():
        idx = cdr_def == k
        gt, pred = gt_al[:, idx], pred_al[:, idx]
        if gt_str_seq is not None:
            gs = ''.join(c for c, keep in zip(gt_str_seq, idx) if keep)
            ps = ''.join(c for c, keep in zip(pred_str_seq, idx) if keep)
            ret[v + '_AAR'] = float(np.mean([a == b for a, b in zip(gs, ps)]))
            if k == 5:
                ret[v + '_Loop_AAR'] = float(np.mean([a == b for a, b in zip(gs[4:-2], ps[4:-2])]))
        ret[v + '_RMSD'] = _rmsd(gt, pred)
        if k == 5:
            ret[v + '_Loop_RMSD'] = _rmsd(gt[:, 4:-2], pred[:, 4:-2])
    return ret


# The row of abx_design_scores (include/abx_hip.h, ABX_SCORE_COLS): the keys of calc_ab_metrics in its order, then the counts
SCORE_COLUMNS = ('heavy_cdr1_AAR', 'heavy_cdr1_RMSD', 'heavy_cdr2_AAR', 'heavy_cdr2_RMSD', 'heavy_cdr3_AAR', 'heavy_cdr3_Loop_AAR',
                 'heavy_cdr3_RMSD', 'heavy_cdr3_Loop_RMSD', 'light_cdr1_AAR', 'light_cdr1_RMSD', 'light_cdr2_AAR', 'light_cdr2_RMSD',
                 'light_cdr3_AAR', 'light_cdr3_RMSD', 'n_viol_c_n', 'n_viol_ca_c_n', 'n_viol_c_n_ca', 'n_clash', 'n_clash_inter')
COUNT_COLUMNS = tuple(c for c in SCORE_COLUMNS if c.startswith('n_'))


# format_scores(row): %.4f for RMSD / AAR (nan for a region without residues), integers for the counts
format_scores = functools.partial(complex_view.format_row, SCORE_COLUMNS, COUNT_COLUMNS, 4)


class DesignScorer(complex_view.ComplexView):
    """Scores batches of designs of ONE complex on the device.  Built once per complex from its featurised batch (or the un-batched
    complex): ground-truth atom14 / tokens / masks, cdr_def, chain ids, residue numbers, Lab = the antibody length.
    link_by_residx: array neighbours are peptide-bonded only with consecutive residue numbers (the guidance default; False: the
    chain-only rule of cal_vio.py:50)."""

    COLUMNS = SCORE_COLUMNS

    def __init__(self, batch, link_by_residx=True, overlap_tolerance=1.5, bond_tolerance_factor=12.0):
        super().__init__(batch, chains=True, link_by_residx=link_by_residx, cdr=True)
        self.kw = dict(overlap_tolerance=float(overlap_tolerance), bond_tolerance_factor=float(bond_tolerance_factor))

    def score(self, atom14, seq, out=None):
        """atom14 (B, Lab or L, 14, 3) f32 predicted coordinates (antibody only: the antigen is the ground truth's), seq (B, Lab) tokens
        -> (B, len(SCORE_COLUMNS)) float64 on the device; out: rows to write into (any row stride).  One call of abx_design_scores,
        no host synchronisation."""
        from abx_amd import ops
        return ops.design_scores(atom14, seq, self.gt_atom14, self.gt_seq, self.gt_exists, self.cdr_def, self.chain_id, Lab=self.Lab,
                                 residx=self.residx, res_mask=self.res_mask, out=out, **self.kw)


def violation_counts(atom14, atom_mask, aatype, chain_id, residx=None, tolerance_factor=12.0):
    """Host twin of the n_viol_* columns: the sums of the three violation masks of between_residue_bond_loss
    (eval/metric_scripts/cal_vio.py:74-75, 93-94, 107-108) in its float32 arithmetic.  atom14 (B,L,14,3), atom_mask (B,L,14),
    aatype (B,L), chain_id (B,L); residx (B,L) or None (None: the reference's chain-only link rule).  -> (B,3) int64 [C-N, CA-C-N, C-N-CA]."""
    import torch
    x = atom14.to(torch.float32)
    m = atom_mask.to(torch.float32)
    ca, c, n, ca2 = x[:, :-1, 1], x[:, :-1, 2], x[:, 1:, 0], x[:, 1:, 1]
    m_ca, m_c, m_n, m_ca2 = m[:, :-1, 1], m[:, :-1, 2], m[:, 1:, 0], m[:, 1:, 1]
    link = chain_id[:, 1:] == chain_id[:, :-1]
    if residx is not None:
        link = link & (residx[:, 1:] == residx[:, :-1] + 1)
    link = link.to(torch.float32)
    pro = (aatype[:, 1:] == 14).to(torch.float32)
    l0 = (1 - pro) * 1.329 + pro * 1.341
    sd = (1 - pro) * 0.014 + pro * 0.016
    err_b = torch.sqrt(1e-6 + (torch.sqrt(1e-6 + ((c - n) ** 2).sum(-1)) - l0) ** 2)
    unit = lambda v: v / torch.sqrt(torch.clamp((v ** 2).sum(-1, keepdim=True), min=1e-12))
    c_ca, c_n, n_ca = unit(ca - c), unit(n - c), unit(ca2 - n)
    err_a1 = torch.sqrt(1e-6 + ((c_ca * c_n).sum(-1) - (-0.4473)) ** 2)
    err_a2 = torch.sqrt(1e-6 + (((-c_n) * n_ca).sum(-1) - (-0.5203)) ** 2)
    t = float(tolerance_factor)
    v_b = m_c * m_n * link * (err_b > t * sd)
    v_a1 = m_ca * m_c * m_n * link * (err_a1 > t * 0.0311)
    v_a2 = m_c * m_n * m_ca2 * link * (err_a2 > t * 0.0353)
    return torch.stack([v_b.sum(1), v_a1.sum(1), v_a2.sum(1)], dim=1).to(torch.int64)


def clash_counts(atom14, atom_mask, aatype, chain_id, residx=None, overlap_tolerance=1.5, margin=1e-4):
    """Host twin of n_clash / n_clash_inter in float64: atom pairs of different residues, each once, with
    d < r_a + r_b - overlap_tolerance, without the peptide bond C(i)-N(i+1) of linked neighbours and SG-SG (the pair rules of the clash
    energy of abx_clash_grad).  -> (n_clash, n_clash_inter, n_borderline), each (B,) int64; n_borderline = candidate pairs within
    `margin` of their bound, i.e. those a float32 evaluation may count differently."""
    import torch
    from abx_amd import ops
    B, L = aatype.shape
    aa = torch.clamp(aatype.long(), 0, 20)
    rad_t = ops.vdw_radius_table('cpu').double()                                # the float32 radii the kernel reads
    res = torch.arange(L).repeat_interleave(14)
    slot = torch.arange(14).repeat(L)
    link = chain_id[:, 1:] == chain_id[:, :-1]
    if residx is not None:
        link = link & (residx[:, 1:] == residx[:, :-1] + 1)
    out = torch.zeros(3, B, dtype=torch.int64)
    for b in range(B):
        x = atom14[b].double().reshape(L * 14, 3)
        rad = rad_t[aa[b]].reshape(L * 14)
        ok = atom_mask[b].reshape(L * 14).bool() & (rad > 0)
        ch = chain_id[b].long().repeat_interleave(14)
        sg = (aa[b] == 4).repeat_interleave(14) & (slot == 5)
        linked = torch.zeros(L, dtype=torch.bool)                               # residue is linked to its array predecessor
        linked[1:] = link[b]
        lk = linked.repeat_interleave(14)
        pair = ok[:, None] & ok[None] & (res[:, None] < res[None])
        bonded = lk[None] & (res[None] == res[:, None] + 1) & (slot[:, None] == 2) & (slot[None] == 0)
        pair = pair & ~bonded & ~(sg[:, None] & sg[None])
        d = torch.sqrt(1e-10 + ((x[:, None] - x[None]) ** 2).sum(-1))
        ov = rad[:, None] + rad[None] - overlap_tolerance - d
        hit = pair & (ov > 0)
        out[0, b] = hit.sum()
        out[1, b] = (hit & (ch[:, None] != ch[None])).sum()
        out[2, b] = (pair & (ov.abs() <= margin)).sum()
    return out[0], out[1], out[2]
