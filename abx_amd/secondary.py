"""Secondary structure of designs: what does the backbone do as a whole?  DSSP (Kabsch & Sander 1983) over the antibody rows - the
electrostatic N-H...O=C energy between every pair of residues on a virtual hydrogen, and from the bonds the turns, helices, bridges,
ladders and bends - as counts, as agreement with the crystal structure and as the state string of `ss_string`.

  bonds     hb(j -> i), C=O of j to N-H of i: e = 27.888 (1/d(N,O) + 1/d(H,C) - 1/d(H,O) - 1/d(N,C)) < hb_energy (-0.5 kcal/mol), the
            C-alpha atoms closer than 9 A; H = N + (C' - O') / |C' - O'| from the preceding residue, none for Pro or after a break.
  turns     turn_n(i), n = 3, 4, 5: hb(i -> i+n) over an unbroken stretch; two consecutive turns start a helix (H: n = 4, G: 3, I: 5).
  bridges   parallel and antiparallel pairs of rows (the two classic bond patterns each); a bridge with a neighbouring bridge of its
            type is laddered: E, a lone one B.
  bends     the C-alpha direction changes by more than 70 degrees over (i-2, i, i+2): S.
  states    '.HGIEBTS-' = 0..8 with the priority H, E / B, G, I, T, S; the three-state class: helix {H, G, I}, strand {E, B}, coil.

Declared limits: ALL bonds below the threshold are kept (mkdssp keeps the two best per residue); there is no beta-bulge merging of
ladders, so a bulge residue stays what it otherwise is; no sheet labels and no kappa / alpha / phi / psi columns; I has the classic
priority below G; the antigen is not read (cross-interface bonds are polar.py's); this is DSSP's electrostatic criterion on a virtual H,
not the heavy-atom rule of polar.py: the two bond counts are not expected to agree.

Every decision is a comparison of float64 expressions from the float32 coordinates in a fixed IEEE operation order (no operation
fused), so the counts, states and flags of the device (`SecondaryScorer`, abx_secondary_scores, csrc/secondary.hip) and of the host twin
(`secondary_host`, numpy) are equal; the one float column is a sum of rint(e * 2^20) in a 64-bit integer.  The definitions, operation by
operation: include/abx_hip.h, AbxSecondaryArgs."""
import functools

import numpy as np

from . import complex_view
from .complex_view import Borderline as _Borderline, to_np, type_index

# The row of abx_secondary_scores (include/abx_hip.h, ABX_SECONDARY_COLS)
SECONDARY_COLUMNS = ('n_hb', 'n_hb_region', 'n_hb_inside', 'hb_wild_region', 'hb_kept_region', 'hb_energy_region', 'n_bridge_region',
                     'bridge_wild_region', 'bridge_kept_region', 'ss_H', 'ss_G', 'ss_I', 'ss_E', 'ss_B', 'ss_T', 'ss_S', 'ss_C', 'n_ss', 'q8_same',
                     'q3_same', 'strand_ab', 'helix_ab')
MEAN_COLUMNS = ('hb_energy_region',)
COUNT_COLUMNS = tuple(c for c in SECONDARY_COLUMNS if c not in MEAN_COLUMNS)
# design minus wild type: the columns the driver writes a difference for
DELTA_COLUMNS = ('n_hb_region', 'n_hb_inside', 'hb_energy_region', 'n_bridge_region', 'ss_H', 'ss_G', 'ss_I', 'ss_E', 'ss_B', 'ss_T', 'ss_S',
                 'ss_C', 'strand_ab')
# the per-residue table of --secondary_rows (AbxSecondaryArgs.rows), int32
ROW_COLUMNS = ('state', 'donated', 'accepted', 'partner0', 'partner1', 'flags')
LETTERS = '.HGIEBTS-'                                   # the letter of a state; 0: the row is not present
ST_NONE, ST_H, ST_G, ST_I, ST_E, ST_B, ST_T, ST_S, ST_C = range(9)
CLASS3 = (0, 1, 1, 1, 2, 2, 3, 3, 3)                    # helix 1, strand 2, coil 3 of a state
F_REGION, F_PRESENT, F_HAS_H, F_PARALLEL, F_ANTIPARALLEL, F_BEND, F_TURN3, F_TURN4, F_TURN5 = 1, 2, 4, 8, 16, 32, 64, 128, 256
MAX_LAB = 800                                           # ABX_SECONDARY_MAX_LAB
BEND_DEGREES = 70.0
COULOMB = 27.888                                        # 332 * 0.42 * 0.20 kcal A / mol, the constant of csrc/secondary.hip
CA_CUTOFF2 = 81.0
MIN_DIST = 0.5
MIN_ENERGY = -9.9
FIXED = 1048576.0                                       # 2^20: the fixed point of hb_energy_region
MISTAKES = ('acceptor_donor_swapped', 'own_peptide_bond', 'pro_donates', 'h_from_own_row', 'chain_linked', 'parallel_as_antiparallel', 'g_over_h')
_PLACES = 2

format_secondary = functools.partial(complex_view.format_row, SECONDARY_COLUMNS, COUNT_COLUMNS, _PLACES)
format_delta = functools.partial(complex_view.format_delta, SECONDARY_COLUMNS, COUNT_COLUMNS, DELTA_COLUMNS, _PLACES)


def thresholds(hb_energy=-0.5):
    """dict(hb_energy, bend = (cos, sin) of 70 degrees) of AbxSecondaryArgs, float64: computed HERE for the device and for the twin."""
    hb_energy = float(hb_energy)
    if not (np.isfinite(hb_energy) and hb_energy < 0.0):
        raise ValueError(f'secondary: hb_energy must be a finite energy below 0 kcal/mol (got {hb_energy})')
    r = np.deg2rad(np.float64(BEND_DEGREES))
    return dict(hb_energy=hb_energy, bend=(float(np.cos(r)), float(np.sin(r))))


def ss_string(classes, region):
    """The state letters of the rows of `region` (a mask over the rows of `classes`, or longer)."""
    cl = np.asarray(classes).astype(np.int64)
    reg = np.asarray(region)[:cl.shape[0]] != 0
    return ''.join(LETTERS[int(v)] for v in cl[reg])


class SecondaryScorer(complex_view.ComplexView):
    """Secondary-structure rows of batches of designs of ONE complex on the device.  Built once per complex from its featurised batch
    (or the un-batched complex) like torsions.TorsionScorer.  region: (L) mask of the designed rows the `*_region` columns describe
    (default: the rows the sampler diffuses).  hb_energy: the energy below which a bond counts, kcal/mol, < 0."""

    COLUMNS = SECONDARY_COLUMNS

    def __init__(self, batch, region=None, hb_energy=-0.5):
        super().__init__(batch, chains=True)
        if self.Lab > MAX_LAB:
            raise ValueError(f'secondary: the antibody has {self.Lab} rows, abx_secondary_scores takes at most {MAX_LAB}')
        self.region = complex_view.region_mask(batch, region, self.gt_atom14.device)
        self.kw = dict(thresholds=thresholds(hb_energy), pro=type_index('P'))

    def new_rows(self, B):
        """An uninitialised (B, Lab, 6) int32 tensor for ROW_COLUMNS of B structures."""
        import torch
        return torch.empty(B, self.Lab, len(ROW_COLUMNS), dtype=torch.int32, device=self.region.device)

    def new_classes(self, B):
        """An uninitialised (B, Lab) int32 tensor for the states of B structures."""
        import torch
        return torch.empty(B, self.Lab, dtype=torch.int32, device=self.region.device)

    def score(self, atom14, seq, rows=None, classes=None, out=None, mask=None, workspace=None):
        """atom14 (B, Lab or L, 14, 3) f32 predicted coordinates (only the antibody rows are read), seq (B, Lab) tokens ->
        (B, len(SECONDARY_COLUMNS)) float64 on the device; out: rows to write into (any row stride); rows: (B,Lab,6) int32 to receive
        ROW_COLUMNS; classes: (B,Lab) int32 to receive the states; mask: (B,L,14) or None (the atoms of the tokens); workspace: a
        uint8 tensor of at least ops.secondary_workspace_bytes(B, Lab) bytes (None: allocated here).  One launch, no host synchronisation."""
        from abx_amd import ops
        return ops.secondary_scores(atom14, seq, self.gt_atom14, self.gt_seq, self.gt_exists, self.chain_id, self.residx, Lab=self.Lab,
                                    region=self.region, mask=mask, res_mask=self.res_mask, out=out, rows=rows, classes=classes,
                                    workspace=workspace, **self.kw)

    def side_outputs(self, B):
        """The record of the designs also carries 'secondary_classes' (B, Lab) int32, the states, and with want_rows 'secondary_rows'
        (B, Lab, 6) int32."""
        return dict({'rows': self.new_rows(B)} if self.want_rows else {}, classes=self.new_classes(B))

    # wild(**kw): the crystal structure against itself - hb_kept_region == hb_wild_region == n_hb_region, q8_same == n_ss: the first
    # line of the driver's table
    # record(): 'secondary' - DSSP's backbone hydrogen bonds, bridges and states of the antibody against the crystal structure - and,
    # with a relaxer, 'secondary_relaxed'; one launch per table


# -------------------------------------------------------------------------------------------------------------------
# host twin (float64, numpy)
# -------------------------------------------------------------------------------------------------------------------
def _norm(d):
    """sqrt((dx*dx + dy*dy) + dz*dz) over the last axis, the bracketing of csrc/secondary.hip::norm3."""
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def _shift(M, di, dj):
    """S[i, j] = M[i + di, j + dj], False outside."""
    n = M.shape[0]
    S = np.zeros_like(M)
    i0, i1, j0, j1 = max(0, -di), min(n, n - di), max(0, -dj), min(n, n - dj)
    if i0 < i1 and j0 < j1:
        S[i0:i1, j0:j1] = M[i0 + di:i1 + di, j0 + dj:j1 + dj]
    return S


def _window(v, lo, hi):
    """w[k] = any v[k + d], lo <= d <= hi, False outside."""
    n = v.shape[0]
    w = np.zeros(n, bool)
    for d in range(lo, hi + 1):
        a, b = max(0, -d), min(n, n - d)
        if a < b:
            w[a:b] |= v[a + d:b + d]
    return w


def _analyse(x, mask, aa, chain, residx, th, pro, near, mistake=None):
    """Bonds, patterns and states of ONE structure.  x (Lab,14,3) float64, mask (Lab,14) bool (res_mask applied) -> dict."""
    Lab = x.shape[0]
    N, CA, C, O = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
    present = mask[:, 0] & mask[:, 1] & mask[:, 2] & mask[:, 3]
    link = np.zeros(Lab, bool)                                                  # link[i]: the link (i-1, i)
    if Lab > 1:
        link[1:] = present[:-1] & present[1:] & (chain[1:] == chain[:-1]) & (True if residx is None else residx[1:] == residx[:-1] + 1)
    broken = np.cumsum(~link)                                                   # cont(i, j), i <= j: broken[j] == broken[i]
    idx = np.arange(Lab)

    def cont(lo, hi):
        ok = (lo >= 0) & (hi < Lab)
        return ok & (broken[np.clip(hi, 0, Lab - 1)] == broken[np.clip(lo, 0, Lab - 1)])

    # the virtual hydrogen
    has_h = link & ((aa != pro) | (mistake == 'pro_donates'))
    src = idx if mistake == 'h_from_own_row' else np.maximum(idx - 1, 0)
    v = C[src] - O[src]
    n = _norm(v)
    has_h &= n != 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        H = N + v / n[:, None]
        # the energy of donor i (axis 0) and acceptor j (axis 1)
        pair = has_h[:, None] & present[None, :] & (idx[:, None] != idx[None, :])
        if mistake != 'own_peptide_bond':
            pair &= ~((idx[None, :] == idx[:, None] - 1) & link[:, None])
        dca = CA[:, None, :] - CA[None, :, :]
        d2 = (dca[..., 0] * dca[..., 0] + dca[..., 1] * dca[..., 1]) + dca[..., 2] * dca[..., 2]
        near(d2, CA_CUTOFF2, CA_CUTOFF2, pair)
        pair &= d2 < CA_CUTOFF2
        d_no, d_hc = _norm(N[:, None, :] - O[None, :, :]), _norm(H[:, None, :] - C[None, :, :])
        d_ho, d_nc = _norm(H[:, None, :] - O[None, :, :]), _norm(N[:, None, :] - C[None, :, :])
        e = COULOMB * (((1.0 / d_no + 1.0 / d_hc) - 1.0 / d_ho) - 1.0 / d_nc)
    e = np.where((d_no < MIN_DIST) | (d_hc < MIN_DIST) | (d_ho < MIN_DIST) | (d_nc < MIN_DIST), MIN_ENERGY, e)
    e = np.where(pair, e, 0.0)
    near(e, th['hb_energy'], th['hb_energy'], pair)
    HB = pair & (e < th['hb_energy'])                                           # HB[i, j]: hb(j -> i)
    E = e
    if mistake == 'acceptor_donor_swapped':
        HB, E = HB.T.copy(), e.T.copy()
    # turns: turn[n][i] = cont(i, i + n) and hb(i -> i + n)
    turn = {}
    for n_ in (3, 4, 5):
        t = np.zeros(Lab, bool)
        if Lab > n_:
            t[:Lab - n_] = HB[idx[n_:], idx[:Lab - n_]]
        turn[n_] = t & cont(idx, idx + n_)
    # bridges
    cont3 = (idx >= 1) & (idx <= Lab - 2) & cont(idx - 1, idx + 1)
    ok = cont3[:, None] & cont3[None, :] & (np.abs(idx[:, None] - idx[None, :]) >= 3)
    T = HB.T                                                                    # T[i, j] = HB[j, i]
    # with A[i, j] = HB[i, j]:  hb(i-1 -> j) = HB[j, i-1] = T[i-1, j];  hb(j -> i+1) = HB[i+1, j];  hb(j-1 -> i) = HB[i, j-1];  hb(i -> j+1) = T[i, j+1]
    par = ok & ((_shift(T, -1, 0) & _shift(HB, 1, 0)) | (_shift(HB, 0, -1) & _shift(T, 0, 1)))
    # hb(i -> j) = T[i, j];  hb(j -> i) = HB[i, j];  hb(i-1 -> j+1) = T[i-1, j+1];  hb(j-1 -> i+1) = HB[i+1, j-1]
    anti = ok & ((T & HB) | (_shift(T, -1, 1) & _shift(HB, 1, -1)))
    if mistake == 'parallel_as_antiparallel':
        par, anti = anti, par
    lad = (par & (_shift(par, 1, 1) | _shift(par, -1, -1))) | (anti & (_shift(anti, 1, -1) | _shift(anti, -1, 1)))
    bridged, laddered = (par | anti).any(1), lad.any(1)
    # bends
    bend = np.zeros(Lab, bool)
    if Lab >= 5:
        u, w = CA[2:-2] - CA[:-4], CA[4:] - CA[2:-2]
        c = (u[:, 0] * w[:, 0] + u[:, 1] * w[:, 1]) + u[:, 2] * w[:, 2]
        rhs = th['bend'][0] * (_norm(u) * _norm(w))
        can = cont(idx[2:-2] - 2, idx[2:-2] + 2)
        near(c, rhs, _norm(u) * _norm(w), can)
        bend[2:-2] = can & (c < rhs)
    # states
    start = {n_: turn[n_] & np.concatenate([[False], turn[n_][:-1]]) for n_ in (3, 4, 5)}
    state = np.zeros(Lab, np.int64)
    is_h = _window(start[4], -3, 0)
    if mistake == 'g_over_h':
        is_g = _window(start[3], -2, 0)
        state[is_h & ~is_g] = ST_H
        state[is_g] = ST_G
    else:
        state[is_h] = ST_H
    free = state == 0
    state[free & bridged & laddered] = ST_E
    state[free & bridged & ~laddered] = ST_B
    for n_, code in ((3, ST_G), (5, ST_I)):
        if mistake == 'g_over_h' and n_ == 3:
            continue
        taken = state != 0
        clear = start[n_] & ~_window(taken, 0, n_ - 1)
        state[_window(clear, -(n_ - 1), 0) & (state == 0)] = code
    is_t = _window(turn[3], -2, -1) | _window(turn[4], -3, -1) | _window(turn[5], -4, -1)
    state[(state == 0) & is_t] = ST_T
    state[(state == 0) & bend] = ST_S
    state[state == 0] = ST_C
    state[~present] = ST_NONE
    return dict(present=present, has_h=has_h, HB=HB, E=E, turn=turn, par=par, anti=anti, bend=bend, state=state)


def secondary_host(x, mask, aa, gt_x, gt_mask, gt_aa, Lab, chain_id, residx=None, region=None, res_mask=None, hb_energy=-0.5, mistake=None):
    """abx_secondary_scores for ONE structure on the host, with the same IEEE operations in the same order (numpy multiplies and adds
    in separate passes) and the constants of `thresholds`.  x (>=Lab,14,3) the design's coordinates (rounded to float32 first: what the
    kernel reads), mask (>=Lab,14) its atoms, aa (>=Lab) its tokens; gt_x, gt_mask, gt_aa the same of the wild type; chain_id, residx,
    region, res_mask (>=Lab) or None.  Only the first Lab rows are read.
    -> dict(row (len(SECONDARY_COLUMNS),) float64, rows (Lab,6) int32 ROW_COLUMNS, classes (Lab) int32, wild_classes (Lab) int32,
            hb (Lab,Lab) bool: hb[i, j] = hb(j -> i), donor i, acceptor j, of the design; par, anti (Lab,Lab) bool: its bridges,
            n_borderline: the decisions - the energy against the threshold, the C-alpha cutoff, the bend - whose two sides differ by less
            than 1e-9 relative: those a device evaluation could take differently).
    mistake: None, or the name of a deliberate error the tests show a column or a string for (MISTAKES)."""
    assert mistake is None or mistake in MISTAKES, mistake
    Lab = int(Lab)
    keep = np.ones(Lab, bool) if res_mask is None else (to_np(res_mask)[:Lab] != 0)
    xd = to_np(x)[:Lab].astype(np.float32).astype(np.float64)
    xw = to_np(gt_x)[:Lab].astype(np.float32).astype(np.float64)
    md, mw = (to_np(mask)[:Lab] != 0) & keep[:, None], (to_np(gt_mask)[:Lab] != 0) & keep[:, None]
    aa_d, aa_w = (np.where((t < 0) | (t > 20), 20, t) for t in (to_np(aa)[:Lab].astype(np.int64), to_np(gt_aa)[:Lab].astype(np.int64)))
    chain = to_np(chain_id)[:Lab].astype(np.int64)
    rsx = None if residx is None else to_np(residx)[:Lab].astype(np.int64)
    if mistake == 'chain_linked':
        chain = np.zeros_like(chain)
        rsx = None if rsx is None else np.arange(Lab)
    reg = np.zeros(Lab, bool) if region is None else ((to_np(region)[:Lab] != 0) & keep)
    th = thresholds(hb_energy)
    pro = type_index('P')
    near = _Borderline()
    W = _analyse(xw, mw, aa_w, chain, rsx, th, pro, near, mistake)
    D = _analyse(xd, md, aa_d, chain, rsx, th, pro, near, mistake)
    end = reg[:, None] | reg[None, :]
    upper = np.triu(np.ones((Lab, Lab), bool), 1)
    row = np.zeros(len(SECONDARY_COLUMNS))
    row[0], row[1], row[2] = D['HB'].sum(), (D['HB'] & end).sum(), (D['HB'] & reg[:, None] & reg[None, :]).sum()
    row[3], row[4] = (W['HB'] & end).sum(), (W['HB'] & D['HB'] & end).sum()
    row[5] = float(np.rint(D['E'][D['HB'] & end] * FIXED).astype(np.int64).sum()) / FIXED
    pairs = lambda S: (S['par'] & end & upper).sum() + (S['anti'] & end & upper).sum()
    row[6], row[7] = pairs(D), pairs(W)
    row[8] = (D['par'] & W['par'] & end & upper).sum() + (D['anti'] & W['anti'] & end & upper).sum()
    sd, sw = D['state'], W['state']
    for k, code in enumerate((ST_H, ST_G, ST_I, ST_E, ST_B, ST_T, ST_S, ST_C)):
        row[9 + k] = ((sd == code) & reg).sum()
    both = reg & D['present'] & W['present']
    c3 = np.asarray(CLASS3)
    row[17], row[18], row[19] = both.sum(), (both & (sd == sw)).sum(), (both & (c3[sd] == c3[sw])).sum()
    row[20], row[21] = ((sd == ST_E) | (sd == ST_B)).sum(), ((sd == ST_H) | (sd == ST_G) | (sd == ST_I)).sum()
    rows = np.full((Lab, len(ROW_COLUMNS)), -1, np.int32)
    rows[:, 0], rows[:, 1], rows[:, 2] = sd, D['HB'].sum(1), D['HB'].sum(0)
    partners = D['par'] | D['anti']
    for i in np.nonzero(partners.any(1))[0]:
        js = np.nonzero(partners[i])[0][:2]
        rows[i, 3:3 + len(js)] = js
    rows[:, 5] = (np.where(reg, F_REGION, 0) | np.where(D['present'], F_PRESENT, 0) | np.where(D['has_h'], F_HAS_H, 0) |
                  np.where(D['par'].any(1), F_PARALLEL, 0) | np.where(D['anti'].any(1), F_ANTIPARALLEL, 0) | np.where(D['bend'], F_BEND, 0) |
                  np.where(D['turn'][3], F_TURN3, 0) | np.where(D['turn'][4], F_TURN4, 0) | np.where(D['turn'][5], F_TURN5, 0))
    return dict(row=row, rows=rows, classes=sd.astype(np.int32), wild_classes=sw.astype(np.int32), hb=D['HB'], par=D['par'], anti=D['anti'],
                n_borderline=near.n)
