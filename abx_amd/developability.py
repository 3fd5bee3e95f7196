"""Developability of designs: can the antibody be made, and is it likely to aggregate?  The three filters every antibody pipeline applies
to a binder before it is taken forward, on the FREE antibody (rows < Lab; the antigen enters only through acc_alone, the antibody's
surface with the antigen taken away): spatial aggregation propensity (SAP, Chennamsetty et al. 2009, with the per-residue grouping
multiplied out into per-atom weights), the net charge of the heavy and the light chain and their product, and the sequence liabilities
(N-glycosylation, deamidation, isomerisation, fragmentation, oxidation, free cysteines) of residues whose side chain is exposed.
Not covered: no pI, no patch metrics (PSH / PPC / PNC: abx_amd.patches), no hydrogens; His carries no charge.  The reference side-chain
area is that of the ISOLATED residue, somewhat larger than Ala-X-Ala tripeptide values: compare designs with the `wild` line, not with
literature thresholds.

Every decision is exact: float64 from the float32 coordinates in a fixed IEEE operation order, fixed-point integer weights, int64 sums
(include/abx_hip.h, AbxDevelopabilityArgs): the row of the device (`DevelopabilityScorer`, abx_developability_scores,
csrc/developability.hip) and of the host twin (`developability_host`, numpy) are equal bit for bit.  The surface comes from the point
counts of the interface analysis (abx_amd.interface: acc_alone of every atom14 slot)."""
import functools

import numpy as np

from . import complex_view
from .complex_view import to_np
from .interface import FOUR_PI, SurfaceScorer

# The row of abx_developability_scores (include/abx_hip.h, ABX_DEV_COLS)
DEVELOPABILITY_COLUMNS = ('sap_pos', 'sap_pos_cdr', 'sap_pos_region', 'sap_max_res', 'n_res_sap_pos', 'n_res_sap_pos_region', 'charge_heavy',
                          'charge_light', 'charge_product', 'n_his', 'n_glyc', 'n_deamid', 'n_isomer', 'n_frag', 'n_met_ox', 'n_trp_ox',
                          'n_cys_free', 'n_liab', 'n_liab_region', 'n_liab_cdr', 'n_atoms')
COUNT_COLUMNS = tuple(c for c in DEVELOPABILITY_COLUMNS if c.startswith(('n_', 'charge_')))
# design minus wild type: the columns the driver writes a difference for
DELTA_COLUMNS = ('sap_pos', 'sap_pos_cdr', 'sap_pos_region', 'sap_max_res', 'charge_heavy', 'charge_light', 'n_liab', 'n_liab_region')
# the per-residue table of --developability_rows (AbxDevelopabilityArgs.rows): the liability mask has bit k for column 10 + k
ROW_COLUMNS = ('sap_mean', 'rel_side_chain_area', 'liability_mask', 'charge')
CDR_CODES = (1, 3, 5, 8, 10, 12)
FIXED_ONE = 1 << 30                     # the fixed point of the atom weights
CYS_SS2 = 6.25                          # an SG within 2.5 Angstrom of another is bonded

# Black & Mould (1991), Anal. Biochem. 193, 72-82: hydrophobicity of the 20 side chains scaled to 0 (Arg) .. 1 (Phe); used by
# Chennamsetty et al. (2009), PNAS 106, 11937-11942, shifted so that Gly = 0 (`hydrophobicity()` subtracts it; X = 0).  Typed from the
# publication.
HYDROPHOBICITY = {'A': 0.616, 'R': 0.000, 'N': 0.236, 'D': 0.028, 'C': 0.680, 'Q': 0.251, 'E': 0.043, 'G': 0.501, 'H': 0.165, 'I': 0.943,
                  'L': 0.943, 'K': 0.283, 'M': 0.738, 'F': 1.000, 'P': 0.711, 'S': 0.359, 'T': 0.450, 'W': 0.878, 'Y': 0.880, 'V': 0.825}

format_developability = functools.partial(complex_view.format_row, DEVELOPABILITY_COLUMNS, COUNT_COLUMNS, 3)
format_delta = functools.partial(complex_view.format_delta, DEVELOPABILITY_COLUMNS, COUNT_COLUMNS, DELTA_COLUMNS, 3)


def hydrophobicity():
    """(21,) float64 per residue type: HYDROPHOBICITY minus its Gly value; X (row 20) is 0."""
    from . import residue_constants as rc
    h = np.zeros(21, np.float64)
    for i, r in enumerate(rc.restypes):
        h[i] = HYDROPHOBICITY[r] - HYDROPHOBICITY['G']
    return h


def ideal_residue(t):
    """(14,3) float64 atom14 coordinates of residue type t alone in its ideal geometry with every chi at 180 degrees, from the
    rigid-group tables: frame 0 is the identity, frames 1-3 their default frames, frame 4 = default[4] F, frame g = frame[g-1]
    default[g] F for g = 5..7, F = diag(1, -1, -1, 1) (the rotation by 180 degrees about x); atom = frame of its group x its position."""
    from . import residue_constants as rc
    default = np.asarray(rc.restype_rigid_group_default_frame, np.float64)[t]            # (8,4,4)
    group = np.asarray(rc.restype_atom14_to_rigid_group)[t]
    pos = np.asarray(rc.restype_atom14_rigid_group_positions, np.float64)[t]             # (14,3)
    F = np.diag([1.0, -1.0, -1.0, 1.0])
    frames = [np.eye(4), default[1], default[2], default[3], default[4] @ F]
    for g in range(5, 8):
        frames.append(frames[g - 1] @ default[g] @ F)
    return np.stack([(frames[group[s]] @ np.append(pos[s], 1.0))[:3] for s in range(14)])


def area_table(P, probe):
    """(21,14) float64: the area of one sphere point of every atom14 slot, 4 pi (r + probe)^2 / P; 0 where the type has no such slot."""
    from .interface import _radius_table
    rad = _radius_table()
    R = rad.astype(np.float64) + float(probe)
    return np.where(rad > 0, FOUR_PI * (R * R) / float(int(P)), 0.0)


def side_chain_area(points, a_of_row):
    """(L,) float64: sum over the slots >= 4 of acc_alone x the area of a point, in slot order (one multiplication and one addition per
    slot, as the kernel does).  points (L,14) integer counts, a_of_row (L,14) float64."""
    rel = np.zeros(points.shape[0], np.float64)
    for s in range(4, 14):
        rel = rel + points[:, s].astype(np.float64) * a_of_row[:, s]
    return rel


@functools.lru_cache(maxsize=None)
def _reference_areas(P, probe):
    from . import residue_constants as rc
    from .interface import interface_host
    a = area_table(P, probe)
    ref = np.zeros(21, np.float64)
    mask = np.asarray(rc.restype_atom14_mask) != 0
    for t in range(20):
        pts = interface_host(ideal_residue(t)[None], mask[t][None], np.array([t]), 1, n_points=P, probe=probe)[1]
        ref[t] = side_chain_area(pts[..., 0].astype(np.int64), a[t][None])[0]
    ref.setflags(write=False)
    return ref


def reference_areas(P=128, probe=1.4):
    """(21,) float64: the solvent-accessible side-chain area (slots >= 4) of every residue type alone (`ideal_residue`), by this
    project's own Shrake-Rupley (interface.interface_host) with P points, `probe` and the project's radii; Gly and X are 0.  Built on
    the host once per (P, probe)."""
    return _reference_areas(int(P), float(probe))


@functools.lru_cache(maxsize=None)
def _weight_table(P, probe):
    a, ref, h = area_table(P, probe), _reference_areas(P, probe), hydrophobicity()
    q = np.zeros((21, 14), np.int64)
    for t in range(21):
        if ref[t] > 0:
            q[t, 4:] = np.rint(float(FIXED_ONE) * a[t, 4:] * h[t] / ref[t]).astype(np.int64)
    for arr in (q, a):
        arr.setflags(write=False)
    return q, a, ref


def weight_table(P=128, probe=1.4):
    """(q (21,14) int64, a (21,14) float64, ref (21,) float64): q = rint(2^30 a h / ref), the fixed-point SAP weight of one accessible
    sphere point of a side-chain slot (0 on slots < 4, for Gly and for X); a = area_table, ref = reference_areas."""
    return _weight_table(int(P), float(probe))


class DevelopabilityScorer(SurfaceScorer):
    """Developability rows of batches of designs of ONE complex on the device.  Built once per complex from its featurised batch (or the
    un-batched complex) like polar.PolarScorer, and holds an InterfaceScorer for the point counts (interface.SurfaceScorer: region,
    n_points / probe of the surface, interface).  radius: of the SAP sphere (Angstrom); exposed: smallest relative side-chain area of an
    exposed residue."""

    COLUMNS = DEVELOPABILITY_COLUMNS

    def __init__(self, batch, region=None, radius=10.0, exposed=0.075, n_points=128, probe=1.4, interface=None):
        import torch
        if not (radius > 0 and 0.0 <= exposed <= 1.0):
            raise ValueError(f'developability: needs radius > 0 and exposed in [0, 1] (got {radius}, {exposed})')
        super().__init__(batch, region, n_points, probe, interface)
        view = complex_view.ComplexView(batch, chains=True, cdr=True)
        self.chain_id, self.residx, self.cdr_def = view.chain_id, view.residx, view.cdr_def
        P, probe = int(self.interface.sphere.shape[0]), self.interface.kw['probe']
        q, a, ref = weight_table(P, probe)
        self.tables = tuple(torch.from_numpy(np.array(t)).to(self.device) for t in (q, a, ref))     # (copies: the cached tables are read-only)
        self.kw = dict(radius=float(radius), exposed=float(exposed), n_points=P, q_max=int(np.abs(q).max()))

    def new_rows(self, B):
        """An uninitialised (B, L, 4) float64 tensor for ROW_COLUMNS of B structures."""
        import torch
        return torch.empty(B, self.L, 4, dtype=torch.float64, device=self.device)

    def score(self, atom14, seq, out=None, points=None, rows=None, mask=None, j_chunk=0):
        """atom14 (B, Lab or L, 14, 3) f32 predicted coordinates, seq (B, Lab) tokens -> (B, len(DEVELOPABILITY_COLUMNS)) float64 on the
        device; out: rows to write into (any row stride); rows: (B,L,4) float64 to receive ROW_COLUMNS of every residue; points: the
        (B,L,14,2) int32 acc_alone / acc_cplx that the interface scorer returned for THESE structures (None: its kernel runs here).
        No host synchronisation."""
        from abx_amd import ops
        points = self.points_of(atom14, seq, points, mask)
        return ops.developability_scores(atom14, seq, self.gt_atom14, self.gt_seq, self.gt_exists, self.chain_id, self.cdr_def, self.tables, points,
                                         Lab=self.Lab, residx=self.residx, region=self.region, mask=mask, res_mask=self.res_mask, out=out,
                                         rows=rows, j_chunk=j_chunk, **self.kw)

    def side_outputs(self, B):
        """want_rows: the record of the designs also carries 'developability_rows' (B, L, 4) float64."""
        return dict(rows=self.new_rows(B)) if self.want_rows else {}

    # record(): 'developability' - aggregation propensity, chain charges and sequence liabilities of the free antibody - and, with a
    # relaxer, 'developability_relaxed'; three launches per table


# -------------------------------------------------------------------------------------------------------------------
# host twin (float64 and int64, numpy)
# -------------------------------------------------------------------------------------------------------------------
def developability_host(x, mask, aa, Lab, chain_id, residx, cdr_def, region=None, points=None, radius=10.0, exposed=0.075, n_points=128,
                        probe=1.4, details=False):
    """The row of abx_developability_scores for ONE structure on the host, with the same IEEE operations in the same order and the same
    integers.  x (L,14,3) coordinates (rounded to float32 first: what the kernel reads), mask (L,14) which slots exist, aa (L) residue
    tokens, Lab = rows of the antibody, chain_id / cdr_def (L), residx (L) or None (array neighbours of a chain are linked), region (L)
    or None, points (L,14,2) acc_alone / acc_cplx of every slot (None: interface.interface_host computes them with n_points and probe).
    -> (row (len(DEVELOPABILITY_COLUMNS),) float64, rows (L,4) float64 ROW_COLUMNS); details=True adds a dict: 'sap' (L,14) int64 SAP_i
    of every counted atom (0 elsewhere), 'w' (L,14) int64 the weights, 'counted' (L,14) bool, 'exposed' (L) bool."""
    from .interface import _radius_table, interface_host
    x = to_np(x).astype(np.float32)
    L, Lab = x.shape[0], int(Lab)
    aa = np.clip(to_np(aa).astype(np.int64), 0, 20)
    mask = to_np(mask) != 0
    chain = to_np(chain_id).astype(np.int64)
    resi = None if residx is None else to_np(residx).astype(np.int64)
    cdr = np.isin(to_np(cdr_def).astype(np.int64), CDR_CODES)
    reg = np.zeros(L, bool) if region is None else (to_np(region) != 0)
    if points is None:
        points = interface_host(x, mask, aa, Lab, region=region, n_points=n_points, probe=probe)[1]
    alone = to_np(points).astype(np.int64)[..., 0]
    q, a, ref = weight_table(n_points, probe)
    ab = np.arange(L) < Lab
    counted = mask & (_radius_table()[aa] > 0) & ab[:, None]
    w = np.where(counted, alone * q[aa], 0)                                     # (L,14) int64
    rows_i, slots_i = np.nonzero(counted)
    ci = x[rows_i, slots_i].astype(np.float64)
    N = rows_i.shape[0]
    sap = np.zeros(N, np.int64)
    jj = np.nonzero(w[rows_i, slots_i] != 0)[0]
    if N and jj.shape[0]:
        cj, wj = ci[jj], w[rows_i, slots_i][jj]
        r2 = float(radius) * float(radius)
        for i0 in range(0, N, 512):
            dx, dy, dz = (cj[None, :, k] - ci[i0:i0 + 512, None, k] for k in range(3))
            near = ((dx * dx + dy * dy) + dz * dz) <= r2
            sap[i0:i0 + 512] = (near * wj[None]).sum(1)
    pos = np.maximum(sap, 0)
    row_sum, row_n = np.zeros(L, np.int64), np.zeros(L, np.int64)
    np.add.at(row_sum, rows_i, sap)
    np.add.at(row_n, rows_i, 1)
    present = row_n > 0
    mean = np.zeros(L, np.float64)
    mean[present] = row_sum[present].astype(np.float64) / row_n[present].astype(np.float64) / float(FIXED_ONE)
    out = np.zeros(len(DEVELOPABILITY_COLUMNS), np.float64)
    out[0] = float(pos.sum()) / float(FIXED_ONE)
    out[1] = float(pos[cdr[rows_i]].sum()) / float(FIXED_ONE)
    out[2] = float(pos[reg[rows_i]].sum()) / float(FIXED_ONE)
    out[3] = mean[present].max() if present.any() else 0.0
    out[4] = (present & (row_sum > 0)).sum()
    out[5] = (present & (row_sum > 0) & reg).sum()
    # charges
    charge = np.where(present, np.isin(aa, (1, 11)).astype(np.int64) - np.isin(aa, (3, 6)).astype(np.int64), 0)
    heavy = chain == chain[0]
    out[6], out[7] = charge[heavy].sum(), charge[~heavy].sum()
    out[8] = out[6] * out[7]
    out[9] = (present & (aa == 8)).sum()
    # exposure and the linked rows
    rel = side_chain_area(np.where(counted, alone, 0), a[aa])
    is_exposed = present & (ref[aa] > 0) & (rel >= float(exposed) * ref[aa])
    link = np.zeros(L, bool)                                                    # row r is linked to row r - 1
    link[1:] = present[1:] & present[:-1] & (chain[1:] == chain[:-1]) & (True if resi is None else (resi[1:] == resi[:-1] + 1))
    nxt = lambda k: np.concatenate([aa[k:], np.full(k, 20)])                    # the type k rows on
    lk1 = np.concatenate([link[1:], [False]])
    lk2 = lk1 & np.concatenate([link[2:], [False, False]])
    n_, d_ = is_exposed & (aa == 2), is_exposed & (aa == 3)
    liab = np.zeros((7, L), bool)
    liab[0] = n_ & lk2 & (nxt(1) != 14) & np.isin(nxt(2), (15, 16))
    liab[1] = n_ & lk1 & np.isin(nxt(1), (7, 15))
    liab[2] = d_ & lk1 & np.isin(nxt(1), (7, 15))
    liab[3] = d_ & lk1 & (nxt(1) == 14)
    liab[4] = is_exposed & (aa == 12)
    liab[5] = is_exposed & (aa == 17)
    sg = np.nonzero(counted[:, 5] & (aa == 4))[0]
    if sg.shape[0]:
        c = x[sg, 5].astype(np.float64)
        dx, dy, dz = (c[None, :, k] - c[:, None, k] for k in range(3))
        bonded = (((dx * dx + dy * dy) + dz * dz) <= CYS_SS2) & ~np.eye(sg.shape[0], dtype=bool)
        liab[6, sg] = ~bonded.any(1)
    out[10:17] = liab.sum(1)
    out[17] = liab.sum()
    out[18] = liab[:, reg].sum()
    out[19] = liab[:, cdr].sum()
    out[20] = N
    rows = np.zeros((L, 4), np.float64)
    rows[:, 0] = mean
    rows[:, 1] = np.where(present & (ref[aa] > 0), rel / np.where(ref[aa] > 0, ref[aa], 1.0), 0.0)
    rows[:, 2] = (liab * (1 << np.arange(7))[:, None]).sum(0)
    rows[:, 3] = charge
    if details:
        full = np.zeros((L, 14), np.int64)
        full[rows_i, slots_i] = sap
        return out, rows, dict(sap=full, w=w, counted=counted, exposed=is_exposed)
    return out, rows
