"""Surface patches of designs: do the hydrophobic or the like-charged residues around the paratope sit NEXT TO each other?  Three of the
five numbers of the Therapeutic Antibody Profiler (Raybould et al. 2019, PNAS 116, 4025) on the FREE antibody (rows < Lab) - the patches
of surface hydrophobicity (PSH), of positive charge (PPC) and of negative charge (PNC) over the exposed residues in the vicinity of the
CDRs -, its structural Fv charge symmetry parameter (SFvCSP) and its CDR length; and, from the same closest heavy-atom distances over
antibody x complex, the charge pairing ACROSS the interface out to the same cutoff: opposite charges facing each other (attract) and
like charges facing each other (repel), which the salt bridges of `polar` (4 Angstrom) do not reach.

A residue is EXPOSED by developability's rule: its side-chain area in the free antibody is at least `exposed` (0.075) of the reference
area of its type; Gly and X have no reference area and are never exposed.  Not the TAP server's numbers: the reference area is this
project's isolated-residue area, the CDRs are `cdr_def` as featurised without the +-2 anchors, there are no hydrogens and no pI, and His
carries +0.1 as in TAP.  Compare designs with the `wild` line, not with TAP's amber / red thresholds.

Every decision is exact: float64 from the float32 coordinates in a fixed IEEE operation order, fixed-point integer terms, int64 sums
(include/abx_hip.h, AbxPatchArgs): the row of the device (`PatchScorer`, abx_patch_scores, csrc/patches.hip) and of the host twin
(`patches_host`, numpy) are equal bit for bit, for finite coordinates."""
import functools

import numpy as np

from . import complex_view
from .complex_view import to_np
from .interface import SurfaceScorer
from .developability import CDR_CODES, FIXED_ONE, side_chain_area, weight_table

# The row of abx_patch_scores (include/abx_hip.h, ABX_PATCH_COLS)
PATCHES_COLUMNS = ('psh', 'ppc', 'pnc', 'sfvcsp', 'psh_region', 'ppc_region', 'pnc_region', 'cross_attract', 'cross_repel',
                   'cross_attract_region', 'cross_repel_region', 'n_cdr', 'n_exposed', 'n_vicinity', 'n_pairs', 'n_salt', 'n_cross',
                   'n_cross_region')
COUNT_COLUMNS = tuple(c for c in PATCHES_COLUMNS if c.startswith('n_'))
# design minus wild type: the columns the driver writes a difference for
DELTA_COLUMNS = PATCHES_COLUMNS[0:5] + PATCHES_COLUMNS[7:11]
# the per-residue table of --patches_rows (AbxPatchArgs.rows)
ROW_COLUMNS = ('psh', 'charge_patch', 'cross_charge', 'flags')
F_PRESENT, F_EXPOSED, F_SEED, F_VICINITY, F_SALT, F_REGION = 1, 2, 4, 8, 16, 32     # bits of ROW_COLUMNS' flags
PLACES = {None: 4, 'psh': 3, 'psh_region': 3, 'sfvcsp': 2}

# Kyte & Doolittle (1982), J. Mol. Biol. 157, 105-132: the hydropathy index of the 20 side chains.  Typed from the publication.
KYTE_DOOLITTLE = {'A': 1.8, 'R': -4.5, 'N': -3.5, 'D': -3.5, 'C': 2.5, 'Q': -3.5, 'E': -3.5, 'G': -0.4, 'H': -3.2, 'I': 4.5, 'L': 3.8,
                  'K': -3.9, 'M': 1.9, 'F': 2.8, 'P': -1.6, 'S': -0.8, 'T': -0.7, 'W': -0.9, 'Y': -1.3, 'V': 4.2}
# TAP's charges in tenths: Lys, Arg +1, Asp, Glu -1, His +0.1
CHARGE_TENTHS = {'K': 10, 'R': 10, 'D': -10, 'E': -10, 'H': 1}

format_patches = functools.partial(complex_view.format_row, PATCHES_COLUMNS, COUNT_COLUMNS, PLACES)
format_delta = functools.partial(complex_view.format_delta, PATCHES_COLUMNS, COUNT_COLUMNS, DELTA_COLUMNS, PLACES)


def kyte_doolittle():
    """(21,) float64 per residue type: the hydropathy index normalised to 1 (Arg) .. 2 (Ile) as in TAP, H = 1 + (KD + 4.5) / 9; X (row
    20) is 0."""
    from . import residue_constants as rc
    h = np.zeros(21, np.float64)
    for i, r in enumerate(rc.restypes):
        h[i] = 1.0 + (KYTE_DOOLITTLE[r] + 4.5) / 9.0
    return h


def charge_table():
    """(21,) int64 per residue type: the charge in tenths (CHARGE_TENTHS; 0 for every other type and for X)."""
    from . import residue_constants as rc
    q = np.zeros(21, np.int64)
    for i, r in enumerate(rc.restypes):
        q[i] = CHARGE_TENTHS.get(r, 0)
    return q


def gly_type():
    from . import residue_constants as rc
    return rc.restypes.index('G')


class PatchScorer(SurfaceScorer):
    """Patch rows of batches of designs of ONE complex on the device.  Built once per complex from its featurised batch (or the
    un-batched complex) like developability.DevelopabilityScorer, and holds an InterfaceScorer for the point counts
    (interface.SurfaceScorer: region, n_points / probe of the surface, interface).  cutoff: of a patch pair and of a cross pair,
    vicinity: of a CDR residue, salt: of a salt bridge (closest heavy-atom distances, Angstrom); exposed: smallest relative side-chain
    area of an exposed residue (Gly and X are never exposed)."""

    COLUMNS = PATCHES_COLUMNS

    def __init__(self, batch, region=None, cutoff=7.5, vicinity=4.0, salt=3.2, exposed=0.075, n_points=128, probe=1.4, interface=None):
        import torch
        from .polar import polar_table_on
        if not (cutoff > 0 and vicinity > 0 and salt > 0 and 0.0 <= exposed <= 1.0):
            raise ValueError(f'patches: needs cutoff, vicinity and salt > 0 and exposed in [0, 1] (got {cutoff}, {vicinity}, {salt}, {exposed})')
        super().__init__(batch, region, n_points, probe, interface)
        dev = self.device
        view = complex_view.ComplexView(batch, chains=True, cdr=True)
        self.chain_id, self.cdr_def = view.chain_id, view.cdr_def
        _, a, ref = weight_table(int(self.interface.sphere.shape[0]), self.interface.kw['probe'])
        h, q10 = kyte_doolittle(), charge_table()
        # (copies: the cached tables are read-only)
        self.tables = tuple(torch.from_numpy(np.array(t)).to(dev) for t in (h, q10.astype(np.int32), a, ref)) + (polar_table_on(dev),)
        self.kw = dict(cutoff=float(cutoff), vicinity=float(vicinity), salt=float(salt), exposed=float(exposed),
                       h_max=float(np.abs(h).max()), q_max=int(np.abs(q10).max()), gly=gly_type())

    def new_rows(self, B):
        """An uninitialised (B, L, 4) float64 tensor for ROW_COLUMNS of B structures."""
        import torch
        return torch.empty(B, self.L, 4, dtype=torch.float64, device=self.device)

    def score(self, atom14, seq, out=None, points=None, rows=None, mask=None, workspace=None):
        """atom14 (B, Lab or L, 14, 3) f32 predicted coordinates, seq (B, Lab) tokens -> (B, len(PATCHES_COLUMNS)) float64 on the device;
        out: rows to write into (any row stride); rows: (B,L,4) float64 to receive ROW_COLUMNS of every residue; points: the (B,L,14,2)
        int32 acc_alone / acc_cplx that the interface scorer returned for THESE structures (None: its kernel runs here); workspace: a
        uint8 tensor of at least ops.patch_workspace_bytes(B, L, Lab) bytes (None: allocated here).  No host synchronisation."""
        from abx_amd import ops
        points = self.points_of(atom14, seq, points, mask)
        return ops.patch_scores(atom14, seq, self.gt_atom14, self.gt_seq, self.gt_exists, self.chain_id, self.cdr_def, self.tables, points,
                                Lab=self.Lab, region=self.region, mask=mask, res_mask=self.res_mask, out=out, rows=rows,
                                workspace=workspace, **self.kw)

    def side_outputs(self, B):
        """want_rows: the record of the designs also carries 'patches_rows' (B, L, 4) float64."""
        return dict(rows=self.new_rows(B)) if self.want_rows else {}

    # record(): 'patches' - the patches of surface hydrophobicity and charge around the CDRs of the free antibody, its charge symmetry,
    # the charge pairing across the interface - and, with a relaxer, 'patches_relaxed'; three launches per table


# -------------------------------------------------------------------------------------------------------------------
# host twin (float64 and int64, numpy)
# -------------------------------------------------------------------------------------------------------------------
def closest_approach(x, counted, roles, Lab):
    """(D2, S2), both (Lab, L) float64: the smallest squared distance between a counted atom of row i < Lab and one of row j, and the
    same over the pairs of a cation atom with an anion atom; +inf on the diagonal and where a row has no such pair.  x (L,14,3) float32,
    counted (L,14) bool, roles (L,14) the polar role bits of every slot."""
    from .polar import ANION, CATION
    L = x.shape[0]
    c = x.astype(np.float64)
    cat, an = counted & ((roles & CATION) != 0), counted & ((roles & ANION) != 0)
    D2, S2 = np.full((Lab, L), np.inf), np.full((Lab, L), np.inf)
    for i0 in range(0, Lab, 16):
        i1 = min(i0 + 16, Lab)
        dx, dy, dz = (c[None, None, :, :, k] - c[i0:i1, :, None, None, k] for k in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz                                      # (rows, 14, L, 14)
        pair = counted[i0:i1, :, None, None] & counted[None, None]
        salt = (cat[i0:i1, :, None, None] & an[None, None]) | (an[i0:i1, :, None, None] & cat[None, None])
        D2[i0:i1] = np.where(pair, d2, np.inf).min((1, 3))
        S2[i0:i1] = np.where(salt, d2, np.inf).min((1, 3))
    ii = np.arange(Lab)
    D2[ii, ii] = S2[ii, ii] = np.inf
    return D2, S2


def patches_host(x, mask, aa, Lab, chain_id, residx, cdr_def, region=None, points=None, cutoff=7.5, vicinity=4.0, salt=3.2, exposed=0.075,
                 n_points=128, probe=1.4, salt_override=True, details=False):
    """The row of abx_patch_scores for ONE structure on the host, with the same IEEE operations in the same order and the same integers.
    x (L,14,3) coordinates (rounded to float32 first: what the kernel reads), mask (L,14) which slots exist, aa (L) residue tokens, Lab =
    rows of the antibody, chain_id / cdr_def (L), residx: not read (the signature is developability_host's), region (L) or None, points
    (L,14,2) acc_alone / acc_cplx of every slot (None: interface.interface_host computes them with n_points and probe).
    salt_override=False leaves a salt-bridged row its own hydrophobicity (not a mode of the kernel: it shows what the override does).
    -> (row (len(PATCHES_COLUMNS),) float64, rows (L,4) float64 ROW_COLUMNS); details=True adds a dict: 'D2', 'S2' (Lab, L) float64,
    'present' (L) and 'exposed', 'seed', 'vicinity', 'salt' (Lab) bool."""
    from .interface import _radius_table, interface_host
    from .polar import polar_table
    x = to_np(x).astype(np.float32)
    L, Lab = x.shape[0], int(Lab)
    aa = np.clip(to_np(aa).astype(np.int64), 0, 20)
    mask = to_np(mask) != 0
    chain = to_np(chain_id).astype(np.int64)
    cdr = np.isin(to_np(cdr_def).astype(np.int64), CDR_CODES)
    reg = np.zeros(L, bool) if region is None else (to_np(region) != 0)
    if points is None:
        points = interface_host(x, mask, aa, Lab, region=region, n_points=n_points, probe=probe)[1]
    alone = to_np(points).astype(np.int64)[..., 0]
    _, a, ref = weight_table(n_points, probe)
    H, q10_t = kyte_doolittle(), charge_table()
    counted = mask & (_radius_table()[aa] > 0)
    present = counted.any(1)
    ab = np.arange(L) < Lab
    # 1. exposure of the antibody rows
    rel = side_chain_area(np.where(counted, alone, 0), a[aa])
    is_exposed = (present & ab & (ref[aa] > 0) & (rel >= float(exposed) * ref[aa]))[:Lab]
    # 2. closest approach
    D2, S2 = closest_approach(x, counted, polar_table()[aa], Lab)
    # 3. salt-bridged rows, 4. vicinity
    salted = (S2[:, :Lab] <= float(salt) * float(salt)).any(1)
    seed = is_exposed & cdr[:Lab]
    near_seed = ((D2[:, :Lab] <= float(vicinity) * float(vicinity)) & seed[None, :]).any(1)
    vic = is_exposed & (seed | near_seed)
    # 5. tables
    h_eff = np.where(salted & bool(salt_override), H[gly_type()], H[aa[:Lab]])
    q10 = q10_t[aa]
    Q = q10.astype(np.float64) / 10.0
    cut2 = float(cutoff) * float(cutoff)
    one = float(FIXED_ONE)
    psh_r, chg_r, crs_r = np.zeros(L, np.int64), np.zeros(L, np.int64), np.zeros(L, np.int64)
    sums = np.zeros(10, np.int64)                  # psh, ppc, pnc, their region variants, attract, repel, their region variants
    n_pairs = n_cross = n_cross_region = 0
    # 6. patch terms
    v = np.nonzero(vic)[0]
    for i in v:
        for j in v[v > i]:
            if not D2[i, j] <= cut2:
                continue
            r2 = max(D2[i, j], 1.0)
            n_pairs += 1
            in_reg = reg[i] or reg[j]
            t = int(np.rint(one * ((h_eff[i] * h_eff[j]) / r2)))
            sums[0] += t
            sums[3] += t if in_reg else 0
            psh_r[i] += t
            psh_r[j] += t
            c = int(np.rint(one * (abs(Q[i] * Q[j]) / r2)))
            k = 1 if (q10[i] > 0 and q10[j] > 0) else 2 if (q10[i] < 0 and q10[j] < 0) else 0
            if k:
                sums[k] += c
                sums[3 + k] += c if in_reg else 0
                chg_r[i] += c
                chg_r[j] += c
    # 7. SFvCSP
    heavy = (chain == chain[0])[:Lab]
    q_ab = q10[:Lab]
    sfv = float(int(q_ab[is_exposed & heavy].sum()) * int(q_ab[is_exposed & ~heavy].sum())) / 100.0
    # 8. across the interface
    for i in np.nonzero(present[:Lab] & (q_ab != 0))[0]:
        for j in Lab + np.nonzero(present[Lab:] & (q10[Lab:] != 0) & (D2[i, Lab:] <= cut2))[0]:
            r2 = max(D2[i, j], 1.0)
            c = int(np.rint(one * (abs(Q[i] * Q[j]) / r2)))
            k = 6 if q10[i] * q10[j] < 0 else 7
            sums[k] += c
            sums[k + 2] += c if reg[i] else 0
            n_cross += 1
            n_cross_region += 1 if reg[i] else 0
            crs_r[i] += c if k == 6 else -c
            crs_r[j] += c if k == 6 else -c
    out = np.zeros(len(PATCHES_COLUMNS), np.float64)
    out[0:3] = sums[0:3].astype(np.float64) / one
    out[3] = sfv
    out[4:7] = sums[3:6].astype(np.float64) / one
    out[7:11] = sums[6:10].astype(np.float64) / one
    out[11] = (present[:Lab] & cdr[:Lab]).sum()
    out[12], out[13], out[14], out[15] = is_exposed.sum(), vic.sum(), n_pairs, (salted & vic).sum()
    out[16], out[17] = n_cross, n_cross_region
    rows = np.zeros((L, 4), np.float64)
    rows[:, 0] = psh_r.astype(np.float64) / one
    rows[:, 1] = chg_r.astype(np.float64) / one
    rows[:, 2] = crs_r.astype(np.float64) / one
    flags = np.where(present, F_PRESENT | np.where(reg, F_REGION, 0), 0)
    flags[:Lab] |= np.where(is_exposed, F_EXPOSED, 0) | np.where(seed, F_SEED, 0) | np.where(vic, F_VICINITY, 0) | \
        np.where(salted & present[:Lab], F_SALT, 0)
    rows[:, 3] = flags
    if details:
        return out, rows, dict(D2=D2, S2=S2, present=present, exposed=is_exposed, seed=seed, vicinity=vic, salt=salted)
    return out, rows
