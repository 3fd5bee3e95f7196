"""Shape complementarity of the interface: the Sc statistic of Lawrence & Colman (1993), the geometric filter that stands beside `dG` and
`dSASA` in every antibody pipeline (upstream's `sc_value` of PyRosetta's InterfaceAnalyzerMover).  Buried surface says that a loop
touches the antigen, Sc says whether the two surfaces FIT: for every dot of one partner's buried surface the nearest dot of the other
partner's, the two outward normals against each other, weighted down with the distance; the median over the dots, averaged over both
directions.  1 = perfectly matched surfaces; antibody-antigen interfaces in the literature sit near 0.64 - 0.68.

The surface is the CONTACT part of the molecular (Connolly) surface of each separated partner, made from the sphere points the
interface analysis already tests: no re-entrant (toroidal / concave) patches, no hydrogens, and the antigen is the featurised patch.
The value rises with the dot density (`n_points`): compare designs with the `wild` row at the same density, and use 512 points for
values comparable with the literature.

Every decision - which dot is buried, which is trimmed, which is the nearest - is taken in float64 in a fixed IEEE operation order
(include/abx_hip.h, AbxShapeArgs): the counts of the device (`ShapeScorer`, abx_shape_scores, csrc/shape.hip) and of the host twin
(`shape_host`, numpy) are equal, the medians agree to the few ulp by which `exp` and `sqrt` differ."""
import functools

import numpy as np

from . import complex_view
from .complex_view import to_np
from .interface import SurfaceScorer

# The row of abx_shape_scores (include/abx_hip.h, ABX_SHAPE_COLS)
SHAPE_COLUMNS = ('sc', 'sc_antibody', 'sc_antigen', 'sc_region', 'gap_antibody', 'gap_antigen', 'n_dots_antibody', 'n_dots_antigen',
                 'n_dots_region', 'n_trimmed_antibody', 'n_trimmed_antigen')
COUNT_COLUMNS = tuple(c for c in SHAPE_COLUMNS if c.startswith('n_'))
# design minus wild type: the columns the driver writes a difference for
DELTA_COLUMNS = ('sc', 'sc_antibody', 'sc_antigen', 'sc_region', 'n_dots_antibody', 'n_dots_antigen', 'n_dots_region')
PLACES = {None: 4, 'gap_antibody': 3, 'gap_antigen': 3}
SLACK = 1e-3                            # of the neighbour prefilter, as in interface_host

# format_shape(row): %.4f for Sc, %.3f for the gaps (Angstrom), integers for the counts; format_delta(row, wild): design minus wild type
format_shape = functools.partial(complex_view.format_row, SHAPE_COLUMNS, COUNT_COLUMNS, PLACES)
format_delta = functools.partial(complex_view.format_delta, SHAPE_COLUMNS, COUNT_COLUMNS, DELTA_COLUMNS, PLACES)


class ShapeScorer(SurfaceScorer):
    """Shape-complementarity rows of batches of designs of ONE complex on the device.  Built once per complex from its featurised batch
    (or the un-batched complex) like developability.DevelopabilityScorer, and holds an InterfaceScorer for the point counts
    (interface.SurfaceScorer: region - the rows `sc_region` / `n_dots_region` count -, n_points / probe of the surface, interface).
    trim: width of the peripheral band that is dropped (Angstrom); weight: of the squared distance in the exponent (1 / square Angstrom);
    max_dots: capacity of each of the four dot lists of a structure - a structure beyond it gets a row of -1."""

    COLUMNS = SHAPE_COLUMNS

    def __init__(self, batch, region=None, trim=1.5, weight=0.5, n_points=128, probe=1.4, max_dots=8192, interface=None):
        if not (trim >= 0 and weight >= 0 and int(max_dots) >= 1):
            raise ValueError(f'shape: needs trim >= 0, weight >= 0 and max_dots >= 1 (got {trim}, {weight}, {max_dots})')
        super().__init__(batch, region, n_points, probe, interface)
        self.kw = dict(trim=float(trim), weight=float(weight), probe=self.interface.kw['probe'], max_dots=int(max_dots))

    def score(self, atom14, seq, out=None, points=None, mask=None, j_chunk=0, workspace=None):
        """atom14 (B, Lab or L, 14, 3) f32 predicted coordinates, seq (B, Lab) tokens -> (B, len(SHAPE_COLUMNS)) float64 on the device;
        out: rows to write into (any row stride); points: the (B,L,14,2) int32 acc_alone / acc_cplx that the interface scorer returned
        for THESE structures (None: its kernel runs here); j_chunk: dots of the other side per LDS chunk of the match (0: the kernel's
        default); workspace: a uint8 tensor of at least ops.shape_workspace_bytes(B, L, P, max_dots) bytes (None: allocated here).
        No host synchronisation."""
        from abx_amd import ops
        points = self.points_of(atom14, seq, points, mask)
        return ops.shape_scores(atom14, seq, self.gt_atom14, self.gt_seq, self.gt_exists, self.interface.sphere, points, Lab=self.Lab,
                                region=self.region, mask=mask, res_mask=self.res_mask, out=out, j_chunk=j_chunk, workspace=workspace, **self.kw)

    # record(): 'shape' - the shape complementarity Sc of the interface, both directions, the designed residues' dots, the gaps and the
    # dot counts - and, with a relaxer, 'shape_relaxed'; five launches per table


# -------------------------------------------------------------------------------------------------------------------
# host twin (float64, numpy)
# -------------------------------------------------------------------------------------------------------------------
def median(v):
    """The median as the kernel takes it: v sorted ascending, the middle value or the mean of the two middle ones; 0 without values."""
    v = np.sort(np.asarray(v, np.float64))
    n = v.shape[0]
    if n == 0:
        return 0.0
    return float(v[(n - 1) // 2]) if n % 2 else float((v[n // 2 - 1] + v[n // 2]) * 0.5)


def _d2(a, b):
    """(len(a), len(b)) squared distances of two (n,3) float64 arrays: (dx*dx + dy*dy) + dz*dz with dx = a - b."""
    dx, dy, dz = (a[:, None, k] - b[None, :, k] for k in range(3))
    return (dx * dx + dy * dy) + dz * dz


def shape_host(x, mask, aa, Lab, region=None, points=None, trim=1.5, weight=0.5, n_points=128, probe=1.4, max_dots=8192, details=False):
    """The row of abx_shape_scores for ONE structure on the host, with the same IEEE operations in the same order (no fused
    multiply-add: numpy multiplies and adds in separate passes).  x (L,14,3) coordinates (rounded to float32 first: what the kernel
    reads), mask (L,14) which slots exist, aa (L) residue tokens, Lab = rows of side A, region (L) or None, points (L,14,2) acc_alone /
    acc_cplx of every slot (None: interface.interface_host computes them with n_points and probe).
    -> row (len(SHAPE_COLUMNS),) float64; eleven -1 when a list would exceed max_dots or the dots of an atom disagree with `points`.
    details=True adds a dict: 'n_buried', 'n_open', 'n_kept' (two integers each, antibody / antigen), 'S' and 'd2' (two arrays each,
    in list order), 'region' (bool per kept dot of the antibody), 'bad' (why the row is -1, or None)."""
    from .interface import _radius_table, golden_spiral, interface_host
    x = to_np(x).astype(np.float32)
    L, Lab = x.shape[0], int(Lab)
    aa = np.clip(to_np(aa).astype(np.int64), 0, 20)
    rad = _radius_table()[aa]                                                   # (L,14) float32
    ok = (to_np(mask) != 0) & (rad > 0)
    reg = np.zeros(L, bool) if region is None else (to_np(region) != 0)
    P = int(n_points)
    u = golden_spiral(P)
    probe, trim, weight = float(probe), float(trim), float(weight)
    if points is None:
        points = interface_host(x, ok, aa, Lab, region=region, n_points=P, probe=probe)[1]
    points = to_np(points).astype(np.int64)
    alone, cplx = points[..., 0], points[..., 1]
    minus = np.full(len(SHAPE_COLUMNS), -1.0)
    empty = dict(n_buried=(0, 0), n_open=(0, 0), n_kept=(0, 0), S=(np.zeros(0), np.zeros(0)), d2=(np.zeros(0), np.zeros(0)),
                 region=np.zeros(0, bool), bad=None)

    def give_up(why):
        return (minus, dict(empty, bad=why)) if details else minus

    if ((alone < 0) | (cplx < 0) | (alone > P) | (cplx > alone)).any() or ((alone > cplx) & ~ok).any():
        return give_up('points')
    rows, slots = np.nonzero(ok)                                                # slot order = the kernel's atom order
    c = x[rows, slots].astype(np.float64)                                       # (N,3)
    r = rad[rows, slots].astype(np.float64)
    R = r + probe
    side = rows >= Lab
    a_alone, a_cplx = alone[rows, slots], cplx[rows, slots]
    sel = np.nonzero(a_alone > a_cplx)[0]                                       # the interface atoms that `points` names
    n_bur = [int((a_alone - a_cplx)[sel][side[sel] == s].sum()) for s in (False, True)]
    n_open = [int(a_cplx[sel][side[sel] == s].sum()) for s in (False, True)]
    if max(n_bur + n_open) > int(max_dots):
        return give_up('max_dots')
    # ---- the dots of the interface atoms: the point test of interface_host, per (atom, point)
    I = [[], []]                                                                # per side: (position (n,3), point index, row)
    E = [[], []]
    for ia in sel:
        d2 = _d2(c[ia:ia + 1], c)[0]
        rs = (R[ia] + R) + SLACK
        nb = np.nonzero((d2 < rs * rs) & (np.arange(c.shape[0]) != ia))[0]
        px, py, pz = (c[ia, k] + R[ia] * u[:, k] for k in range(3))             # (P): multiply, then add
        ex, ey, ez = px[:, None] - c[None, nb, 0], py[:, None] - c[None, nb, 1], pz[:, None] - c[None, nb, 2]
        hit = ((ex * ex + ey * ey) + ez * ez) < (R[nb] * R[nb])[None]            # (P, neighbours)
        other = side[nb] != side[ia]
        surface = ~(hit & ~other[None]).any(1)
        buried = surface & (hit & other[None]).any(1)
        opened = surface & ~buried
        if int(buried.sum()) != a_alone[ia] - a_cplx[ia] or int(opened.sum()) != a_cplx[ia]:
            return give_up('points')
        m = np.stack([c[ia, k] + r[ia] * u[:, k] for k in range(3)], 1)         # (P,3) positions on the van-der-Waals sphere
        s = int(side[ia])
        for which, lst in ((buried, I), (opened, E)):
            p = np.nonzero(which)[0]
            lst[s].append((m[p], p, np.full(p.shape[0], rows[ia])))
    cat = lambda parts: (np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts]), np.concatenate([q[2] for q in parts])) \
        if parts else (np.zeros((0, 3)), np.zeros(0, np.int64), np.zeros(0, np.int64))
    I, E = [cat(q) for q in I], [cat(q) for q in E]
    # ---- trimming: a buried dot within `trim` of an open dot of its own side goes
    T = []
    for s in (0, 1):
        pos, p, row = I[s]
        keep = np.ones(pos.shape[0], bool)
        if pos.shape[0] and E[s][0].shape[0]:
            keep = ~(_d2(pos, E[s][0]) < trim * trim).any(1)
        T.append((pos[keep], p[keep], row[keep]))
    # ---- match: the nearest kept dot of the other side, ties to the lowest list index
    S, D2 = [], []
    for s in (0, 1):
        (pos, p, _), (opos, op, _) = T[s], T[1 - s]
        if pos.shape[0] == 0 or opos.shape[0] == 0:
            S.append(np.zeros(0))
            D2.append(np.zeros(0))
            continue
        d2 = _d2(pos, opos)
        j = d2.argmin(1)
        dmin = d2[np.arange(pos.shape[0]), j]
        ui, uj = u[p], u[op[j]]
        dot = (ui[:, 0] * uj[:, 0] + ui[:, 1] * uj[:, 1]) + ui[:, 2] * uj[:, 2]
        S.append(-dot * np.exp(-(weight * dmin)))
        D2.append(dmin)
    in_reg = reg[T[0][2]]
    out = np.zeros(len(SHAPE_COLUMNS), np.float64)
    out[1], out[2] = median(S[0]), median(S[1])
    out[0] = (out[1] + out[2]) * 0.5
    out[3] = median(S[0][in_reg]) if S[0].shape[0] else 0.0
    out[4], out[5] = np.sqrt(median(D2[0])), np.sqrt(median(D2[1]))
    out[6], out[7] = T[0][0].shape[0], T[1][0].shape[0]
    out[8] = in_reg.sum()
    out[9], out[10] = n_bur[0] - out[6], n_bur[1] - out[7]
    if details:
        return out, dict(n_buried=tuple(n_bur), n_open=tuple(n_open), n_kept=(int(out[6]), int(out[7])), S=tuple(S), d2=tuple(D2),
                         region=in_reg, bad=None)
    return out
