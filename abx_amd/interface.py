"""Interface analysis of designs: the geometric half of what upstream takes from PyRosetta's InterfaceAnalyzerMover for every written
PDB and for the wild type (abx/metric.py:28-59, eval/traj_evaluate.py:242-261: dG_design, dG_wild, ddG).  Energies need a force field,
which this project does not have; buried solvent-accessible surface (dSASA_int), interface residues (nres_int) and antibody-antigen
contacts need none.  Side A is the antibody (rows < Lab), side B the FEATURISED antigen (rows >= Lab): when the complex was cropped
to a patch around the epitope, the antigen surface is that of the patch - the buried surface and the contacts are unaffected as long
as the patch holds every antigen atom near the antibody, `sasa_antigen` and `sasa_complex` are not those of the whole antigen.

Shrake-Rupley on a golden-spiral point set, heavy atoms of the atom14 slots with the project's van-der-Waals radii plus a probe, point
tests in float64 in a fixed IEEE operation order (include/abx_hip.h, AbxInterfaceArgs): the point counts of the device
(`InterfaceScorer`, abx_interface_scores, csrc/interface.hip) and of the host twin (`interface_host`, numpy) are equal integers."""
import functools

import numpy as np

from . import complex_view
from .complex_view import to_np

# The row of abx_interface_scores (include/abx_hip.h, ABX_IFACE_COLS)
INTERFACE_COLUMNS = ('sasa_complex', 'sasa_antibody', 'sasa_antigen', 'dsasa_int', 'dsasa_antibody', 'dsasa_region',
                     'n_res_int_antibody', 'n_res_int_antigen', 'n_res_int_region', 'n_contact', 'n_contact_region', 'n_atoms')
COUNT_COLUMNS = tuple(c for c in INTERFACE_COLUMNS if c.startswith('n_'))
# design minus wild type, the geometric analogue of ddG: the columns the driver writes a difference for
DELTA_COLUMNS = ('dsasa_int', 'dsasa_antibody', 'dsasa_region', 'n_contact', 'n_contact_region')
FOUR_PI = 12.566370614359172


# format_interface(row): %.2f for the areas (square Angstrom), integers for the counts; format_delta(row, wild): design minus wild type
# for DELTA_COLUMNS, signed
format_interface = functools.partial(complex_view.format_row, INTERFACE_COLUMNS, COUNT_COLUMNS, 2)
format_delta = functools.partial(complex_view.format_delta, INTERFACE_COLUMNS, COUNT_COLUMNS, DELTA_COLUMNS, 2)


def golden_spiral(P):
    """(P,3) float64 unit vectors: z = 1 - (2k + 1) / P, r = sqrt(1 - z^2), phi = k pi (3 - sqrt 5)."""
    P = int(P)
    if not 1 <= P <= 1024:
        raise ValueError(f'sphere points: P = {P} outside 1..1024')
    k = np.arange(P, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / P
    r = np.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.ascontiguousarray(np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1))


_SPHERE = {}


def sphere_points(P, device='cpu'):
    """golden_spiral(P) as a float64 tensor on `device` (cached per P and device: built on the host once, no trigonometry on the device)."""
    import torch
    key = (int(P), str(device))
    if key not in _SPHERE:
        _SPHERE[key] = torch.from_numpy(golden_spiral(P)).to(device).contiguous()
    return _SPHERE[key]


class InterfaceScorer(complex_view.ComplexView):
    """Interface rows of batches of designs of ONE complex on the device.  Built once per complex from its featurised batch (or the
    un-batched complex) like metrics.DesignScorer.  region: (L) mask of the rows the `*_region` columns count (default: the rows the
    sampler diffuses, sample 0's (1 - fixed_mask) * backbone mask).  n_points: sphere points per atom (128: two per lane of a wave);
    probe: probe radius; cutoff: contact distance of heavy atoms (Angstrom)."""

    COLUMNS = INTERFACE_COLUMNS
    takes_points = True                 # record(): sampler.sample_fn hands it the buffer that the SurfaceScorers built on it read

    def __init__(self, batch, region=None, n_points=128, probe=1.4, cutoff=4.0):
        super().__init__(batch)
        dev = self.gt_atom14.device
        self.region = complex_view.region_mask(batch, region, dev)
        self.sphere = sphere_points(n_points, dev)
        self.kw = dict(probe=float(probe), cutoff=float(cutoff))

    def score(self, atom14, seq, out=None, points=None, mask=None):
        """atom14 (B, Lab or L, 14, 3) f32 predicted coordinates (antibody only: the antigen is the ground truth's), seq (B, Lab) tokens
        -> (B, len(INTERFACE_COLUMNS)) float64 on the device; out: rows to write into (any row stride); points: (B,L,14,2) int32 to
        receive acc_alone / acc_cplx of every atom14 slot.  One call of abx_interface_scores, no host synchronisation."""
        from abx_amd import ops
        return ops.interface_scores(atom14, seq, self.gt_atom14, self.gt_seq, self.gt_exists, self.sphere, Lab=self.Lab, region=self.region,
                                    mask=mask, res_mask=self.res_mask, out=out, points=points, **self.kw)

    # wild(points=None): the counterpart of upstream's dG_wild - a design's row minus this one is the geometric analogue of ddG
    # record(): 'interface' and, with a relaxer, 'interface_relaxed'; three launches each


class SurfaceScorer(complex_view.ComplexView):
    """The base of the scorers that read the point counts of the interface analysis (polar.PolarScorer, developability.
    DevelopabilityScorer, shape.ShapeScorer, patches.PatchScorer): holds an InterfaceScorer of the complex and sees the complex through
    it.  interface: an existing InterfaceScorer of the same complex (None: one is built from region, n_points and probe) -
    `score(..., points=)` then takes the counts of ITS call for the same structures, so that the surface kernel runs once per structure
    set: sampler.sample_fn hands one buffer to every SurfaceScorer whose `.interface` is its `interface=` scorer.  region: (L) mask of the
    rows the `*_region` columns count (default: the interface scorer's)."""

    takes_points = True

    def __init__(self, batch, region, n_points, probe, interface):
        it = self.interface = interface if interface is not None else InterfaceScorer(batch, region=region, n_points=n_points, probe=probe)
        self.device = it.gt_atom14.device
        self.region = it.region if region is None else complex_view.region_mask(batch, region, self.device)
        self.Lab, self.L = it.Lab, it.L
        self.gt_atom14, self.gt_exists, self.gt_seq, self.res_mask = it.gt_atom14, it.gt_exists, it.gt_seq, it.res_mask

    def new_points(self, B):
        """An uninitialised (B, L, 14, 2) int32 tensor for the point counts of B structures."""
        import torch
        return torch.empty(B, self.L, 14, 2, dtype=torch.int32, device=self.device)

    def points_of(self, atom14, seq, points, mask):
        """`points`, or (None) the counts of these structures from a call of the surface kernel here."""
        if points is None:
            points = self.new_points(atom14.shape[0])
            self.interface.score(atom14, seq, points=points, mask=mask)
        return points

    # new_table(*lead), wild(**kw) - the row of the ground-truth complex itself with its own atoms: a design's row minus this one is what
    # the design gained or lost - and record() are ComplexView's


# -------------------------------------------------------------------------------------------------------------------
# host twin (float64, numpy)
# -------------------------------------------------------------------------------------------------------------------
def _radius_table():
    from abx_amd import ops
    return ops.vdw_radius_table('cpu').numpy().astype(np.float32)


def interface_host(x, mask, aa, Lab, region=None, n_points=128, probe=1.4, cutoff=4.0, chunk=256):
    """The row of abx_interface_scores for ONE structure on the host, with the same IEEE operations in the same order (no fused
    multiply-add: numpy multiplies and adds in separate passes).  x (L,14,3) coordinates (rounded to float32 first: what the kernel
    reads), mask (L,14) which slots exist, aa (L) residue tokens, Lab = rows of side A, region (L) or None.
    -> (row (len(INTERFACE_COLUMNS),) float64, points (L,14,2) int32: acc_alone, acc_cplx of every slot).
    Neighbours by a dense float64 distance matrix (N <= 14 L atoms) with the kernel's conservative prefilter, then the point tests
    of at most `chunk` atoms at a time on flat (pair, point) arrays."""
    x = to_np(x).astype(np.float32)
    L = x.shape[0]
    aa = np.clip(to_np(aa).astype(np.int64), 0, 20)
    rad = _radius_table()[aa]                                                   # (L,14) float32
    ok = (to_np(mask) != 0) & (rad > 0)
    region = np.zeros(L, bool) if region is None else (to_np(region) != 0)
    P = int(n_points)
    u = golden_spiral(P)
    probe, cutoff = float(probe), float(cutoff)
    rows, slots = np.nonzero(ok)                                                # slot order = the kernel's atom order
    N = rows.shape[0]
    c = x[rows, slots].astype(np.float64)                                       # (N,3)
    R = rad[rows, slots].astype(np.float64) + probe
    side = rows >= Lab
    alone, cplx, contacts = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros(N, np.int64)
    if N:
        dx, dy, dz = (c[:, None, k] - c[None, :, k] for k in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        del dx, dy, dz
        notme = ~np.eye(N, dtype=bool)
        cross = side[:, None] != side[None]
        contacts = (cross & (d2 < cutoff * cutoff) & ~side[:, None]).sum(1)     # counted on the side-A atom
        rs = (R[:, None] + R[None]) + 1e-3
        nb = notme & (d2 < rs * rs)
        del d2, rs
        ia, ib = np.nonzero(nb)                                                 # sorted by ia
        ptr = np.searchsorted(ia, np.arange(N + 1))
        px, py, pz = (c[:, k, None] + R[:, None] * u[None, :, k] for k in range(3))     # (N,P): multiply, then add
        Rb2 = R * R

        def points_of(a0, a1):
            lo, hi = ptr[a0], ptr[a1]
            own_hit = np.zeros((a1 - a0, P), np.int32)
            oth_hit = np.zeros((a1 - a0, P), np.int32)
            if hi > lo:
                pa, pb = ia[lo:hi], ib[lo:hi]
                ex, ey, ez = px[pa] - c[pb, 0, None], py[pa] - c[pb, 1, None], pz[pa] - c[pb, 2, None]
                hit = ((ex * ex + ey * ey) + ez * ez) < Rb2[pb, None]            # (pairs, P)
                is_other = cross[pa, pb][:, None]
                # per-atom sums over its pairs; a zero row at the end makes the start of a trailing atom without pairs a valid index
                pad = np.zeros((1, P), np.int32)
                start = ptr[a0:a1] - lo
                cnt = ptr[a0 + 1:a1 + 1] - ptr[a0:a1]
                own_hit = np.add.reduceat(np.concatenate([(hit & ~is_other).astype(np.int32), pad]), start, axis=0)
                oth_hit = np.add.reduceat(np.concatenate([(hit & is_other).astype(np.int32), pad]), start, axis=0)
                own_hit[cnt == 0] = 0
                oth_hit[cnt == 0] = 0
            free = own_hit == 0
            alone[a0:a1] = free.sum(1)
            cplx[a0:a1] = (free & (oth_hit == 0)).sum(1)

        # chunks of atoms whose (pair, point) arrays stay in cache (~2 MB each)
        per_atom = max(1, int(ptr[N]) // N) * P
        step = max(1, min(int(chunk), (1 << 18) // per_atom))
        for a0 in range(0, N, step):
            points_of(a0, min(a0 + step, N))
    unit = FOUR_PI * (R * R)
    area = lambda n: unit * n.astype(np.float64) / float(P)
    A_alone, A_cplx, A_bur = area(alone), area(cplx), area(alone - cplx)
    reg_atom = region[rows]
    touched = np.zeros(L, bool)
    touched[rows[alone > cplx]] = True
    row_side = np.arange(L) >= Lab
    out = np.array([A_cplx.sum(), A_alone[~side].sum(), A_alone[side].sum(), A_bur.sum(), A_bur[~side].sum(), A_bur[reg_atom].sum(),
                    (touched & ~row_side).sum(), (touched & row_side).sum(), (touched & region).sum(),
                    contacts.sum(), contacts[reg_atom].sum(), N], dtype=np.float64)
    points = np.zeros((L, 14, 2), np.int32)
    points[rows, slots, 0] = alone
    points[rows, slots, 1] = cplx
    return out, points
