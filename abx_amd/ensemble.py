"""Ensemble analysis of the designs of one complex: how many different loops are these, which are the same answer twice, which few go
on to the expensive evaluation.  Every other analysis of this package (metrics, relax, interface) describes one design alone; this one
compares each design with every other: RMSD of the designed residues after the optimal proper rotation (`rmsd_fit`, the Kabsch
convention of abx/utils.py:444-465: shape), RMSD without any superposition (`rmsd_frame`: all designs share the frame of the complex,
placement) and the number of differing designed residues (`seq_diff`), then clusters by the Daura / GROMOS rule (Daura et al. 1999: the
design with the most unassigned neighbours within the cutoff becomes a centre, takes them, repeat) and one summary row per design.

On the device: `EnsembleAnalyzer` (abx_ensemble_pairs + abx_ensemble_cluster, csrc/ensemble.hip).  `ensemble_host` is the numpy float64
twin; its rmsd_fit goes through `abx_amd.metrics.kabsch`."""
import numpy as np

from .complex_view import to_np

# The row of abx_ensemble_cluster (include/abx_hip.h, ABX_ENS_COLS)
ENSEMBLE_COLUMNS = ('cluster', 'is_centre', 'n_neighbours', 'rmsd_fit_mean', 'rmsd_fit_min', 'rmsd_frame_mean', 'rmsd_frame_min',
                    'seq_diff_mean', 'n_same_seq', 'first_same_seq')
COUNT_COLUMNS = ('cluster', 'is_centre', 'n_neighbours', 'n_same_seq', 'first_same_seq')
SUMMARY_COLUMNS = ('n_designs', 'n_clusters', 'largest_cluster', 'n_unique_seq', 'rmsd_fit_mean', 'rmsd_frame_mean', 'seq_diff_mean',
                   'seq_identity_mean')
METRICS = {'fit': 0, 'frame': 1}
ATOMS = {'ca': 1, 'backbone': 4}
MAX_POINTS, MAX_N = 512, 1024


def format_ensemble(row):
    """One row as TSV fields: integers for the counts and indices, %.4f for the others (nan for a single design)."""
    return [str(int(v)) if c in COUNT_COLUMNS else f'{float(v):.4f}' for c, v in zip(ENSEMBLE_COLUMNS, row)]


def summary(table, n_region=None):
    """The ensemble in one line, from the (N, len(ENSEMBLE_COLUMNS)) table: an OrderedDict over SUMMARY_COLUMNS.  The means of the
    per-design means are the means over all pairs (every row averages over the same N - 1 others).  n_region: the number of compared
    residues M, for seq_identity_mean = 1 - seq_diff_mean / M (nan without it)."""
    from collections import OrderedDict
    t = np.asarray(table, dtype=np.float64).reshape(-1, len(ENSEMBLE_COLUMNS))
    N = t.shape[0]
    sizes = np.bincount(t[:, 0].astype(np.int64))
    mean = lambda k: float(t[:, k].mean()) if N > 1 else float('nan')
    sd = mean(7)
    return OrderedDict([('n_designs', N), ('n_clusters', int(sizes.shape[0])), ('largest_cluster', int(sizes.max())),
                        ('n_unique_seq', int((t[:, 9] == np.arange(N)).sum())),
                        ('rmsd_fit_mean', mean(3)), ('rmsd_frame_mean', mean(5)), ('seq_diff_mean', sd),
                        ('seq_identity_mean', 1.0 - sd / n_region if n_region else float('nan'))])


def format_summary(s):
    return [str(int(v)) if c.startswith('n_') or c == 'largest_cluster' else f'{float(v):.4f}' for c, v in s.items()]


def _check(atoms, metric, cutoff):
    if atoms not in ATOMS:
        raise ValueError(f'atoms: {atoms!r} is none of {sorted(ATOMS)}')
    if metric not in METRICS:
        raise ValueError(f'metric: {metric!r} is none of {sorted(METRICS)}')
    if not float(cutoff) >= 0.0:
        raise ValueError(f'cutoff: {cutoff!r} must be >= 0')


class EnsembleAnalyzer:
    """Compares the designs of ONE complex on the device.  Built once per complex from its featurised batch (or the un-batched complex)
    like interface.InterfaceScorer.  region: (L) or (Lab) mask of the compared rows (default: the rows the sampler diffuses, sample
    0's (1 - fixed_mask) * backbone mask, below Lab); atoms: 'backbone' (N, CA, C, O) or 'ca'; metric: the plane the clusters are
    built on, 'fit' or 'frame'; cutoff: the neighbour distance (Angstrom)."""

    def __init__(self, batch, region=None, atoms='backbone', metric='fit', cutoff=1.0):
        import torch
        _check(atoms, metric, cutoff)
        one = (lambda k: batch[k][0]) if batch['seq'].dim() == 2 else (lambda k: batch[k])
        self.Lab = int(batch['anchor_flag'].shape[-1])
        if region is None:
            region = (1 - one('fixed_mask')) * one('atom14_gt_exists')[..., 0]
        dev = one('seq').device
        self.region = (torch.as_tensor(region).to(dev)[:self.Lab] != 0).to(torch.uint8).contiguous()
        self.n_region = int(self.region.sum())                 # once per complex (the only host synchronisation)
        self.atoms, self.metric, self.cutoff = ATOMS[atoms], METRICS[metric], float(cutoff)
        if not 1 <= self.n_region * self.atoms <= MAX_POINTS:
            raise ValueError(f'{self.n_region} compared residues x {self.atoms} atoms: outside 1..{MAX_POINTS} points')

    def pairs(self, atom14, seq):
        """atom14 (N, >= Lab, 14, 3) f32, seq (N, >= Lab) tokens -> (3, N, N) float64 on the device: rmsd_fit, rmsd_frame, seq_diff."""
        from abx_amd import ops
        return ops.ensemble_pairs(atom14[:, :self.Lab], seq, self.region, atoms=self.atoms, n_region=self.n_region)

    def analyze(self, atom14, seq):
        """-> dict(table (N, len(ENSEMBLE_COLUMNS)) float64, centres (N) int32 padded with -1, n_clusters (1) int32, planes (3,N,N)),
        all on the device: two C calls, no host synchronisation before the caller reads."""
        from abx_amd import ops
        if atom14.shape[0] > MAX_N:
            raise ValueError(f'{atom14.shape[0]} designs: the clusters are built for at most {MAX_N}')
        planes = self.pairs(atom14, seq)
        table, centres, n_clusters = ops.ensemble_cluster(planes, metric=self.metric, cutoff=self.cutoff)
        return dict(table=table, centres=centres, n_clusters=n_clusters, planes=planes)


# -------------------------------------------------------------------------------------------------------------------
# host twin (float64, numpy)
# -------------------------------------------------------------------------------------------------------------------
def cluster_host(d, cutoff):
    """The Daura / GROMOS rule on the (N,N) matrix d, as a literal loop -> (cluster (N) int64, centres list)."""
    d = np.asarray(d, dtype=np.float64)
    N = d.shape[0]
    nb = (d <= cutoff) & ~np.eye(N, dtype=bool)
    cluster = np.full(N, -1, np.int64)
    centres = []
    while (cluster < 0).any():
        free = cluster < 0
        count = np.where(free, (nb & free[None]).sum(1), -1)
        c = int(np.argmax(count))                               # the first of the largest: ties go to the lowest index
        cluster[free & (nb[c] | (np.arange(N) == c))] = len(centres)
        centres.append(c)
    return cluster, centres


def table_host(planes, metric='fit', cutoff=1.0):
    """The rows of abx_ensemble_cluster from (3,N,N) planes on the host -> (table (N, cols) float64, centres list)."""
    planes = np.asarray(planes, dtype=np.float64)
    N = planes.shape[1]
    cluster, centres = cluster_host(planes[METRICS[metric]], cutoff)
    t = np.zeros((N, len(ENSEMBLE_COLUMNS)))
    for i in range(N):
        oth = np.arange(N) != i
        fit, frame, sd = planes[0, i, oth], planes[1, i, oth], planes[2, i, oth]
        same = np.nonzero(planes[2, i] == 0)[0]
        stats = [fit.mean(), fit.min(), frame.mean(), frame.min(), sd.mean()] if N > 1 else [np.nan] * 5
        t[i] = [cluster[i], float(centres[cluster[i]] == i), (planes[METRICS[metric], i, oth] <= cutoff).sum()] + stats + \
               [(sd == 0).sum(), same.min()]                   # (the diagonal is 0: the design itself is among `same`)
    return t, centres


def ensemble_host(x, seq, region, atoms='backbone', metric='fit', cutoff=1.0):
    """What EnsembleAnalyzer.analyze computes, on the host in float64: x (N, L, 14, 3) coordinates (rounded to float32 first: what the
    kernel reads), seq (N, >= L) tokens, region (<= L) mask of the compared rows.
    -> dict(planes (3,N,N), table (N, cols), centres (N) int32 padded with -1, n_clusters).  rmsd_fit: metrics.kabsch of the two
    point sets, then the root mean square of the aligned difference."""
    from abx_amd.metrics import kabsch
    _check(atoms, metric, cutoff)
    x = to_np(x).astype(np.float32).astype(np.float64)
    seq = to_np(seq).astype(np.int64)
    rows = np.nonzero(to_np(region) != 0)[0]
    rows = rows[rows < x.shape[1]]
    N = x.shape[0]
    pts = (x[:, rows, 1:2] if ATOMS[atoms] == 1 else x[:, rows, :4]).reshape(N, -1, 3)            # (N,P,3), residue order
    if not 1 <= pts.shape[1] <= MAX_POINTS:
        raise ValueError(f'{pts.shape[1]} points: outside 1..{MAX_POINTS}')
    planes = np.zeros((3, N, N))
    for i in range(N):
        for j in range(i + 1, N):
            a, b = kabsch(pts[i].T, pts[j].T)
            planes[0, i, j] = planes[0, j, i] = np.sqrt(np.mean(np.sum(np.square(a - b), axis=0)))
            planes[1, i, j] = planes[1, j, i] = np.sqrt(np.mean(np.sum(np.square(pts[i] - pts[j]), axis=1)))
            planes[2, i, j] = planes[2, j, i] = (seq[i, rows] != seq[j, rows]).sum()
    table, centres = table_host(planes, metric, cutoff)
    cen = np.full(N, -1, np.int32)
    cen[:len(centres)] = centres
    return dict(planes=planes, table=table, centres=cen, n_clusters=len(centres))
