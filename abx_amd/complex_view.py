"""One complex as the per-design analyses see it, and the pieces their scorers share (metrics.DesignScorer, relax.ViolationRelaxer,
interface.InterfaceScorer and the interface.SurfaceScorer classes on its point counts - polar.PolarScorer,
developability.DevelopabilityScorer, shape.ShapeScorer, patches.PatchScorer -, accuracy.AccuracyScorer, confidence.DistogramScorer,
torsions.TorsionScorer, secondary.SecondaryScorer): the extraction of the complex from a featurised batch, the default region, the
result tables, the wild-type row, what a scorer adds to the sampler's last record, the TSV formatting of a row and the conversions that
open the host twins.  The device side of the same conventions is csrc/structure_dev.h; ops._structure_args passes one to the other."""
import numpy as np
import torch


def to_np(t):
    """A tensor (on any device) or an array-like as a numpy array: what every host twin reads its arguments through."""
    return t.detach().cpu().numpy() if hasattr(t, 'detach') else np.asarray(t)


def type_index(letter):
    """The token of a one-letter residue type."""
    from . import residue_constants as rc
    return rc.restypes.index(letter)


class Borderline:
    """Counts the decisions `lhs ? rhs` of a host twin whose two sides differ by less than 1e-9 relative (of the size of the operands)."""

    def __init__(self):
        self.n = 0

    def __call__(self, lhs, rhs, scale, where=True):
        near = np.abs(lhs - rhs) < 1e-9 * np.maximum(np.abs(scale), 1e-300)
        self.n += int(np.count_nonzero(near & where))


def one_of(batch):
    """k -> batch[k] of ONE complex: sample 0 of a featurised batch, or the un-batched complex itself."""
    return (lambda k: batch[k][0]) if batch['seq'].dim() == 2 else (lambda k: batch[k])


def region_mask(batch, region, device):
    """(L) uint8 mask from `region`, or the default: the rows the sampler diffuses, sample 0's (1 - fixed_mask) * backbone mask."""
    if region is None:
        one = one_of(batch)
        region = (1 - one('fixed_mask')) * one('atom14_gt_exists')[..., 0]
    return (torch.as_tensor(region).to(device) != 0).to(torch.uint8).contiguous()


def new_table(columns, device, *lead):
    """An uninitialised (*lead, len(columns)) float64 table on `device` for `score(..., out=table[i])`."""
    return torch.empty(*lead, len(columns), dtype=torch.float64, device=device)


class ComplexView:
    """The ground truth of ONE complex on its device: Lab = the antibody length, gt_atom14 (L,14,3) f32, gt_exists (L,14) uint8,
    gt_seq (L) int64, res_mask (L) uint8 or None; with chains: chain_id (L) int32 and residx (L) int32 (None without link_by_residx:
    array neighbours are then linked by chain id alone); with cdr: cdr_def (L) int32.  A scorer names its row in COLUMNS."""
    COLUMNS = ()
    want_rows = False                   # set on an instance: the design's record also carries the per-residue tables of side_outputs
    takes_points = False                # score(..., points=): the (B,L,14,2) point counts of the surface kernel, written or read

    def __init__(self, batch, chains=False, link_by_residx=True, cdr=False):
        one = one_of(batch)
        self.Lab = int(batch['anchor_flag'].shape[-1])
        self.gt_atom14 = one('atom14_gt_positions').to(torch.float32).contiguous()
        self.gt_exists = one('atom14_gt_exists').to(torch.uint8).contiguous()
        self.gt_seq = one('seq').to(torch.int64).contiguous()
        self.res_mask = one('mask').to(torch.uint8).contiguous() if 'mask' in batch else None
        self.L = int(self.gt_seq.shape[0])
        if cdr:
            self.cdr_def = one('cdr_def').to(torch.int32).contiguous()
        if chains:
            self.chain_id = one('chain_id').to(torch.int32).contiguous()
            self.residx = one('residx').to(torch.int32).contiguous() if link_by_residx and 'residx' in batch else None

    def new_table(self, *lead):
        """An uninitialised (*lead, len(COLUMNS)) float64 table on the complex's device for `score(..., out=table[i])`."""
        return new_table(self.COLUMNS, self.gt_atom14.device, *lead)

    def wild(self, **kw):
        """(1, len(COLUMNS)): the row of the ground-truth complex itself with its own atoms; kw: the optional outputs of score()."""
        return self.score(self.gt_atom14[None, :self.Lab], self.gt_seq[None, :self.Lab], mask=self.gt_exists[None], **kw)

    def side_outputs(self, B):
        """{keyword of score(): an uninitialised tensor for B structures}: what the record of the designs carries beside their row."""
        return {}

    def record(self, rec, key, atom14, seq, design=True, points=None, **context):
        """What sampler.sample_fn adds to its last record for this scorer: rec[key] = the (B, len(COLUMNS)) float64 rows of the structures
        atom14; design: they are the designs themselves, not their relaxed structures, and rec[f'{key}_{k}'] receives the side_outputs.
        points: the point counts that the scorers of one surface share (takes_points), or None; context: what other scorers read - the
        model's output `out` and the per-residue `plddt` of the last network call.  Launches only, no host synchronisation."""
        side = self.side_outputs(atom14.shape[0]) if design else {}
        rec.update({f'{key}_{k}': v for k, v in side.items()})
        rec[key] = self.score(atom14, seq, **side, **({'points': points} if self.takes_points else {}))


def _places(places, column):
    return places.get(column, places[None]) if isinstance(places, dict) else places


def format_row(columns, count_columns, places, row):
    """One row as TSV fields: integers for count_columns, fixed point for the rest.  places: the decimals, or {column: decimals}
    with the default under None."""
    return [str(int(v)) if c in count_columns else f'{float(v):.{_places(places, c)}f}' for c, v in zip(columns, row)]


def format_delta(columns, count_columns, delta_columns, places, row, base):
    """row minus base for delta_columns, signed, at the precision of format_row."""
    out = []
    for c in delta_columns:
        k = columns.index(c)
        d = float(row[k]) - float(base[k])
        out.append(f'{int(round(d)):+d}' if c in count_columns else f'{d:+.{_places(places, c)}f}')
    return out
