"""Confidence of designs from the network's distogram head: what the pair representation of the LAST network call predicts about the
pseudo-beta distances of a design, and how well the structure the network emitted agrees with it (a self-consistency score).

Upstream trains the head with every checkpoint (`impl.distogram.proj`, abx/model/head.py:26-44: logits = 0.5 (x + x^T), x = proj(pair),
64 bins between first_break and last_break) and turns it into contact predictions at 8 A (MetricDictHead, head.py:90-113: pred =
sum softmax(logits)[..., :t+1], t = #{breaks <= cutoff}).  At the headline shape the logits are 3.2 GB that exist only to be reduced
again, so `DistogramScorer` never forms them: abx_distogram_scores (csrc/distogram.hip, include/abx_hip.h AbxDistogramArgs) projects,
symmetrises, takes the softmax and reduces in one kernel.  `distogram_host` is its float64 twin on the host (numpy; no GPU)."""
import functools

import numpy as np

from . import complex_view
from .complex_view import to_np

# The row of abx_distogram_scores (include/abx_hip.h, ABX_DISTO_COLS).  region = the designed rows; pairs are ordered, i != j, both valid.
CONFIDENCE_COLUMNS = ('nll_all', 'nll_antibody_antigen', 'nll_region', 'nll_region_antigen', 'dist_err_region', 'entropy_region',
                      'exp_contacts_region_antigen', 'n_contacts_region_antigen', 'p_on_contacts_region_antigen', 'n_pairs_region')
COUNT_COLUMNS = ('n_contacts_region_antigen', 'n_pairs_region')
# design minus wild type: the columns the driver writes a difference for
DELTA_COLUMNS = ('nll_all', 'nll_antibody_antigen', 'nll_region', 'nll_region_antigen', 'exp_contacts_region_antigen',
                 'n_contacts_region_antigen')
# per residue (the `rows` of abx_distogram_scores)
ROW_COLUMNS = ('nll_mean', 'exp_contacts_antigen', 'n_contacts_antigen', 'entropy_mean')
ANTIBODY, ANTIGEN, DESIGNED = 1, 2, 4          # ABX_DISTO_* class bits
GLY = 7                                        # residue_constants.restype_order['G']
MAX_LOGITS_BYTES = 1 << 30


def format_confidence(row):
    """One row as TSV fields: %.4f for the values, integers for the counts."""
    return [str(int(round(float(v)))) if c in COUNT_COLUMNS else f'{float(v):.4f}' for c, v in zip(CONFIDENCE_COLUMNS, row)]


# format_delta(row, wild): design minus wild type for DELTA_COLUMNS, signed
format_delta = functools.partial(complex_view.format_delta, CONFIDENCE_COLUMNS, COUNT_COLUMNS, DELTA_COLUMNS, 4)


def distogram_breaks(conf=None):
    """(breaks, squared breaks) as fp32 host tensors, as upstream builds them (head.py:34; the squares as common_modules.py:108-109)."""
    import torch
    if conf is None:
        from abx_amd.config import default_config
        conf = default_config().model.heads.distogram
    breaks = torch.linspace(conf.first_break, conf.last_break, steps=conf.num_bins - 1)
    return breaks, torch.square(breaks)


def bin_centres(breaks):
    """(64) float64: bin k holds (breaks[k-1], breaks[k]]; the midpoint, the two open end bins extended by half a step."""
    b = np.asarray(breaks, dtype=np.float32).astype(np.float64)
    return np.concatenate([[b[0] - 0.5 * (b[1] - b[0])], 0.5 * (b[:-1] + b[1:]), [b[-1] + 0.5 * (b[-1] - b[-2])]])


def pseudo_beta(atom14, seq):
    """atom14 (..., L, 14, 3), seq (..., L) tokens -> (..., L, 3): CB (slot 4), CA (slot 1) for Gly (common_modules.py:85-96)."""
    import torch
    return torch.where((seq == GLY)[..., None], atom14[..., 1, :], atom14[..., 4, :])


class DistogramScorer(complex_view.ComplexView):
    """Confidence rows of batches of designs of ONE complex on the device.  Built once per complex from its featurised batch (or the
    un-batched complex) like interface.InterfaceScorer: the antigen rows (>= Lab) come from the ground-truth atom14, the antibody rows
    from the design; the pseudo-beta atom is CB, or CA for a Gly of the design's own `seq`.  params_or_model: a state dict or a module
    holding `impl.distogram.proj.{weight,bias}`.  region: (L) mask of the designed rows (default: the rows the sampler diffuses, sample
    0's (1 - fixed_mask) * backbone mask); cutoff: contact distance of the pseudo-beta atoms (Angstrom)."""

    COLUMNS = CONFIDENCE_COLUMNS
    want_planes = False                 # set on an instance: sampler.sample_fn also records 'confidence_planes'

    def __init__(self, batch, params_or_model, region=None, cutoff=8.0, conf=None):
        import torch
        from abx_amd import ops
        super().__init__(batch)
        L, dev = self.L, self.gt_atom14.device
        self.device = dev
        self.gt_exists = self.gt_exists.ne(0)               # (this scorer's masks are bool: they are combined on the host side of the call)
        self.res_mask = self.res_mask.ne(0) if self.res_mask is not None else torch.ones(L, dtype=torch.bool, device=dev)
        region = complex_view.region_mask(batch, region, dev)
        cls = torch.full((L,), ANTIGEN, dtype=torch.uint8, device=dev)
        cls[:self.Lab] = ANTIBODY
        self.classes = (cls | (region * DESIGNED)).contiguous()
        sd = params_or_model.state_dict() if hasattr(params_or_model, 'state_dict') else params_or_model
        self.weight = sd['impl.distogram.proj.weight'].detach().to(dev, torch.float32).contiguous()
        self.bias = sd['impl.distogram.proj.bias'].detach().to(dev, torch.float32).contiguous()
        self.w_packed = ops.distogram_pack_weight(self.weight)
        breaks, sq = distogram_breaks(conf)
        assert breaks.numel() == 63, 'the kernel is built for 64 bins'
        self.breaks, self.sq_breaks = breaks.to(dev), sq.to(dev)
        self.cutoff = float(cutoff)

    def inputs(self, atom14, seq, wild=False):
        """(pb (B,L,3) f32, valid (B,L) bool) of designs atom14 (B, Lab or L, 14, 3) / seq (B, >= Lab): antigen rows from the ground truth.
        wild: the antibody rows are the ground truth's too, valid where its pseudo-beta atom exists (a design has every atom)."""
        import torch
        B, Lab = atom14.shape[0], self.Lab
        x = torch.cat([atom14[:, :Lab].to(torch.float32), self.gt_atom14[None, Lab:].expand(B, -1, -1, -1)], dim=1)
        tok = torch.cat([seq[:, :Lab].to(torch.int64), self.gt_seq[None, Lab:].expand(B, -1)], dim=1)
        pb = pseudo_beta(x, tok).contiguous()
        gly = tok == GLY
        have = torch.where(gly, self.gt_exists[None, :, 1], self.gt_exists[None, :, 4])
        if not wild:
            have = have.clone()
            have[:, :Lab] = True
        return pb, (have & self.res_mask[None]).contiguous()

    def score(self, pair, atom14, seq, out=None, wild=False, planes=False):
        """pair (B,L,L,192) f32: representations['pair'] of the network call that produced the designs (overwritten by the next call:
        score right after it).  -> (table (B, len(CONFIDENCE_COLUMNS)) float64, rows (B, L, len(ROW_COLUMNS)) float64) on the device.
        Two launches, no host synchronisation."""
        from abx_amd import ops
        pb, valid = self.inputs(atom14, seq, wild)
        table, rows, pl = ops.distogram_scores(pair, self.w_packed, self.bias, self.breaks, self.sq_breaks, pb, self.classes, valid,
                                               cutoff=self.cutoff, table=out, rows=True, planes=planes)
        return (table, rows, pl) if planes else (table, rows)

    def planes(self, pair, atom14, seq):
        """(p_contact, exp_dist): (B,L,L) f32 planes of every residue pair, exactly symmetric."""
        return self.score(pair, atom14, seq, planes=True)[2]

    def wild(self, pair):
        """(table (B,10), rows): the input complex's own coordinates scored against the same predictions."""
        B = pair.shape[0]
        return self.score(pair, self.gt_atom14[None].expand(B, -1, -1, -1), self.gt_seq[None].expand(B, -1), wild=True)

    def record(self, rec, key, atom14, seq, design=True, out=None, **context):
        """ComplexView.record: 'confidence' and, for the designs, 'confidence_rows' (B, L, 4) - the distogram head of the last network call
        against the designs it emitted -, 'confidence_wild' (the input complex's own coordinates against the same predictions) and with
        want_planes 'confidence_planes' = (p_contact, exp_dist); with a relaxer 'confidence_relaxed'.  Reads out['representations']['pair']
        of the call just made (the next call overwrites that buffer: model/abx.py:16-18, and nothing between it and here runs the
        network); two launches per table."""
        pair = out['representations']['pair']
        if not design:
            rec[key] = self.score(pair, atom14, seq)[0]
            return
        got = self.score(pair, atom14, seq, planes=bool(self.want_planes))
        rec[key], rec[key + '_rows'] = got[0], got[1]
        if len(got) > 2:
            rec[key + '_planes'] = got[2]
        rec[key + '_wild'] = self.wild(pair)[0]

    def logits(self, pair, samples):
        """{'logits': (n,L,L,64) f32, 'breaks': (63) f32} of the designs `samples` (indices into the batch), the layout of upstream's
        heads['distogram'] (head.py:44).  For a few designs: an output above 1 GiB is refused."""
        import torch
        from abx_amd import ops
        samples = [int(s) for s in samples]
        size = len(samples) * self.L * self.L * 64 * 4
        if size > MAX_LOGITS_BYTES:
            raise ValueError(f'distogram logits of {len(samples)} designs at L = {self.L} take {size} bytes ({size / 2**30:.2f} GiB), above the '
                             f'limit of 1 GiB: ask for fewer designs, or use score() / planes(), which never form them')
        z = pair[torch.as_tensor(samples, dtype=torch.int64, device=pair.device)]
        return {'logits': ops.distogram_logits(z, self.w_packed, self.bias), 'breaks': self.breaks}

    def host(self, pair, atom14, seq, wild=False):
        """distogram_host on this scorer's set-up (float64 twin; everything is copied to the host)."""
        pb, valid = self.inputs(atom14, seq, wild)
        return distogram_host(pair, self.weight, self.bias, self.breaks, pb, self.classes, valid, self.cutoff)


# -------------------------------------------------------------------------------------------------------------------
# host twin (float64, numpy)
# -------------------------------------------------------------------------------------------------------------------
def distogram_host(pair, W, b, breaks, pb, classes, valid, cutoff=8.0):
    """abx_distogram_scores / abx_distogram_logits on the host.  pair (B,L,L,192), W (64,192) torch Linear.weight, b (64), breaks (63),
    pb (B,L,3), classes (L) class bits, valid (B,L).  The operand is symmetrised in fp32 exactly as on the device, 0.5f * (a + b), and the
    realised bin and contact are taken in fp32 in the kernel's operation order (numpy multiplies and adds in separate passes: no
    fused multiply-add); everything else is float64.  -> dict: logits (B,L,L,64) f64, bound_scale (B,L,L,64) f64 = sum_k |zs_k W_kn| +
    |b_n| (what the fp32 dot-product bound multiplies), d2 (B,L,L) f32, bin_real, contact, ok (the pair sets' base: i != j, both
    valid), nll, entropy, p_contact, exp_dist (B,L,L) f64, table (B, len(CONFIDENCE_COLUMNS)), rows (B, L, len(ROW_COLUMNS))."""
    z = to_np(pair).astype(np.float32)
    B, L = z.shape[:2]
    W64, b64 = to_np(W).astype(np.float32).astype(np.float64), to_np(b).astype(np.float32).astype(np.float64)
    brk = to_np(breaks).astype(np.float32)
    zs = np.float32(0.5) * (z + z.transpose(0, 2, 1, 3))
    zs64 = zs.astype(np.float64)
    logits = zs64 @ W64.T + b64
    bound_scale = np.abs(zs64) @ np.abs(W64).T + np.abs(b64)
    p3 = to_np(pb).astype(np.float32)
    dx, dy, dz = (p3[:, :, None, k] - p3[:, None, :, k] for k in range(3))
    d2 = (dx * dx + dy * dy) + dz * dz                                          # fp32, each operation rounded on its own
    sqb = brk * brk
    bin_real = (d2[..., None] > sqb).sum(-1)
    cut = np.float32(cutoff)
    contact = d2 < cut * cut
    t = int((brk <= cut).sum())
    cen = bin_centres(brk)
    x = logits - logits.max(-1, keepdims=True)
    e = np.exp(x)
    s = e.sum(-1)
    lns = np.log(s)
    nll = lns - np.take_along_axis(x, bin_real[..., None], -1)[..., 0]
    entropy = lns - (e * x).sum(-1) / s
    p_contact = e[..., :t + 1].sum(-1) / s
    exp_dist = (e * cen).sum(-1) / s
    cls = to_np(classes).astype(np.int64)
    v = to_np(valid) != 0
    ok = v[:, :, None] & v[:, None, :] & ~np.eye(L, dtype=bool)[None]
    ab, ag, des = ((cls & m) != 0 for m in (ANTIBODY, ANTIGEN, DESIGNED))
    okag = ok & ag[None, None, :]
    within = ok & (bin_real < brk.shape[0])
    d_real = np.sqrt(d2.astype(np.float64))

    def tot(val, sel):
        return np.where(sel, val, 0.0).sum((1, 2))

    def mean(val, sel):
        n = sel.sum((1, 2))
        return np.where(n > 0, tot(val, sel) / np.maximum(n, 1), 0.0)

    ri_ab, ri_des = ab[None, :, None], des[None, :, None]
    con = okag & ri_des & contact
    table = np.stack([mean(nll, ok), mean(nll, okag & ri_ab), mean(nll, ok & ri_des), mean(nll, okag & ri_des),
                      mean(np.abs(exp_dist - d_real), within & ri_des), mean(entropy, ok & ri_des),
                      tot(p_contact, okag & ri_des), con.sum((1, 2)).astype(np.float64), mean(p_contact, con),
                      (ok & ri_des).sum((1, 2)).astype(np.float64)], axis=1)
    n_i = ok.sum(2)
    rmean = lambda val: np.where(n_i > 0, np.where(ok, val, 0.0).sum(2) / np.maximum(n_i, 1), 0.0)
    rows = np.stack([rmean(nll), np.where(okag, p_contact, 0.0).sum(2), (okag & contact).sum(2).astype(np.float64), rmean(entropy)], axis=2)
    return dict(logits=logits, bound_scale=bound_scale, d2=d2, bin_real=bin_real, contact=contact, ok=ok, nll=nll, entropy=entropy,
                p_contact=p_contact, exp_dist=exp_dist, table=table, rows=rows)
