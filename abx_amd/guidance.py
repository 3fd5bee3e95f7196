"""Opt-in structural-violation guidance of the reverse process (BASELINE config 4 "guidance-gradient terms on"; SURVEY.md §8a
row G, §8f-4).  The reference samples WITHOUT guidance (its loop runs under no_grad), so this is an extension:
default off, and with `guidance=None` the sampler executes exactly the un-guided code path (bit-identical, tested).

Energy: the clash + peptide-bond + bond-angle violation terms of csrc/guidance.hip (`abx_clash_grad`), evaluated on the network's predicted
structure x0_hat (`final_atom14_positions`, frames = predicted rigids).  Reconstruction guidance: the scores handed to
`FullDiffuser.reverse` become
    trans_score -= scale_trans * dE/dt_i / coordinate_scaling         (the R^3 process runs on 0.1 x coordinates, r3_diffuser.py:27-40)
    rot_score   -= scale_rot   * R_i^T (sum_a (x_a - t_i) x dE/dx_a)  (the SO(3) step right-multiplies: body-frame tangent vector)
for diffused residues only (fixed residues are restored by the mask merge of `reverse` anyway).

Interface guidance (`InterfaceGuidance`, csrc/contact.hip, `abx_contact_grad`) is the geometric half: it pulls the designed residues
toward the antigen instead of pushing atoms apart.  On the structure that a written design carries - the predicted atoms on the moved
rows, the ground truth elsewhere - it evaluates a smooth count of heavy-atom contacts with the partner rows, a soft-minimum distance
of the designed pseudo-betas to each chosen hotspot residue, and user-given pair-distance restraints (include/abx_hip.h,
AbxContactArgs; `contact_energy_host` is the float64 torch twin).  `Sum` composes it with the violation terms."""
import torch

from abx_amd import ops


def quat_to_rot(q):
    """(…,4) unit quaternion (w,x,y,z) -> (…,3,3)."""
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(q.shape[:-1] + (3, 3))


class ViolationGuidance:
    def __init__(self, scale_trans=1.0, scale_rot=1.0, w_clash=1.0, w_bond=1.0, w_angle=1.0, overlap_tolerance=1.5,
                 between_chain_factor=0.2, bond_tolerance_factor=12.0, coordinate_scaling=0.1, link_by_residx=True):
        """link_by_residx: array neighbours are peptide-bonded only when they share a chain id AND have consecutive residue numbers
        (a cropped antigen patch keeps one chain id across its gaps); False = the chain-only rule of cal_vio.py:51."""
        self.scale_trans, self.scale_rot = float(scale_trans), float(scale_rot)
        self.kw = dict(w_clash=w_clash, w_bond=w_bond, w_angle=w_angle, overlap_tolerance=overlap_tolerance,
                       between_chain_factor=between_chain_factor, bond_tolerance_factor=bond_tolerance_factor)
        self.coordinate_scaling = float(coordinate_scaling)
        self.link_by_residx = bool(link_by_residx)
        self.last_energy = None             # (B, 3) [clash, bond, angle] of the most recent call (device tensor)

    def energy_and_grads(self, batch, out):
        f = out['heads']['folding']
        seq0 = out['heads']['sequence_module']['seq_0']
        exists = ops.atom14_mask_table(seq0.device)[torch.clamp(seq0, 0, 20)] & batch['mask'][..., None].bool()
        return ops.clash_grad(f['final_atom14_positions'], exists, seq0, batch['chain_id'], f['rigids'][..., 4:],
                              residx=batch['residx'] if self.link_by_residx else None, **self.kw)

    def __call__(self, batch, out, rot_score, trans_score, diffuse_mask):
        energy, _, g_t, g_r = self.energy_and_grads(batch, out)
        self.last_energy = energy
        R = quat_to_rot(out['heads']['folding']['rigids'][..., :4])
        body = torch.einsum('...ji,...j->...i', R, g_r)                  # R^T tau
        m = diffuse_mask.to(g_t.dtype)[..., None]
        rot = rot_score - (self.scale_rot * body * m).to(rot_score.dtype)
        trans = trans_score - (self.scale_trans / self.coordinate_scaling * g_t * m).to(trans_score.dtype)
        return rot, trans


def _hub(v):
    """0 for v <= 0, v^2 / 2 for 0 < v < 1, v - 1/2 beyond: a hinge with a bounded, continuous slope."""
    return torch.where(v <= 0, torch.zeros_like(v), torch.where(v < 1, 0.5 * v * v, v - 0.5))


def pseudo_beta(atom14, exists):
    """CB (slot 4) where it exists, else CA (slot 1) -> positions (...,L,3), exists (...,L)."""
    cb = exists[..., 4].bool()
    return torch.where(cb[..., None], atom14[..., 4, :], atom14[..., 1, :]), cb | exists[..., 1].bool()


def contact_energy_host(atom14, exists, moved, target, hotspots=None, restraints=None, w_contact=0.0, d0=4.0, d1=8.0, w_hot=1.0,
                        d_hot=8.0, beta=1.0, details=False):
    """The float64 torch twin of abx_contact_grad's three energies (include/abx_hip.h, AbxContactArgs), term for term; differentiable
    by autograd with respect to atom14, no GPU needed.  atom14 (B,L,14,3) and exists (B,L,14): ONE structure per sample (the predicted
    atoms on the moved rows, the ground truth elsewhere); moved (B,L); target (L); hotspots: row indices; restraints: None or
    (idx (R,4) of row_i, slot_i, row_j, slot_j; par (R,3) of lo, hi, weight).  -> energy (B,3) [contact, hotspot, restraint]; with
    details also a dict: 'pair_d' the distances of the contact pairs, 'm_h' (B,H) soft minima (NaN: inactive), 'restr_d' (B,R) (NaN: an
    atom is missing)."""
    x = atom14.double()
    B, L = moved.shape
    ex, mv, tg = exists.bool(), moved.bool(), torch.as_tensor(target).bool()
    dist = lambda a, b: torch.sqrt(1e-10 + ((a - b) ** 2).sum(-1))
    e_c, e_h, e_r = [], [], []
    info = dict(pair_d=[], m_h=torch.full((B, 0 if hotspots is None else len(hotspots)), float('nan'), dtype=torch.float64),
                restr_d=torch.full((B, 0 if restraints is None else len(restraints[0])), float('nan'), dtype=torch.float64))
    for b in range(B):
        # contacts: existing atoms of moved rows x existing atoms of target rows that are not moved
        am = (ex[b] & mv[b][:, None]).reshape(-1)
        at = (ex[b] & (tg & ~mv[b])[:, None]).reshape(-1)
        xa, xt = x[b].reshape(-1, 3)[am], x[b].reshape(-1, 3)[at]
        d = dist(xa[:, None], xt[None])
        u = (d - d0) / (d1 - d0)
        s = torch.where(d <= d0, torch.ones_like(d), torch.where(d < d1, (1 - u * u) ** 2, torch.zeros_like(d)))
        e_c.append(-w_contact * s.sum() if w_contact != 0 else x.new_zeros(()))
        info['pair_d'].append(d.detach().reshape(-1))
        # hotspots: the soft minimum over the moved pseudo-betas, the maximum subtracted
        pb, pb_ok = pseudo_beta(x[b], ex[b])
        rows = torch.nonzero(mv[b] & pb_ok)[:, 0]
        eh = x.new_zeros(())
        for k, h in enumerate([] if hotspots is None else [int(v) for v in hotspots]):
            if len(rows) == 0 or bool(mv[b, h]) or not bool(pb_ok[h]):
                continue
            v = -beta * dist(pb[rows], pb[h][None])
            mx = v.max().detach()
            m = -(mx + torch.log(torch.exp(v - mx).sum())) / beta
            info['m_h'][b, k] = m.detach()
            eh = eh + w_hot * _hub(m - d_hot)
        e_h.append(eh)
        er = x.new_zeros(())
        if restraints is not None:
            for r, (q, (lo, hi, w)) in enumerate(zip(restraints[0].tolist(), restraints[1].tolist())):
                ri, si, rj, sj = (int(v) for v in q)
                if not (bool(ex[b, ri, si]) and bool(ex[b, rj, sj])):
                    continue
                dr = dist(x[b, ri, si], x[b, rj, sj])
                info['restr_d'][b, r] = dr.detach()
                er = er + w * (_hub(dr - hi) + _hub(lo - dr))
        e_r.append(er)
    energy = torch.stack([torch.stack(e_c), torch.stack(e_h), torch.stack(e_r)], dim=1)
    return (energy, info) if details else energy


def epitope_rows(atom14_gt, exists_gt, moved, target, d0=4.0, limit=64):
    """The target rows with a ground-truth heavy atom within d0 of a ground-truth heavy atom of a moved row: what the wild-type loop
    touched.  More than `limit`: the nearest.  Un-batched host tensors (L,14,3), (L,14), (L), (L) -> sorted list of rows."""
    x, ex = atom14_gt.double().cpu(), exists_gt.bool().cpu()
    mv, tg = moved.bool().cpu(), torch.as_tensor(target).bool().cpu() & ~moved.bool().cpu()
    a, b = x[mv][ex[mv]], x[tg]                                     # (Na,3), (T,14,3)
    if a.shape[0] == 0 or b.shape[0] == 0:
        return []
    d = torch.cdist(b.reshape(-1, 3), a).min(1)[0].reshape(-1, 14)
    d = torch.where(ex[tg], d, torch.full_like(d, float('inf'))).min(1)[0]
    rows = torch.nonzero(tg)[:, 0]
    keep = torch.nonzero(d <= d0)[:, 0]
    keep = keep[torch.argsort(d[keep], stable=True)][:limit]
    return sorted(rows[keep].tolist())


class InterfaceGuidance:
    """Contact, hotspot and pair-restraint guidance of one featurised batch (abx_contact_grad).  Built once per batch: every table goes
    to the device here, and a call launches kernels and elementwise device operations only (no host synchronisation, no host-to-device
    copy: it can be recorded by graph.GraphedSteps).  hotspots: None, 'epitope' (epitope_rows of sample 0) or row indices;
    restraints: None or (idx (R,4), par (R,3)) as parse_restraints returns; target: (L) mask of the partner rows, default the rows
    >= Lab (the featurised antigen).  The default weights are not tuned on a trained checkpoint."""

    def __init__(self, batch, w_contact=0.0, d0=4.0, d1=8.0, hotspots=None, w_hot=1.0, d_hot=8.0, beta=1.0, restraints=None, scale_trans=1.0,
                 scale_rot=1.0, target=None, coordinate_scaling=0.1):
        self.scale_trans, self.scale_rot, self.coordinate_scaling = float(scale_trans), float(scale_rot), float(coordinate_scaling)
        dev = batch['seq'].device
        L, Lab = batch['seq'].shape[1], batch['anchor_flag'].shape[1]
        if target is None:
            target = torch.arange(L) >= Lab
        target = torch.as_tensor(target).bool().cpu()
        assert tuple(target.shape) == (L,), target.shape
        if isinstance(hotspots, str):
            if hotspots != 'epitope':
                raise ValueError(f"hotspots: None, 'epitope' or row indices, not {hotspots!r}")
            moved0 = ((1 - batch['fixed_mask'][0]) * batch['atom14_gt_exists'][0, :, 0]).bool()
            hotspots = epitope_rows(batch['atom14_gt_positions'][0], batch['atom14_gt_exists'][0], moved0, target, d0=d0)
        self.hotspots = [] if hotspots is None else [int(h) for h in hotspots]
        self.tables = ops.ContactTables(dev, self.hotspots, restraints)
        self.target = target.to(dev).to(torch.uint8)
        self.kw = dict(w_contact=w_contact, d0=d0, d1=d1, w_hot=w_hot, d_hot=d_hot, beta=beta)
        self.last_energy = None             # (B, 3) [contact, hotspot, restraint] of the most recent call (device tensor)

    def structure(self, batch, out, diffuse_mask):
        """The structure a written design carries -> (atom14 (B,L,14,3), exists (B,L,14), moved (B,L) bool): the predicted atoms, typed
        by the predicted tokens, on the moved rows and the ground truth elsewhere."""
        f = out['heads']['folding']
        seq0 = out['heads']['sequence_module']['seq_0']
        moved = diffuse_mask.bool()
        pred_ok = ops.atom14_mask_table(seq0.device)[torch.clamp(seq0, 0, 20)]
        exists = torch.where(moved[..., None], pred_ok, batch['atom14_gt_exists'].bool()) & batch['mask'][..., None].bool()
        x = torch.where(moved[..., None, None], f['final_atom14_positions'], batch['atom14_gt_positions'].to(f['final_atom14_positions'].dtype))
        return x, exists, moved

    def energy_and_grads(self, batch, out, diffuse_mask):
        x, exists, moved = self.structure(batch, out, diffuse_mask)
        return ops.contact_grad(x, exists, moved, self.target, out['heads']['folding']['rigids'][..., 4:], self.tables, **self.kw)

    def __call__(self, batch, out, rot_score, trans_score, diffuse_mask):
        energy, _, g_t, g_r = self.energy_and_grads(batch, out, diffuse_mask)
        self.last_energy = energy
        R = quat_to_rot(out['heads']['folding']['rigids'][..., :4])
        body = torch.einsum('...ji,...j->...i', R, g_r)                  # R^T tau
        m = diffuse_mask.to(g_t.dtype)[..., None]
        rot = rot_score - (self.scale_rot * body * m).to(rot_score.dtype)
        trans = trans_score - (self.scale_trans / self.coordinate_scaling * g_t * m).to(trans_score.dtype)
        return rot, trans


class Sum:
    """Guidance terms applied one after the other: each receives the scores the previous one returned."""

    def __init__(self, *terms):
        self.terms = [t for t in terms if t is not None]

    def __call__(self, batch, out, rot_score, trans_score, diffuse_mask):
        for t in self.terms:
            rot_score, trans_score = t(batch, out, rot_score, trans_score, diffuse_mask)
        return rot_score, trans_score


def _rows_of(batch_one):
    """(chain_id, residx, seq) of a one-complex batch as host lists, with or without the leading batch dimension."""
    get = lambda k: (batch_one[k][0] if batch_one[k].dim() == 2 else batch_one[k]).cpu().tolist()
    return get('chain_id'), get('residx'), get('seq')


def _find_row(token, batch_one, chains):
    """'<chain letter>:<residx as featurised>' -> row of the featurised complex.  chains: the chain letters in the order of the chain
    ids (heavy 0, light 1, the k-th antigen chain 2 + k)."""
    try:
        letter, num = token.split(':')
        num = int(num)
    except ValueError:
        raise SystemExit(f'residue {token!r}: expected <chain letter>:<residue index as featurised>')
    if letter not in chains:
        raise SystemExit(f'residue {token!r}: no chain {letter!r} in this complex (chains: {" ".join(chains)})')
    cid = list(chains).index(letter)
    chain_id, residx, _ = _rows_of(batch_one)
    for r, (c, n) in enumerate(zip(chain_id, residx)):
        if c == cid and n == num:
            return r
    raise SystemExit(f'residue {token!r} is not in the featurised complex (an antigen residue outside the 16 A patch or the '
                     f'32-residue window, or a residue outside the variable domain)')


def parse_residues(spec, batch_one, chains):
    """Residue tokens (a list, or one string separated by blanks or commas) -> rows of the featurised complex; SystemExit names a
    residue that is not there."""
    tokens = spec.replace(',', ' ').split() if isinstance(spec, str) else list(spec)
    return [_find_row(t, batch_one, chains) for t in tokens]


def parse_restraints(path, batch_one, chains):
    """A restraint file, one `res atom res atom lo hi [weight]` per line (# comments, blank lines) -> (idx (R,4) int32 of row_i, slot_i,
    row_j, slot_j; par (R,3) float32 of lo, hi, weight).  Atom names resolve to atom14 slots by the ground-truth residue type."""
    from abx_amd import residue_constants as rc
    _, _, seq = _rows_of(batch_one)
    idx, par = [], []

    def slot(token, row, name):
        aa = seq[row]
        res3 = rc.restype_1to3[rc.restypes[aa]] if 0 <= aa < 20 else 'UNK'
        names = rc.restype_name_to_atom14_names[res3]
        if name not in names or not name:
            raise SystemExit(f'atom {name!r} of residue {token!r}: a {res3} has no such atom')
        return list(names).index(name)

    with open(path) as f:
        for ln, line in enumerate(f, 1):
            w = line.split('#')[0].split()
            if not w:
                continue
            if len(w) not in (6, 7):
                raise SystemExit(f'{path}:{ln}: expected `res atom res atom lo hi [weight]`')
            ri, rj = _find_row(w[0], batch_one, chains), _find_row(w[2], batch_one, chains)
            lo, hi, wt = float(w[4]), float(w[5]), float(w[6]) if len(w) == 7 else 1.0
            if lo > hi:
                raise SystemExit(f'{path}:{ln}: lo {lo} > hi {hi}')
            idx.append([ri, slot(w[0], ri, w[1]), rj, slot(w[2], rj, w[3])])
            par.append([lo, hi, wt])
    if len(idx) > 256:
        raise SystemExit(f'{path}: {len(idx)} restraints, at most 256')
    return torch.tensor(idx, dtype=torch.int32).reshape(-1, 4), torch.tensor(par, dtype=torch.float32).reshape(-1, 3)
