"""Violation relaxation of designed residues: the step between design and evaluation.  Upstream runs PyRosetta FastRelax on the designed
CDRs (relax_pdb.py, abx/relax.py) and writes <name>_relaxed.pdb; here the violation energy of the guidance terms (csrc/guidance.hip:
steric overlap, C-N bond, CA-C-N / C-N-CA angles), restricted to the terms that touch a movable residue, is minimised by steepest
descent with an adaptive step in the space of rigid-body motions of every movable residue plus its side-chain chi angles.  Bond
lengths and angles inside a residue stay what the torsion head produced; fixed residues and the antigen never move.

    E = E_viol|M + k_restraint * sum_{r in M} |CA_r - CA_r(input)|^2

`ViolationRelaxer` runs it on the device for a batch of designs of one complex (abx_relax, csrc/relax.hip: one launch, one workgroup
per design).  `relax_host` is the plain-torch float64 twin of the same algorithm (autograd gradients) for tests and for machines
without a GPU.  k_restraint has no principled default (the energy is in Angstrom of overlap, not kcal/mol): it is 0; a positive value
bounds the motion by k * sum |dCA|^2 <= E_viol(input), because E never increases."""
import torch

from . import complex_view
from . import residue_constants as rc

# The report row of abx_relax (include/abx_hip.h, ABX_RELAX_COLS)
RELAX_COLUMNS = ('E_clash_in', 'E_bond_in', 'E_angle_in', 'E_clash', 'E_bond', 'E_angle', 'E_restraint', 'evaluations', 'accepted',
                 'eta', 'max_ca_shift')
_INT_COLUMNS = ('evaluations', 'accepted')
DEFAULTS = dict(overlap_tolerance=1.5, between_chain_factor=0.2, bond_tolerance_factor=12.0, w_clash=1.0, w_bond=1.0, w_angle=1.0,
                k_restraint=0.0, eta0=0.01, rho=2.0, grow=1.2, shrink=0.5, max_iter=200)


def format_report(row):
    """One report row as TSV fields: integers for the counters, %.6g for the rest."""
    return [str(int(v)) if c in _INT_COLUMNS else f'{float(v):.6g}' for c, v in zip(RELAX_COLUMNS, row)]


def expand_movable(movable, chain_id, residx=None, flank=0, limit=None):
    """movable (L) bool plus `flank` peptide-linked neighbours on each side of every movable stretch (linked: same chain id and, with
    residx, consecutive residue numbers); rows >= limit are never added."""
    mov = movable.bool().clone()
    L = mov.shape[0]
    link = chain_id[1:] == chain_id[:-1]
    if residx is not None:
        link = link & (residx[1:] == residx[:-1] + 1)
    for _ in range(int(flank)):
        grown = mov.clone()
        grown[1:] |= mov[:-1] & link
        grown[:-1] |= mov[1:] & link
        mov = grown
    if limit is not None:
        mov[limit:] = False
    assert mov.shape[0] == L
    return mov


class ViolationRelaxer(complex_view.ComplexView):
    """Relaxes batches of designs of ONE complex on the device.  Built once per complex from its featurised batch like
    metrics.DesignScorer.  movable: (L) mask of the rows that may move (default: the rows the sampler diffuses, sample 0's
    (1 - fixed_mask) * backbone mask); flank: that many peptide-linked neighbours on each side are added.  Only antibody rows
    (< Lab) can move.  params: DEFAULTS."""

    def __init__(self, batch, movable=None, flank=0, link_by_residx=True, **params):
        super().__init__(batch, chains=True, link_by_residx=link_by_residx)
        movable = complex_view.region_mask(batch, movable, self.chain_id.device)
        movable = expand_movable(movable, self.chain_id, self.residx, flank, limit=self.Lab)
        self.movable = movable.to(torch.uint8).contiguous()
        self.M = int(self.movable.sum())                     # (the one host synchronisation: at construction)
        if self.M == 0:
            raise ValueError('ViolationRelaxer: no movable residue among the antibody rows')
        unknown = set(params) - set(DEFAULTS)
        if unknown:
            raise TypeError(f'ViolationRelaxer: unknown parameters {sorted(unknown)}')
        self.params = dict(DEFAULTS, **params)

    def relax(self, atom14, seq):
        """atom14 (B, Lab or L, 14, 3) f32 predicted coordinates, seq (B, Lab) tokens -> (atom14_relaxed, same shape, f32;
        report (B, len(RELAX_COLUMNS)) float64), both on the device.  One launch, no host synchronisation."""
        from . import ops
        return ops.relax(atom14, seq, self.gt_atom14, self.gt_seq, self.gt_exists, self.chain_id, self.movable, Lab=self.Lab,
                         residx=self.residx, res_mask=self.res_mask, n_movable=self.M, **self.params)


# -------------------------------------------------------------------------------------------------------------------
# host twin (float64, plain torch)
# -------------------------------------------------------------------------------------------------------------------
_VDW = {'C': 1.7, 'N': 1.55, 'O': 1.52, 'S': 1.8}


def _tables():
    rad = torch.zeros(21, 14, dtype=torch.float64)
    for i, r in enumerate(rc.restypes):
        for j, name in enumerate(rc.restype_name_to_atom14_names[rc.restype_1to3[r]]):
            if name:
                rad[i, j] = _VDW[name[0]]
    idx37 = torch.as_tensor(rc.chi_angles_atom_indices).long()[:, :, 1:3]
    a14 = torch.as_tensor(rc.restype_atom37_to_atom14).long()
    axis = torch.gather(a14[:, None, :].expand(-1, 4, -1), 2, idx37)                        # (21, 4, 2) atom14 slots
    has = torch.as_tensor(rc.chi_angles_mask) > 0                                           # (21, 4)
    group = torch.as_tensor(rc.restype_atom14_to_rigid_group).long()                        # (21, 14)
    return rad, axis, has, group


def rodrigues(axis, ang):
    """Rotation matrices (..., 3, 3) about unit vectors axis (..., 3) by ang (...)."""
    x, y, z = axis.unbind(-1)
    c, s = torch.cos(ang), torch.sin(ang)
    C = 1 - c
    return torch.stack([c + x * x * C, x * y * C - z * s, x * z * C + y * s,
                        y * x * C + z * s, c + y * y * C, y * z * C - x * s,
                        z * x * C - y * s, z * y * C + x * s, c + z * z * C], -1).reshape(ang.shape + (3, 3))


def rotvec_to_matrix(w):
    th = torch.sqrt((w * w).sum(-1) + 1e-30)
    return rodrigues(w / th[..., None], th)


def rebuild(x_in, mask, aa, R, t, chi):
    """Positions of M residues from their input coordinates and a state.  x_in (M,14,3), mask (M,14) bool, aa (M,), R (M,3,3),
    t (M,3), chi (M,4) -> (M,14,3): local = x_in - CA_in; chi_k (where the residue type has it and both axis atoms exist) rotates the
    slots of rigid group >= 3 + k about the axis through its two axis atoms, k = 1..4 in order; x = R local + CA_in + t."""
    _, AXIS, HAS, GROUP = _tables()
    aa = aa.clamp(0, 20)
    ca = x_in[:, 1]
    x = x_in - ca[:, None]
    ar = torch.arange(aa.shape[0])
    for k in range(4):
        a1, a2 = AXIS[aa, k, 0], AXIS[aa, k, 1]
        active = HAS[aa, k] & mask[ar, a1] & mask[ar, a2]
        p1, p2 = x[ar, a1], x[ar, a2]
        ax = p2 - p1
        ax = ax / torch.sqrt((ax * ax).sum(-1, keepdim=True) + 1e-30)
        Rk = rodrigues(ax, chi[:, k] * active.to(chi.dtype))
        moved = torch.einsum('mij,maj->mai', Rk, x - p2[:, None]) + p2[:, None]
        x = torch.where(((GROUP[aa] >= 4 + k) & active[:, None])[..., None], moved, x)
    return torch.einsum('mij,maj->mai', R, x) + (ca + t)[:, None]


def _peptide_losses(x, mask, aa, chain, residx, tol):
    """Per pair (l, l + 1): masked bond and angle losses of eval/metric_scripts/cal_vio.py:29-110 (the expressions of peptide_dev.h)."""
    m = mask.to(x.dtype)
    ca, c, n, ca2 = x[:-1, 1], x[:-1, 2], x[1:, 0], x[1:, 1]
    m_ca, m_c, m_n, m_ca2 = m[:-1, 1], m[:-1, 2], m[1:, 0], m[1:, 1]
    link = chain[1:] == chain[:-1]
    if residx is not None:
        link = link & (residx[1:] == residx[:-1] + 1)
    link = link.to(x.dtype)
    pro = (aa[1:] == 14).to(x.dtype)
    l0 = (1 - pro) * 1.329 + pro * 1.341
    sd = (1 - pro) * 0.014 + pro * 0.016
    dist = torch.sqrt(1e-6 + ((c - n) ** 2).sum(-1))
    err_b = torch.sqrt(1e-6 + (dist - l0) ** 2)
    unit = lambda v: v / torch.sqrt(torch.clamp((v ** 2).sum(-1, keepdim=True), min=1e-12))
    c_ca, c_n, n_ca = unit(ca - c), unit(n - c), unit(ca2 - n)
    err_a1 = torch.sqrt(1e-6 + ((c_ca * c_n).sum(-1) - (-0.4473)) ** 2)
    err_a2 = torch.sqrt(1e-6 + (((-c_n) * n_ca).sum(-1) - (-0.5203)) ** 2)
    bond = torch.relu(err_b - tol * sd) * m_c * m_n * link
    angle = torch.relu(err_a1 - tol * 0.0311) * m_ca * m_c * m_n * link + torch.relu(err_a2 - tol * 0.0353) * m_c * m_n * m_ca2 * link
    return bond, angle


def restricted_energy(x, mask, aa, chain, residx, movable, ca_in=None, overlap_tolerance=1.5, between_chain_factor=0.2,
                      bond_tolerance_factor=12.0, w_clash=1.0, w_bond=1.0, w_angle=1.0, k_restraint=0.0):
    """The violation energy restricted to the terms that touch a movable residue, plus the restraint.  x (L,14,3) float64, mask (L,14)
    bool, aa (L), chain (L), residx (L) or None, movable (L) bool, ca_in (L,3) the input C-alpha (None: no restraint term).
    -> (E_clash, E_bond, E_angle, E_restraint) 0-dim tensors.  Atom pairs with at least one atom in a movable residue (pairs inside the
    movable set once), without pairs of one residue, the C(i)-N(i+1) of linked neighbours and SG-SG; the peptide terms of (l, l+1)
    when l or l+1 is movable."""
    RAD = _tables()[0]
    L = aa.shape[0]
    aa = aa.clamp(0, 20).long()
    mov = movable.bool()
    rad = RAD[aa].to(x.dtype)
    ok = mask.bool() & (rad > 0)
    mi = torch.nonzero(mov)[:, 0]
    nm = mi.shape[0]
    xm, rm, okm = x[mi].reshape(-1, 3), rad[mi].reshape(-1), ok[mi].reshape(-1)
    resm, slotm, chm = mi.repeat_interleave(14), torch.arange(14).repeat(nm), chain[mi].repeat_interleave(14)
    xa, ra, oka = x.reshape(-1, 3), rad.reshape(-1), ok.reshape(-1)
    resa, slota, cha = torch.arange(L).repeat_interleave(14), torch.arange(14).repeat(L), chain.repeat_interleave(14)
    mova = mov.repeat_interleave(14)
    d = torch.sqrt(1e-10 + ((xm[:, None] - xa[None]) ** 2).sum(-1))
    pair = okm[:, None] & oka[None] & (resm[:, None] != resa[None]) & (~mova[None] | (resm[:, None] < resa[None]))
    link = chain[1:] == chain[:-1]
    if residx is not None:
        link = link & (residx[1:] == residx[:-1] + 1)
    linked = torch.zeros(L, dtype=torch.bool)
    linked[1:] = link                                                                        # linked to the array predecessor
    b1 = (resa[None] == resm[:, None] + 1) & linked[resa][None] & (slotm[:, None] == 2) & (slota[None] == 0)
    b2 = (resm[:, None] == resa[None] + 1) & linked[resm][:, None] & (slota[None] == 2) & (slotm[:, None] == 0)
    sgm, sga = (aa[resm] == 4) & (slotm == 5), (aa[resa] == 4) & (slota == 5)
    pair = pair & ~b1 & ~b2 & ~(sgm[:, None] & sga[None])
    w = torch.where(chm[:, None] == cha[None], 1.0, float(between_chain_factor)).to(x.dtype)
    e_clash = w_clash * (w * torch.relu(rm[:, None] + ra[None] - overlap_tolerance - d) * pair).sum()
    bond, angle = _peptide_losses(x, mask, aa, chain, residx, bond_tolerance_factor)
    touch = (mov[:-1] | mov[1:]).to(x.dtype)
    e_bond = w_bond * (bond * touch).sum()
    e_angle = w_angle * (angle * touch).sum()
    e_res = x.new_zeros(())
    if ca_in is not None and k_restraint:
        e_res = k_restraint * ((x[mi, 1] - ca_in[mi]) ** 2).sum()
    return e_clash, e_bond, e_angle, e_res


def relax_host(x_in, mask, aa, chain, residx, movable, max_iter=200, eta0=0.01, rho=2.0, grow=1.2, shrink=0.5, k_restraint=0.0,
               return_grad=False, **energy_kw):
    """The algorithm of abx_relax in float64 with autograd gradients.  x_in (L,14,3), mask (L,14) bool, aa (L), chain (L), residx (L)
    or None, movable (L) bool.  -> (x (L,14,3) float64, report: (len(RELAX_COLUMNS),) float64[, generalised gradient (M,10) of the
    returned state: dE/dt, dE/d(infinitesimal rotation about the C-alpha, world frame), dE/dchi]).  State per movable residue:
    translation, rotation matrix, chi increments; trial t -= eta g_t, R <- exp(-eta tau / rho^2) R, chi -= eta g_chi / rho^2; taken when
    E_trial < E (eta *= grow) else dropped (eta *= shrink); ends after max_iter evaluations or at E == 0.  max_iter = 0: one evaluation.
    A structure without an accepted step is returned as a copy of its input."""
    x_in = x_in.to(torch.float64)
    mask = mask.bool()
    mov = movable.bool()
    mi = torch.nonzero(mov)[:, 0]
    M = mi.shape[0]
    assert M > 0, 'no movable residue'
    xm, mm, am = x_in[mi], mask[mi], aa[mi]
    ca_in = x_in[:, 1]

    def evaluate(R, t, chi, at_input=False):
        dw = torch.zeros(M, 3, dtype=torch.float64, requires_grad=True)        # dE/d(dw) at 0 is the torque about the C-alpha
        t_ = t.clone().requires_grad_(True)
        chi_ = chi.clone().requires_grad_(True)
        xb = rebuild(xm, mm, am, rotvec_to_matrix(dw) @ R, t_, chi_)
        if at_input:                                                            # the input itself, not its rebuild: same derivatives
            xb = xm + (xb - xb.detach())
        x = x_in.index_put((mi,), xb)
        parts = restricted_energy(x, mask, aa, chain, residx, mov, ca_in, k_restraint=k_restraint, **energy_kw)
        E = ((parts[0] + parts[1]) + parts[2]) + parts[3]
        g = torch.autograd.grad(E, [t_, dw, chi_], allow_unused=True)
        g = [torch.zeros_like(p) if gi is None else gi for p, gi in zip([t_, dw, chi_], g)]
        return float(E.detach()), [float(p.detach()) for p in parts], torch.cat(g, dim=1), x.detach()

    st = (torch.eye(3, dtype=torch.float64).expand(M, 3, 3).clone(), torch.zeros(M, 3, dtype=torch.float64), torch.zeros(M, 4, dtype=torch.float64))
    E, parts, G, x = evaluate(*st, at_input=True)
    parts0, eta, n, acc = parts, float(eta0), 1, 0
    while n < max_iter and E != 0.0:
        trial = (rotvec_to_matrix(-eta * G[:, 3:6] / rho ** 2) @ st[0], st[1] - eta * G[:, 0:3], st[2] - eta * G[:, 6:10] / rho ** 2)
        E2, parts2, G2, x2 = evaluate(*trial)
        n += 1
        if E2 < E:
            st, E, parts, G, x = trial, E2, parts2, G2, x2
            eta *= grow
            acc += 1
        else:
            eta *= shrink
    if acc == 0:
        x = x_in.clone()
    shift = float((x[mi, 1] - x_in[mi, 1]).norm(dim=-1).max())
    report = torch.tensor(parts0[:3] + parts + [n, acc, eta, shift], dtype=torch.float64)
    return (x, report, G) if return_grad else (x, report)
