"""Inputs shared by tests/test_torsions_host.py and tests/test_gpu_torsions.py: chains built from ideal bond lengths and angles and given
(phi, psi, omega) per residue whose classes are written down, the twin on a complex of relax_cases, the structures the GPU test scores,
and helpers that mutate a residue or turn one chi angle.  Importing it touches no GPU."""
import numpy as np
import torch

import relax_cases as RC

A_, R_, N_, D_, C_, Q_, E_, G_, H_, I_, L_, K_, M_, F_, P_, S_, T_, W_, Y_, V_ = range(20)
# Engh & Huber (1991) backbone geometry, the values of the literature tables the reference also quotes
BOND = dict(n_ca=1.458, ca_c=1.525, c_n=1.329, c_o=1.231, ca_cb=1.530)
ANGLE = dict(n_ca_c=111.0, ca_c_n=116.2, c_n_ca=121.7, ca_c_o=120.8, n_ca_cb=110.5)
N_RES = 8
HELIX = (-57.0, -47.0)
# (phi, psi, expected ABEGO letter) of the four uniform chains; omega = 180
UNIFORM = ((-57.0, -47.0, 'A'), (-120.0, 130.0, 'B'), (57.0, 47.0, 'G'), (60.0, -150.0, 'E'))
CIS_LINK, TWISTED_LINK = 3, 5                          # chain 4: omega of the link (2, 3) is 0, of the link (4, 5) 120 degrees
SEEDS = RC.SEEDS                                        # the seeded perturbations the GPU test scores: no borderline decision (asserted on the host)


def place(a, b, c, length, angle, torsion):
    """NeRF: the point d with |d - c| = length, angle(b, c, d) = angle and dihedral(a, b, c, d) = torsion (degrees), float64."""
    th, ta = np.deg2rad(angle), np.deg2rad(torsion)
    bc = (c - b) / np.linalg.norm(c - b)
    n = np.cross(b - a, bc)
    n = n / np.linalg.norm(n)
    m = np.cross(n, bc)
    return c + length * (-np.cos(th) * bc + np.sin(th) * np.cos(ta) * m + np.sin(th) * np.sin(ta) * n)


def build_chain(phi, psi, omega):
    """Poly-Ala of len(phi) residues with N, CA, C, O, CB (atom14 slots 0..4) from BOND / ANGLE and the given dihedrals in degrees:
    phi[i] and omega[i] (of the link (i-1, i)) for i >= 1, psi[i] for i < n - 1.  -> (x (n,14,3) float32 as float64, mask (n,14) bool)."""
    n = len(phi)
    x = np.zeros((n, 14, 3))
    x[0, 0] = (0.0, 0.0, 0.0)
    x[0, 1] = (BOND['n_ca'], 0.0, 0.0)
    th = np.deg2rad(ANGLE['n_ca_c'])
    x[0, 2] = x[0, 1] + BOND['ca_c'] * np.array([-np.cos(th), np.sin(th), 0.0])
    for i in range(1, n):
        x[i, 0] = place(x[i - 1, 0], x[i - 1, 1], x[i - 1, 2], BOND['c_n'], ANGLE['ca_c_n'], psi[i - 1])
        x[i, 1] = place(x[i - 1, 1], x[i - 1, 2], x[i, 0], BOND['n_ca'], ANGLE['c_n_ca'], omega[i])
        x[i, 2] = place(x[i - 1, 2], x[i, 0], x[i, 1], BOND['ca_c'], ANGLE['n_ca_c'], phi[i])
    for i in range(n):
        x[i, 3] = place(x[i, 0], x[i, 1], x[i, 2], BOND['c_o'], ANGLE['ca_c_o'], (psi[i] if i < n - 1 else 0.0) + 180.0)
        x[i, 4] = place(x[i, 2], x[i, 0], x[i, 1], BOND['ca_cb'], ANGLE['n_ca_cb'], -122.6)
    mask = np.zeros((n, 14), bool)
    mask[:, :5] = True
    return x.astype(np.float32).astype(np.float64), mask


def built_chains():
    """The five chains of N_RES residues -> list of dict(x, mask, phi, psi, omega (built values, degrees), letters: the expected class of
    every residue ('-' at the two ends), cis, twisted: the expected counts)."""
    out = []
    for phi, psi, letter in UNIFORM:
        om = np.full(N_RES, 180.0)
        x, mask = build_chain(np.full(N_RES, phi), np.full(N_RES, psi), om)
        out.append(dict(x=x, mask=mask, phi=np.full(N_RES, phi), psi=np.full(N_RES, psi), omega=om,
                        letters='-' + letter * (N_RES - 2) + '-', cis=0, twisted=0))
    om = np.full(N_RES, 180.0)
    om[CIS_LINK], om[TWISTED_LINK] = 0.0, 120.0
    x, mask = build_chain(np.full(N_RES, HELIX[0]), np.full(N_RES, HELIX[1]), om)
    letters = ['-'] + ['A'] * (N_RES - 2) + ['-']
    letters[CIS_LINK] = 'O'
    out.append(dict(x=x, mask=mask, phi=np.full(N_RES, HELIX[0]), psi=np.full(N_RES, HELIX[1]), omega=om, letters=''.join(letters), cis=1, twisted=1))
    return out


def chain_complex(ch):
    """A built chain as a complex of relax_cases.load_complex (one chain, no antigen, every residue in the region)."""
    n = ch['x'].shape[0]
    return dict(x=torch.from_numpy(ch['x']), mask=torch.from_numpy(ch['mask']), aa=torch.zeros(n, dtype=torch.long), chain=torch.zeros(n, dtype=torch.long),
                residx=torch.arange(n), cdr=torch.zeros(n, dtype=torch.long), mov=torch.ones(n, dtype=torch.bool), Lab=n)


def twin(c, x, mask=None, seq=None, wild_x=None, **kw):
    """torsions_host of structure x of complex c against its crystal structure, region = its movable set."""
    from abx_amd import torsions
    return torsions.torsions_host(x, c['mask'] if mask is None else mask, c['aa'] if seq is None else seq, c['x'] if wild_x is None else wild_x,
                                  c['mask'], c['aa'], c['Lab'], c['chain'], c['residx'], region=c['mov'], **kw)


def mutate(c, seq, rows, token):
    """(tokens, atom mask) of the complex with `rows` retyped to `token`: a mutated row has the atoms of its new type that the crystal
    residue also has (its coordinates are the crystal's)."""
    from abx_amd import residue_constants as rc
    seq = seq.clone()
    seq[rows] = token
    mask = c['mask'].clone()
    mask[rows] = mask[rows] & torch.as_tensor(rc.restype_atom14_mask)[seq[rows]].bool()
    return seq, mask


def mutated(c, seed):
    """The tokens and mask of the `mutated version` of a seeded perturbation: every second movable residue retyped, Ala / Gly / Pro in turn."""
    rows = torch.nonzero(c['mov'])[:, 0][::2]
    seq, mask = c['aa'].clone(), c['mask'].clone()
    for k, r in enumerate(rows.tolist()):
        seq, m = mutate(c, seq, [r], (A_, G_, P_)[(k + seed) % 3])
        mask[r] = m[r]
    return seq, mask


def turn_chi(c, x, row, k, degrees):
    """x with chi_k (k = 1..4) of residue `row` turned by `degrees`: the atoms beyond the chi axis rotate about it (relax.rebuild, the
    idea of relax_cases.perturb without the rigid-body move); rounded to float32."""
    from abx_amd import relax
    chi = torch.zeros(1, 4, dtype=torch.float64)
    chi[0, k - 1] = float(np.deg2rad(degrees))
    x = x.clone()
    sl = slice(row, row + 1)
    x[sl] = relax.rebuild(x[sl], c['mask'][sl], c['aa'][sl], torch.eye(3, dtype=torch.float64)[None], torch.zeros(1, 3, dtype=torch.float64), chi)
    return x.float().double()


def region_rows(c, token, with_chi2=True):
    """The movable rows of the complex with the token (and with chi2 atoms present)."""
    from abx_amd import torsions
    atoms, _ = torsions.chi_table()
    rows = []
    for r in torch.nonzero(c['mov'] & (c['aa'] == token))[:, 0].tolist():
        sl = atoms[token, 1 if with_chi2 else 0]
        if (sl >= 0).all() and bool(c['mask'][r, torch.as_tensor(sl.astype(np.int64))].all()):
            rows.append(r)
    return rows


def gpu_structures(c):
    """What the GPU test scores of a shipped complex in one batch, as (x (L,14,3) float64, tokens, (L,14) mask) triples: the wild type,
    the three seeded perturbations and their mutated versions (7 structures)."""
    out = [(c['x'].float().double(), c['aa'], c['mask'])]
    for s in SEEDS:
        xp = RC.perturb(c, s)
        out.append((xp, c['aa'], c['mask']))
        seq, mask = mutated(c, s)
        out.append((xp, seq, mask))
    return out


def tiny_structures():
    """The tiny synthetic workload (Lab = 16) and two noisy copies of its antibody -> (cx, xh (2,Lab,14,3) float32, region (L) bool)."""
    from abx_amd import synthetic
    cx = synthetic.make_complex(seed=3, **synthetic.WORKLOADS['tiny'])
    Lab = cx['anchor_flag'].shape[0]
    g = torch.Generator().manual_seed(5)
    xh = (cx['atom14_gt_positions'][None, :Lab] + 0.3 * torch.randn(2, Lab, 14, 3, generator=g)).float()
    return cx, xh, cx['cdr_def'] == 5


def synthetic_twin(cx, x, region):
    """torsions_host of a design x (Lab,14,3) of a synthetic complex whose rows have the atoms of their tokens."""
    from abx_amd import residue_constants as rc, torsions
    Lab = cx['anchor_flag'].shape[0]
    typed = torch.as_tensor(rc.restype_atom14_mask)[cx['seq'][:Lab]].bool()
    return torsions.torsions_host(x, typed, cx['seq'], cx['atom14_gt_positions'], cx['atom14_gt_exists'], cx['seq'], Lab, cx['chain_id'],
                                  cx['residx'], region=region, res_mask=cx['mask'])
