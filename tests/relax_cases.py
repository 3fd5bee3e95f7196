"""Inputs shared by tests/test_relax_host.py and tests/test_gpu_relax.py: the two shipped complexes (tests/golden/pdb_6qd7.npz,
pdb_6ct7.npz), their movable sets, and the seeded rigid-body + chi perturbation of the movable residues."""
import torch

from conftest import load_npz, tt

CDR_CODES = (1, 3, 5, 8, 10, 12)
# (fixture, movable set): CDR-H3 of both complexes (14 and 4 residues), all six CDRs of 6qd7 (48 residues)
MOVABLE_SETS = (('6qd7', 'h3'), ('6ct7', 'h3'), ('6qd7', 'all'))
SEEDS = (5, 6, 7)


def load_complex(code, sel):
    """-> dict of un-batched tensors: x (L,14,3) float64 crystal coordinates, mask (L,14) bool, aa, chain, residx, cdr (L) int64,
    mov (L) bool, Lab."""
    z = load_npz(f'pdb_{code}.npz')
    one = lambda k: tt(z['batch.' + k][0])
    cdr = one('cdr_def').long()
    mov = (cdr == 5) if sel == 'h3' else torch.isin(cdr, torch.tensor(CDR_CODES))
    return dict(x=one('atom14_gt_positions').double(), mask=one('atom14_gt_exists').bool(), aa=one('seq').long(), chain=one('chain_id').long(),
                residx=one('residx').long(), cdr=cdr, mov=mov, Lab=int(z['batch.anchor_flag'].shape[1]))


def perturb(c, seed, sig_t=0.7, sig_r=0.25, sig_chi=0.5):
    """The movable residues of complex c moved as rigid bodies (N(0, sig_r rad) rotation vector about the C-alpha, N(0, sig_t A)
    translation) with N(0, sig_chi rad) chi increments, seeded; rounded to float32 (what a kernel sees), returned as float64."""
    from abx_amd import relax
    mi = torch.nonzero(c['mov'])[:, 0]
    g = torch.Generator().manual_seed(seed)
    w = sig_r * torch.randn(len(mi), 3, generator=g, dtype=torch.float64)
    t = sig_t * torch.randn(len(mi), 3, generator=g, dtype=torch.float64)
    chi = sig_chi * torch.randn(len(mi), 4, generator=g, dtype=torch.float64)
    x = c['x'].clone()
    x[mi] = relax.rebuild(c['x'][mi], c['mask'][mi], c['aa'][mi], relax.rotvec_to_matrix(w), t, chi)
    return x.float().double()


def counts(x, c):
    """The five count columns (n_viol_c_n, n_viol_ca_c_n, n_viol_c_n_ca, n_clash, n_clash_inter) of one structure, host twins."""
    from abx_amd import metrics
    args = (x[None].float(), c['mask'][None], c['aa'][None], c['chain'][None], c['residx'][None])
    v = metrics.violation_counts(*args)[0].tolist()
    cl = metrics.clash_counts(*args)
    return v + [int(cl[0][0]), int(cl[1][0])]
