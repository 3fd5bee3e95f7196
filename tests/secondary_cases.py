"""Inputs shared by tests/test_secondary_host.py and tests/test_gpu_secondary.py: 12-residue chains built from given (phi, psi) whose
state strings and bond lists are written down, two-strand sheets placed by a written-down rotation or translation, the twin on a
complex of relax_cases, the structures the GPU test scores, concatenated chains of a given length and the edge helpers (a residx gap, a
missing O, a row taken out by res_mask).  Importing it touches no GPU."""
import numpy as np
import torch

import relax_cases as RC
import torsions_cases as TC

N_RES = 12
# (phi, psi, the expected state string, the step n of its bonds donor i + n -> acceptor i, the number of bonds); omega = 180
CHAINS = ((-57.0, -47.0, '-HHHHHHHHHH-', 4, 8), (-49.0, -26.0, '-GGGGGGGGGG-', 3, 9), (-57.0, -70.0, '-IIIIIIIIII-', 5, 7),
          (-139.0, 135.0, '------------', 0, 0), (-75.0, 145.0, '------------', 0, 0))
BOTH_TURNS = (-60.0, -35.0)                            # a helix with the i+3 AND the i+4 bonds (17): H by priority, G with it reversed
STRAND = (-139.0, 135.0)
N_STRAND = 7
SHEET_STRING = '-EEEEE--EEEEE-'
# the antiparallel partner: the strand rotated by 180 degrees about the axis of direction e1 through cen + 2.2 (cos 75 e1 + sin 75 e2)
ANTI_OFFSET, ANTI_ANGLE = 2.2, 75.0
# the parallel partner: the strand translated by 4.4 (cos 135 e1 + sin 135 e2), found by a search on the host over 4.4 .. 5.2 A,
# steps of 15 degrees and shifts along the axis: 120 and 135 degrees give five parallel bridge pairs for shifts of -0.5 .. 0.5 A
PAR_DISTANCE, PAR_ANGLE = 4.4, 135.0
SEEDS = RC.SEEDS


def chain_of(phi, psi, n=N_RES):
    """Poly-Ala of n residues with the given phi / psi and omega = 180 -> (x (n,14,3) float64 of float32 values, mask (n,14) bool)."""
    return TC.build_chain(np.full(n, float(phi)), np.full(n, float(psi)), np.full(n, 180.0))


def built_chains():
    """The five chains of CHAINS -> list of dict(x, mask, letters, bonds: the expected [donor, acceptor] list)."""
    out = []
    for phi, psi, letters, step, n_bonds in CHAINS:
        x, mask = chain_of(phi, psi)
        bonds = [[i + step, i] for i in range(N_RES - step)] if step else []
        assert len(bonds) == n_bonds
        out.append(dict(x=x, mask=mask, letters=letters, bonds=bonds))
    return out


def _strand_frame(x):
    ca = x[:, 1]
    ax = ca[-1] - ca[0]
    ax = ax / np.linalg.norm(ax)
    e1 = np.cross(ax, [0.0, 0.0, 1.0])
    e1 = e1 / np.linalg.norm(e1)
    return ax, ca.mean(0), e1, np.cross(ax, e1)


def sheet(parallel=False):
    """Two strands of N_STRAND residues with chain ids 0 and 1 -> dict(x (14,14,3), mask, chain, letters, bonds, anti, par: the expected
    string, number of bonds and of antiparallel / parallel bridge pairs)."""
    x, mask = chain_of(*STRAND, n=N_STRAND)
    ax, cen, e1, e2 = _strand_frame(x)
    if parallel:
        r = np.deg2rad(PAR_ANGLE)
        x2 = x + PAR_DISTANCE * (np.cos(r) * e1 + np.sin(r) * e2)
    else:
        r = np.deg2rad(ANTI_ANGLE)
        p = cen + ANTI_OFFSET * (np.cos(r) * e1 + np.sin(r) * e2)
        d = x - p
        x2 = p + 2.0 * (d @ e1)[..., None] * e1 - d
    xs = np.concatenate([x, x2]).astype(np.float32).astype(np.float64)
    xs[:, 5:] = 0.0
    return dict(x=xs, mask=np.concatenate([mask, mask]), chain=np.repeat([0, 1], N_STRAND), letters=SHEET_STRING, bonds=6,
                anti=0 if parallel else 5, par=5 if parallel else 0)


def as_complex(x, mask, chain=None, residx=None):
    """Poly-Ala rows as a complex of relax_cases.load_complex (no antigen, every residue in the region)."""
    n = x.shape[0]
    return dict(x=torch.from_numpy(np.asarray(x, np.float64)), mask=torch.from_numpy(np.asarray(mask, bool)), aa=torch.zeros(n, dtype=torch.long),
                chain=torch.zeros(n, dtype=torch.long) if chain is None else torch.as_tensor(np.asarray(chain)).long(),
                residx=torch.arange(n) if residx is None else torch.as_tensor(np.asarray(residx)).long(), cdr=torch.zeros(n, dtype=torch.long),
                mov=torch.ones(n, dtype=torch.bool), Lab=n)


def concatenated(n):
    """n rows: the built chains and the two sheets one after the other, each piece with a chain id of its own and 40 A from the last,
    repeated and cut at n rows (a cut piece stays a shorter chain)."""
    pieces = [(o['x'], o['mask'], None) for o in built_chains()] + [(s['x'], s['mask'], s['chain']) for s in (sheet(), sheet(True))]
    xs, ms, ch = [], [], []
    k = cid = 0
    while sum(len(v) for v in xs) < n:
        x, m, c = pieces[k % len(pieces)]
        xs.append(x + np.array([40.0 * k, 0.0, 0.0]))
        ms.append(m)
        ch.append(cid + (np.zeros(len(x), int) if c is None else np.asarray(c)))
        cid = int(ch[-1].max()) + 1
        k += 1
    x = np.concatenate(xs)[:n].astype(np.float32).astype(np.float64)
    return as_complex(x, np.concatenate(ms)[:n], np.concatenate(ch)[:n])


def twin(c, x=None, mask=None, seq=None, wild_x=None, res_mask=None, **kw):
    """secondary_host of structure x of complex c against its crystal structure, region = its movable set."""
    from abx_amd import secondary
    return secondary.secondary_host(c['x'] if x is None else x, c['mask'] if mask is None else mask, c['aa'] if seq is None else seq,
                                    c['x'] if wild_x is None else wild_x, c['mask'], c['aa'], c['Lab'], c['chain'], c['residx'], region=c['mov'],
                                    res_mask=res_mask, **kw)


def gpu_structures(c):
    """What the GPU test scores of a shipped complex in one batch: the wild type, the three seeded perturbations and their mutated
    versions (Ala / Gly / Pro in turn: Pro removes donors), 7 (x, tokens, mask) triples - the arrangement of torsions_cases."""
    return TC.gpu_structures(c)


def tiny_structures():
    """The tiny synthetic workload (Lab = 16) and two noisy copies of its antibody -> (cx, xh (2,Lab,14,3) float32, region (L) bool)."""
    return TC.tiny_structures()


def synthetic_twin(cx, x, region, **kw):
    """secondary_host of a design x (Lab,14,3) of a synthetic complex whose rows have the atoms of their tokens."""
    from abx_amd import residue_constants as rc, secondary
    Lab = cx['anchor_flag'].shape[0]
    typed = torch.as_tensor(rc.restype_atom14_mask)[cx['seq'][:Lab]].bool()
    return secondary.secondary_host(x, typed, cx['seq'], cx['atom14_gt_positions'], cx['atom14_gt_exists'], cx['seq'], Lab, cx['chain_id'],
                                    cx['residx'], region=region, res_mask=cx['mask'], **kw)


# ---- edge helpers on the 12-residue alpha helix (bonds i + 4 -> i, turns at 0..7, H at 1..10)
GAP_AT = 6


def helix_with_gap():
    """The helix with residx jumping by 2 before row GAP_AT: the link (5, 6) is gone."""
    x, mask = chain_of(*CHAINS[0][:2])
    residx = np.arange(N_RES)
    residx[GAP_AT:] += 1
    return as_complex(x, mask, residx=residx)


def helix_without_o(row=GAP_AT):
    """(complex, mask): the helix and an atom mask with the O of `row` missing: the row is not present."""
    x, mask = chain_of(*CHAINS[0][:2])
    m = mask.copy()
    m[row, 3] = False
    return as_complex(x, mask), torch.from_numpy(m)


def res_mask_without(n, row=GAP_AT):
    m = torch.ones(n, dtype=torch.uint8)
    m[row] = 0
    return m
