"""Inputs shared by tests/test_accuracy_host.py and tests/test_gpu_accuracy.py: mutated versions of the perturbed shipped complexes of
relax_cases (a design differs from the wild type in coordinates, residue types and atoms) and the call of the host twin on them."""
import numpy as np
import torch

GLY = 7


def mutate(c, x, seed):
    """Structure x (L,14,3) of complex c with seeded random tokens at the movable rows - at least one change to Gly and, where a movable
    row is Gly, one away from it - as a design: -> (x (L,14,3) float64 of float32 values, aa (L) int64, mask (L,14) bool).  The mask is
    the typed atom mask of the new tokens on the antibody rows and the crystal's on the antigen rows; slots the wild type lacks sit at
    the C-alpha plus a seeded offset."""
    from abx_amd import residue_constants as rc
    g = torch.Generator().manual_seed(1000 + seed)
    mi = torch.nonzero(c['mov'])[:, 0]
    aa = c['aa'].clone()
    aa[mi] = torch.randint(0, 20, (len(mi),), generator=g)
    not_gly = mi[c['aa'][mi] != GLY]
    aa[not_gly[int(torch.randint(0, len(not_gly), (1,), generator=g))]] = GLY
    was_gly = mi[c['aa'][mi] == GLY]
    if len(was_gly):
        aa[was_gly[0]] = int(torch.randint(0, 7, (1,), generator=g))
    typed = torch.as_tensor(rc.restype_atom14_mask)[aa].bool()
    mask = torch.cat([typed[:c['Lab']], c['mask'][c['Lab']:]])
    x = x.clone()
    new = mask & ~c['mask']
    off = torch.randn(x.shape, generator=g, dtype=torch.float64)
    x[new] = (x[:, 1:2].expand(-1, 14, -1) + off)[new]
    return x.float().double(), aa, mask


def host(c, x, aa=None, mask=None, **kw):
    """accuracy_host of structure x of complex c against the crystal structure (region: the movable set unless given)."""
    from abx_amd import accuracy
    kw.setdefault('region', c['mov'])
    return accuracy.accuracy_host(x, c['mask'] if mask is None else mask, c['aa'] if aa is None else aa, c['x'], c['mask'], c['aa'], c['Lab'], **kw)


def rigid(seed):
    """A seeded proper rotation (3,3) and translation (3) in float64."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    a, b, c, d = q / np.linalg.norm(q)
    R = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                  [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                  [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])
    return R, rng.normal(size=3) * 20
