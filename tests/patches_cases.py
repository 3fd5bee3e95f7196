"""Inputs shared by tests/test_patches_host.py and tests/test_gpu_patches.py: the numbers a numpy prototype of the definition printed for
the two shipped complexes, the twin on a complex of relax_cases, and hand-built structures of a few residues whose answer is written down."""
import numpy as np
import torch

import relax_cases as RC

A, R, N, D, C, Q, E, G, H, I, L_, K, M, F, P, S, T, W, Y, V = range(20)
X = 20
TWO30 = float(1 << 30)
# A prototype of the definition on the crystal complexes (region = CDR-H3, P = 128, probe 1.4, the default thresholds): the float columns
# to the printed digits, the integers n_cdr, n_exposed, n_vicinity, n_pairs, n_salt, n_cross, n_cross_region
PROTOTYPE = {
    '6ct7': dict(psh='46.972', ppc='0.0527', pnc='0.2984', sfvcsp='5.51', psh_region='4.357', cross_attract='0.2399', cross_repel='0.1752',
                 counts=(42, 135, 46, 220, 4, 12, 1)),
    '6qd7': dict(psh='42.521', ppc='0.2301', pnc='0.0000', sfvcsp='4.40', psh_region='13.834', cross_attract='0.00193', cross_repel='0.0000',
                 counts=(48, 135, 47, 198, 2, 1, 0)),
}
PSH_WITHOUT_OVERRIDE = {'6ct7': '45.075'}
# the seeded perturbations of 6ct7 (relax_cases.SEEDS): n_vicinity and n_pairs
PERTURBED = {5: (48, 238), 6: (47, 232), 7: (47, 231)}
FREE_COLUMNS = (0, 1, 2, 3, 4, 5, 6, 11, 12, 13, 14, 15)       # the columns of the free antibody
CROSS_COLUMNS = (7, 8, 9, 10, 16, 17)


def twin(c, x, mask, pts, seq=None, **kw):
    """patches_host of structure x of complex c with region = its movable set."""
    from abx_amd import patches
    return patches.patches_host(x, mask, c['aa'] if seq is None else seq, c['Lab'], c['chain'], c['residx'], c['cdr'], region=c['mov'],
                                points=pts, **kw)


def structures(c):
    """(4, L, 14, 3) float64: the crystal structure and its three seeded perturbations."""
    return torch.stack([c['x'].float().double()] + [RC.perturb(c, s) for s in RC.SEEDS])


def cut_complex(c, L):
    """The complex cut to its first L rows (L > Lab)."""
    assert c['Lab'] < L <= c['aa'].shape[0]
    return {k: (v[:L] if torch.is_tensor(v) and v.dim() and v.shape[0] == c['aa'].shape[0] else v) for k, v in c.items()}


def hand_built(types, centres, cdr, Lab=None, chain=None, region=None, n_points=128):
    """A structure of len(types) residues for patches_host: every atom of residue r sits AT centres[r], so the closest approach of two
    residues - and of their charged atoms - is the distance of their centres; every atom is fully accessible (acc_alone = n_points), so
    every residue with a side chain is exposed.  -> the keyword-free arguments of patches_host as a dict."""
    from abx_amd import residue_constants as rc
    n = len(types)
    aa = np.asarray(types, np.int64)
    mask = np.asarray(rc.restype_atom14_mask)[aa] != 0
    x = np.repeat(np.asarray(centres, np.float32)[:, None, :], 14, 1)
    pts = np.full((n, 14, 2), n_points, np.int32)
    return dict(x=x, mask=mask, aa=aa, Lab=n if Lab is None else Lab, chain_id=np.zeros(n, np.int64) if chain is None else np.asarray(chain),
                residx=np.arange(n), cdr_def=np.asarray(cdr, np.int64), region=region, points=pts)


def term(h2_or_q2, r2):
    """One fixed-point pair term as a column shows it: rint(2^30 * (product / r2)) / 2^30."""
    return float(np.rint(TWO30 * (h2_or_q2 / r2))) / TWO30
