"""Inputs shared by tests/test_shape_host.py and tests/test_gpu_shape.py: the shipped complexes as the shape analysis takes them, the
numbers a numpy prototype of the definition printed for them, and structures with a small, an empty and a removed interface."""
import functools

import torch

import relax_cases as RC

# A prototype of the definition on the crystal complexes (region = CDR-H3, trim 1.5, weight 0.5, probe 1.4): per point density the row's
# float columns 0-3 and the integers |I|, |E|, kept per side and the region dots
PROTOTYPE = {
    ('6ct7', 128): dict(sc=(0.549, 0.574, 0.524, 0.573), buried=(701, 881), open=(428, 437), kept=(347, 532), region=82),
    ('6qd7', 128): dict(sc=(0.0, 0.0, 0.0, 0.0), buried=(68, 74), open=None, kept=(8, 0), region=0),
}
# Sc of 6ct7 against the dot density, and antibody -> antigen / antigen -> antibody at 512
DENSITY = {64: 0.462, 128: 0.549, 256: 0.590, 512: 0.615}
DENSITY_512 = (0.648, 0.581)
# the seeded perturbations of CDR-H3 of 6ct7 (relax_cases.SEEDS): the whole interface, and the CDR-H3 dots
PERTURBED = {5: (0.545, 0.544), 6: (0.530, 0.339), 7: (0.494, 0.347)}
G = 7                                   # the Gly token
SMALL_SHIFT = 14.0                      # antibody_moved(6ct7, 14): 8 / 8 buried and 51 / 64 open dots at P = 128


@functools.lru_cache(maxsize=None)
def complex_of(code):
    return RC.load_complex(code, 'h3')


def batch_of(c, device, res_mask=None, x=None):
    """The un-batched complex of relax_cases.load_complex as a scorer takes it, on `device`; x: other ground-truth coordinates."""
    b = {'seq': c['aa'], 'atom14_gt_positions': (c['x'] if x is None else x).float(), 'atom14_gt_exists': c['mask'],
         'anchor_flag': torch.zeros(c['Lab']), 'chain_id': c['chain'], 'residx': c['residx'], 'cdr_def': c['cdr']}
    if res_mask is not None:
        b['mask'] = res_mask
    return {k: v.to(device) for k, v in b.items()}


def twin(c, x, mask, pts, seq=None, **kw):
    """shape_host of structure x of complex c with region = its movable set."""
    from abx_amd import shape
    return shape.shape_host(x, mask, c['aa'] if seq is None else seq, c['Lab'], region=c['mov'], points=pts, **kw)


def structures(c):
    """(4, L, 14, 3) float64: the crystal structure and its three seeded perturbations."""
    return torch.stack([c['x'].float().double()] + [RC.perturb(c, s) for s in RC.SEEDS])


def antibody_moved(c, distance):
    """The crystal structure with the antibody moved `distance` Angstrom away from the antigen along the line between the two centres."""
    Lab, m = c['Lab'], c['mask']
    n = c['x'][:Lab][m[:Lab]].mean(0) - c['x'][Lab:][m[Lab:]].mean(0)
    x = c['x'].clone()
    x[:Lab] += distance * n / n.norm()
    return x.float().double()


def antigen_moved(c, distance=100.0):
    """The crystal structure with the antigen moved `distance` Angstrom along x: no interface is left."""
    x = c['x'].clone()
    x[c['Lab']:, :, 0] += distance
    return x.float().double()
