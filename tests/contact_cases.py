"""The cases that the host and the GPU tests of the interface guidance share (test_contact_guidance_host.py, test_gpu_contact_guidance.py):
ONE structure per sample (the predicted atoms on the moved rows, the crystal structure elsewhere), the moved rows, the partner rows, hotspot
rows and a restraint table.  Importing it touches no GPU; the float64 twin's energies and autograd gradients are computed once per case."""
import functools

import torch

KW = dict(w_contact=0.7, d0=4.0, d1=8.0, w_hot=1.3, d_hot=8.0, beta=1.0)
EXACT = {'d0': ((0, 1), (23, 1)), 'd1': ((22, 1), (24, 1))}        # sample 0 of the small case: (row, slot) pairs set exactly d0 / d1 apart


def _exists(seq):
    from abx_amd import residue_constants as rc
    return torch.as_tensor(rc.restype_atom14_mask)[seq].bool().clone()


def _restraints(pairs, gen, gt):
    """Restraints on the (row, slot) pairs: bounds of +-0.2 A about the crystal distance (satisfied there), so that what they cost in a
    sample comes from the moved rows alone."""
    idx, par = [], []
    for (ri, si, rj, sj) in pairs:
        dg = float((gt[ri, si] - gt[rj, sj]).norm())
        idx.append([ri, si, rj, sj])
        par.append([dg - 0.2, dg + 0.2, float(0.5 + torch.rand((), generator=gen))])
    return idx, par


@functools.lru_cache(maxsize=None)
def small_case():
    """L = 37, Lab = 23, B = 3: moved rows {0, 9, 10, 11, 22} in sample 0, {4, 5, 6, 17, 18, 30} in sample 1 (30 is a partner row AND a
    hotspot: it leaves both roles there), none in sample 2.  Row 10 (moved) and row 27 (a hotspot) are glycines; slots are missing on both
    sides; hotspot 33 is far from every designed residue."""
    g = torch.Generator().manual_seed(4)
    B, L, Lab = 3, 37, 23
    seq = torch.randint(0, 20, (L,), generator=g)
    seq[10] = 7
    seq[27] = 7                                                     # glycine: no CB
    seq[[0, 9, 11, 22, 4, 17, 23, 24, 25, 30]] = torch.tensor([1, 11, 18, 3, 13, 9, 10, 17, 14, 6])     # long side chains where it matters
    ex1 = _exists(seq)
    ex1[26, 3] = False                                              # a partner atom the crystal lacks
    ex1[31, 5:] = False
    centre = 3.0 * torch.randn(L, 3, generator=g)
    centre[:Lab] += torch.tensor([40.0, 0.0, 0.0])                 # the antibody's crystal rows: far from the partner rows
    centre[33] += torch.tensor([0.0, 19.0, 0.0])
    gt = centre[:, None] + 1.5 * torch.randn(L, 14, 3, generator=g)
    gt[23, 1] = torch.round(gt[23, 1] * 64) / 64                    # exactly representable: the pairs placed exactly d0 / d1 apart
    gt[24, 1] = torch.round(gt[24, 1] * 64) / 64
    sets = [[0, 9, 10, 11, 22], [4, 5, 6, 17, 18, 30], []]
    moved = torch.zeros(B, L, dtype=torch.bool)
    x = gt[None].repeat(B, 1, 1, 1)
    exists = ex1[None].repeat(B, 1, 1)
    for b, rows in enumerate(sets):
        moved[b, rows] = True
        for r in rows:                                              # the "predicted" residue: beside the partner rows
            c = 2.5 * torch.randn(3, generator=g) + torch.tensor([4.5, 0.0, 0.0])
            x[b, r] = c + 1.5 * torch.randn(14, 3, generator=g)
    exists[0, 9, 6:] = False                                        # a moved residue typed as a shorter one
    exists[1, 17, 4] = False                                        # a moved residue without CB
    x[0, 0, 1] = gt[23, 1] + torch.tensor([4.0, 0.0, 0.0])
    x[0, 22, 1] = gt[24, 1] + torch.tensor([0.0, 8.0, 0.0])
    x = x.float()
    target = torch.arange(L) >= Lab
    hotspots = [24, 27, 30, 33]
    pairs = [(9, 1, 11, 1), (9, 0, 10, 2), (0, 1, 22, 1), (10, 1, 25, 1), (11, 2, 28, 0), (22, 4, 3, 1), (0, 4, 15, 4), (9, 2, 29, 2),      # sample 0
             (4, 1, 6, 1), (5, 0, 17, 2), (18, 1, 26, 1), (30, 1, 2, 1), (6, 2, 24, 0), (17, 1, 31, 2),                                       # sample 1
             (10, 4, 25, 1)]                                                                                                                  # CB of a glycine
    idx, par = _restraints(pairs, g, gt.float())
    idx += [[9, 1, 25, 1], [5, 1, 26, 1]]                           # wide bounds: the flat bottom in a sample where an end moves
    par += [[0.0, 80.0, 1.0], [0.0, 80.0, 1.0]]
    for b, (ri, si, rj, sj) in ((0, (9, 1, 28, 1)), (1, (5, 1, 27, 1))):       # half an Angstrom outside: the quadratic branch, flat in the crystal
        ds, dg = float((x[b, ri, si] - x[b, rj, sj]).norm()), float((gt[ri, si] - gt[rj, sj]).norm())
        assert abs(ds - dg) > 0.5
        idx.append([ri, si, rj, sj])
        par.append([min(dg, ds - 0.5) - 1.0, ds - 0.5, 1.0] if dg < ds else [ds + 0.5, max(dg, ds + 0.5) + 1.0, 1.0])
    restraints = (torch.tensor(idx, dtype=torch.int32), torch.tensor(par, dtype=torch.float32))
    return finish(dict(B=B, L=L, Lab=Lab, x=x, exists=exists, moved=moved, target=target, hotspots=hotspots, restraints=restraints))


@functools.lru_cache(maxsize=None)
def l352_case():
    """synthetic.WORKLOADS['L352'], B = 2: 22 tiles (the last one partly filled) and more rows than the 256 threads of the frame kernel
    cover.  Sample 0 moves the 13 rows of the CDR, sample 1 ten antibody rows and six partner rows beyond row 256."""
    from abx_amd import synthetic
    cx = synthetic.make_complex(seed=2, **synthetic.WORKLOADS['L352'])
    g = torch.Generator().manual_seed(31)
    B, L, Lab = 2, 352, 228
    gt, ex1 = cx['atom14_gt_positions'].float(), cx['atom14_gt_exists'].bool()
    sets = [list(range(97, 110)), list(range(20, 30)) + list(range(300, 306))]
    moved = torch.zeros(B, L, dtype=torch.bool)
    x = gt[None].repeat(B, 1, 1, 1)
    exists = ex1[None].repeat(B, 1, 1)
    near = gt[Lab:, 1].mean(0)
    for b, rows in enumerate(sets):
        moved[b, rows] = True
        for r in rows:
            c = gt[Lab + int(torch.randint(0, L - Lab, (), generator=g)), 1] + 3.0 * torch.randn(3, generator=g)
            x[b, r] = 0.7 * c + 0.3 * near + 1.5 * torch.randn(14, 3, generator=g)
            exists[b, r] = _exists(torch.randint(0, 20, (1,), generator=g))[0]          # typed by a predicted token
    target = torch.arange(L) >= Lab
    ca = x[0, sets[0], 1]
    hotspots = sorted(set((Lab + torch.cdist(ca, gt[Lab:, 1]).argmin(1)).tolist()))[:6] + [340]
    pairs = [(97 + k, 1, 230 + 9 * k, 1) for k in range(12)] + [(20 + k, 2, 21 + k, 0) for k in range(8)] + [(300, 1, 240, 4), (304, 0, 25, 1)]
    idx, par = _restraints(pairs, g, gt)
    restraints = (torch.tensor(idx, dtype=torch.int32), torch.tensor(par, dtype=torch.float32))
    return finish(dict(B=B, L=L, Lab=Lab, x=x, exists=exists, moved=moved, target=target, hotspots=hotspots, restraints=restraints))


def twin(c, x=None, details=False, **kw):
    from abx_amd.guidance import contact_energy_host
    return contact_energy_host(c['x'].double() if x is None else x, c['exists'], c['moved'], c['target'], hotspots=c['hotspots'],
                               restraints=c['restraints'], details=details, **dict(KW, **kw))


def finish(c):
    """Adds the frame origins (the CA atoms) and the twin's answers: energy (B,3), info, and the autograd gradient of the summed energy
    restricted to the existing atoms of the moved rows, with its frame pull-back."""
    c['frame_trans'] = c['x'][:, :, 1].contiguous()
    xd = c['x'].double().requires_grad_(True)
    e, info = twin(c, xd, details=True)
    e.sum().backward()
    c['energy'], c['info'] = e.detach(), info
    c['grad'] = xd.grad * (c['exists'] & c['moved'][..., None])[..., None]
    c['grad_trans'] = c['grad'].sum(2)
    c['grad_rot'] = torch.cross(c['x'].double() - c['frame_trans'].double()[:, :, None], c['grad'], dim=-1).sum(2)
    return c
