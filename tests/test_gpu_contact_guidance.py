"""Interface guidance on the GPU (csrc/contact.hip, abx_contact_grad, abx_amd.guidance.InterfaceGuidance): the kernels against the float64
twin and its autograd gradient on the cases of contact_cases.py (whose branches test_contact_guidance_host.py asserts), each term alone,
batch independence, the score formula inside the sampler, graph replay of the composed guidance, and the design driver."""
import os

import numpy as np
import pytest
import torch

import contact_cases as CC
from analysis_gpu_cases import DEV, gpu_model, names, ops, pdb_args, sample_tiny, tiny_batch          # noqa: F401

pytestmark = pytest.mark.gpu


def check(a, b, tol, name):
    """The helper of test_gpu_kernels.py: the largest error relative to the largest reference value."""
    assert a.shape == b.shape, (name, a.shape, b.shape)
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    e = float((a - b).abs().max() / (b.abs().max() + 1e-30))
    assert np.isfinite(e) and e <= tol, f'{name}: rel err {e:.3e} > {tol}'


def run(ops, c, sel=None, restraints=True, hotspots=True, **kw):
    """abx_contact_grad on case c (sel: the samples to keep) -> (energy, grad_atom, grad_trans, grad_rot) on the host."""
    from abx_amd.ops import ContactTables
    s = slice(None) if sel is None else sel
    tables = ContactTables(DEV, c['hotspots'] if hotspots else None, c['restraints'] if restraints else None)
    out = ops.contact_grad(c['x'][s].to(DEV), c['exists'][s].to(DEV), c['moved'][s].to(DEV), c['target'].to(DEV), c['frame_trans'][s].to(DEV), tables,
                           **dict(CC.KW, **kw))
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


@pytest.mark.parametrize('case', ['small_case', 'l352_case'])
def test_contact_grad_vs_twin_autograd(ops, case):
    """Energies and analytic gradients against contact_energy_host and its autograd gradient, the frame pull-back against the same
    gradients: the bounds of test_clash_grad_vs_oracle_autograd (2e-5 energies, 5e-5 gradients, relative to the largest reference value)."""
    c = getattr(CC, case)()
    e, ga, gt, gr = run(ops, c)
    for k, name in enumerate(('contact', 'hotspot', 'restraint')):
        print(name, 'energy', e[:, k].tolist(), c['energy'][:, k].tolist())
        assert float(c['energy'][:, k].abs().max()) > 1e-2
        check(e[:, k], c['energy'][:, k], 2e-5, name + ' energy')
    print('gradient errors', float((ga.double() - c['grad']).abs().max()), float((gt.double() - c['grad_trans']).abs().max()),
          float((gr.double() - c['grad_rot']).abs().max()), 'of', float(c['grad'].abs().max()), float(c['grad_trans'].abs().max()), float(c['grad_rot'].abs().max()))
    check(ga, c['grad'], 5e-5, 'atom gradients')
    check(gt, c['grad_trans'], 5e-5, 'frame translation gradient')
    check(gr, c['grad_rot'], 5e-5, 'frame rotation gradient (torque)')
    # each term's gradient on its own, so that a small term cannot hide behind a large one
    for k, kw in enumerate((dict(w_hot=0.0, restraints=False), dict(w_contact=0.0, restraints=False), dict(w_contact=0.0, w_hot=0.0))):
        ga1 = run(ops, c, **kw)[1]
        xd = c['x'].double().requires_grad_(True)
        CC.twin(c, xd)[:, k].sum().backward()
        ref = xd.grad * (c['exists'] & c['moved'][..., None])[..., None]
        print('term', k, 'gradient error', float((ga1.double() - ref).abs().max()), 'of', float(ref.abs().max()))
        check(ga1, ref, 5e-5, f'atom gradients of term {k}')


def test_each_term_alone_leaves_the_others_at_zero(ops):
    c = CC.small_case()
    full = run(ops, c)[0]
    for k, kw in ((0, dict(w_hot=0.0, restraints=False)), (1, dict(w_contact=0.0, restraints=False)), (2, dict(w_contact=0.0, w_hot=0.0)),
                  (0, dict(restraints=False, hotspots=False)), (2, dict(w_contact=0.0, hotspots=False))):         # (the last two: no table at all)
        e = run(ops, c, **kw)[0]
        others = [j for j in range(3) if j != k]
        assert float(e[:, others].abs().max()) == 0.0, (k, e)
        assert torch.equal(e[:, k], full[:, k]) and bool((e[:2, k] != 0).all()), (k, e, full)
    assert float(full[2].abs().max()) == 0.0                                # a sample without a moved row: exactly nothing


def test_unmoved_rows_are_zero_and_samples_do_not_see_each_other(ops):
    """Gradients on rows that are not moved are exactly 0; a sample computed alone is bit-equal to the same sample inside the batch."""
    for c in (CC.small_case(), CC.l352_case()):
        full = run(ops, c)
        for t in full[1:]:
            assert float(t[~c['moved']].abs().max()) == 0.0
        assert float(full[1][~c['exists']].abs().max()) == 0.0
        assert float(full[1][c['moved']].abs().max()) > 0.1
        for b in range(c['B']):
            alone = run(ops, c, sel=slice(b, b + 1))
            for a, f in zip(alone, full):
                assert torch.equal(a[0], f[b]), b
    c = CC.small_case()
    swapped = run(ops, c, sel=[2, 1, 0])
    for a, f in zip(swapped, run(ops, c)):
        assert torch.equal(a, f[[2, 1, 0]])


def _tiny_guide(batch, cls=None, **kw):
    """Interface guidance of the tiny workload (L = 20, the antigen = rows 16..19) that acts whatever the seeded weights predict: a contact
    shell out to 30 A, every antigen row a hotspot, one restraint from a diffused CA to an antigen CA."""
    from abx_amd.guidance import InterfaceGuidance
    restraints = (torch.tensor([[6, 1, 17, 1], [5, 0, 7, 2]], dtype=torch.int32), torch.tensor([[0.0, 3.0, 1.0], [5.0, 6.0, 0.5]]))
    return (cls or InterfaceGuidance)(batch, w_contact=1.0, d0=4.0, d1=30.0, hotspots=[16, 17, 18, 19], w_hot=1.0, restraints=restraints, **kw)


def test_sampler_hands_reverse_the_guided_scores(gpu_model, cfg):
    """The pattern of test_guidance_off_is_bit_identical_and_on_follows_the_formula: the scores that leave the guidance are the model's
    scores minus the scaled frame gradients of the kernel's own outputs, on diffused residues only."""
    from abx_amd.guidance import InterfaceGuidance, quat_to_rot
    batch, sid = tiny_batch(gpu_model)
    seen = []

    class Spy(InterfaceGuidance):
        def __call__(self, b, out, rot_score, trans_score, diffuse_mask):
            rot, trans = super().__call__(b, out, rot_score, trans_score, diffuse_mask)
            e, _, g_t, g_r = self.energy_and_grads(b, out, diffuse_mask)
            R = quat_to_rot(out['heads']['folding']['rigids'][..., :4])
            m = diffuse_mask.float()[..., None]
            exp_t = trans_score - (self.scale_trans / 0.1) * g_t * m
            exp_r = rot_score - self.scale_rot * torch.einsum('...ji,...j->...i', R, g_r) * m
            seen.append((float((trans - exp_t).abs().max()), float((rot - exp_r).abs().max()), self.last_energy.clone(), torch.equal(self.last_energy, e),
                         float((trans - trans_score).abs().max()), float((rot - rot_score)[~diffuse_mask.bool()].abs().max()),
                         float(g_t[~diffuse_mask.bool()].abs().max())))
            return rot, trans

    guide = _tiny_guide(batch, cls=Spy, scale_trans=0.02, scale_rot=0.02)
    plain = sample_tiny(gpu_model, cfg, batch, sid)
    guided = sample_tiny(gpu_model, cfg, batch, sid, guidance=guide)
    assert len(seen) == 4 and all(s[0] < 1e-9 and s[1] < 1e-5 and s[3] for s in seen), [s[:2] for s in seen]
    assert all(s[5] == 0.0 and s[6] == 0.0 for s in seen)                         # nothing on fixed residues
    assert tuple(seen[0][2].shape) == (3, 3) and float(seen[0][2].abs().sum()) > 0 and seen[0][4] > 0, seen[0]
    assert not torch.equal(guided[0]['rigids_t'], plain[0]['rigids_t'])
    fixed = batch['fixed_mask'].bool()
    assert torch.equal(guided[0]['rigids_t'][fixed], plain[0]['rigids_t'][fixed])
    assert torch.isfinite(guided[-1]['rigids_t']).all()


def test_graph_replay_of_the_composed_guidance_equals_eager(gpu_model, cfg):
    """Sum(ViolationGuidance, InterfaceGuidance) inside the captured step: no host synchronisation, no host-to-device copy on the step path,
    and the same trajectory as the eager loop, record by record."""
    from abx_amd.guidance import Sum, ViolationGuidance
    batch, sid = tiny_batch(gpu_model)
    runs = []
    for use_graph in (False, True):
        guide = Sum(ViolationGuidance(scale_trans=0.02, scale_rot=0.02), _tiny_guide(batch, scale_trans=0.02, scale_rot=0.02))
        runs.append(sample_tiny(gpu_model, cfg, batch, sid, guidance=guide, use_graph=use_graph))
    only_violation = sample_tiny(gpu_model, cfg, batch, sid, guidance=ViolationGuidance(scale_trans=0.02, scale_rot=0.02))
    assert len(runs[0]) == len(runs[1]) == 5
    for k, (e, g) in enumerate(zip(*runs)):
        assert torch.equal(e['seq'], g['seq']) and torch.equal(e['rigids_t'].double(), g['rigids_t'].double()), f'step {k}'
        assert torch.equal(e['atom14_results'], g['atom14_results'])
    assert not torch.equal(runs[0][1]['rigids_t'], only_violation[1]['rigids_t'])          # the interface term did act


def test_design_driver_with_interface_guidance(tmp_path):
    """BASELINE config 4 shape on 6ct7 with and without the two new flags: the same file names; the fixed backbone stays where it is
    (3 decimals of a PDB file, the criterion of the config 4 test of test_gpu_model.py); the diffused residues move."""
    from abx_amd import design
    from abx_amd.io.pdb_reader import read_pdb, chain_feature
    common = pdb_args(['6ct7_H_L_S']) + ['--num_samples', '2', '--mode', 'optimize', '--optimize_steps', '10']
    guided = design.main(common + ['--guidance_contact', '1', '--guidance_hotspots', 'epitope', '--output_dir', str(tmp_path / 'guided')])
    plain = design.main(common + ['--output_dir', str(tmp_path / 'plain')])
    assert names(guided) == names(plain) and sorted(os.listdir(tmp_path / 'guided')) == sorted(os.listdir(tmp_path / 'plain'))
    pdbs = [n for n in names(plain) if n.endswith('.pdb')]
    assert len(pdbs) == 2
    fixed = [i for i in range(113) if not 98 <= i <= 100]
    moved = 0.0
    for n in pdbs:
        hp, hg = (chain_feature(read_pdb(str(tmp_path / d / n))['H'])['coords'][:113, :4] for d in ('plain', 'guided'))
        assert np.isfinite(hg).all()
        print(n, 'fixed', float(np.nanmax(np.abs(hp[fixed] - hg[fixed]))), 'diffused', float(np.nanmax(np.abs(hp[98:101] - hg[98:101]))))
        assert float(np.nanmax(np.abs(hp[fixed] - hg[fixed]))) < 2.1e-3
        moved = max(moved, float(np.nanmax(np.abs(hp[98:101] - hg[98:101]))))
    assert moved > 1e-3, 'the interface guidance changed nothing on the diffused residues'
