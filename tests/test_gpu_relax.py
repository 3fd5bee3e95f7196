"""GPU checks of the violation relaxation (abx_relax, csrc/relax.hip; abx_amd.relax.ViolationRelaxer): energies and the generalised
gradient against float64 autograd of the host twin, the constant offset against abx_clash_grad, convergence on the perturbed loops of
the two shipped complexes, the invariants of the rigid-body + chi parametrisation, batch invariance at the headline size, and the
path through the sampler and the design driver."""
import os

import numpy as np
import pytest
import torch

from analysis_gpu_cases import (ALONE, CODES, DEV, SHARED, assert_same_bytes, l352_designs, names, pdb_args,
                                sample_tiny, spy_on_sampler, structure_inputs, table_lines, tiny_batch, ops, gpu_model)  # noqa: F401  (ops, gpu_model: set up once per importing module)
import relax_cases as RC

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def check(a, b, tol, name):
    assert a.shape == b.shape, (name, a.shape, b.shape)
    e = rel_err(a, b)
    print(f'{name}: rel err {e:.3e}')
    assert np.isfinite(e) and e <= tol, f'{name}: rel err {e:.3e} > {tol}'


def gpu_relax(ops, c, xs, Lp=None, **kw):
    """abx_relax on structures xs (B,L,14,3) of complex c (rows >= Lp come from the crystal structure, which is what xs holds there)."""
    x, sq, cplx, m, mov = structure_inputs(c, xs, Lp)
    return ops.relax(x, sq, *cplx, c['chain'].int().to(DEV), mov, Lab=c['Lab'], residx=c['residx'].int().to(DEV), mask=m, **kw)


def gpu_counts(ops, c, xs):
    """The five count columns of abx_design_scores for structures xs (B,L,14,3)."""
    x, sq, cplx, m, _ = structure_inputs(c, xs)
    s = ops.design_scores(x, sq, *cplx, c['cdr'].int().to(DEV), c['chain'].int().to(DEV), Lab=c['Lab'], residx=c['residx'].int().to(DEV), mask=m)
    return s[:, 14:].cpu().long().tolist()


def full_energy(ops, c, xs):
    """abx_clash_grad energies (B,3) of whole structures xs (B,L,14,3)."""
    B = xs.shape[0]
    d = lambda t: t.to(DEV)
    rep = lambda t: d(t[None].repeat(B, *([1] * t.dim())))
    return ops.clash_grad(d(xs.float()), rep(c['mask']), rep(c['aa']), rep(c['chain'].int()), d(xs[:, :, 1].float()), residx=rep(c['residx'].int()))[0].cpu().double()


def host_gradient(c, x, **kw):
    from abx_amd import relax
    _, rep, G = relax.relax_host(x, c['mask'], c['aa'], c['chain'], c['residx'], c['mov'], max_iter=0, return_grad=True, **kw)
    return rep, G


def compact_complex():
    """The compact random two-chain + antigen complex of test_gpu_kernels.py::test_clash_grad_vs_oracle_autograd (thousands of overlapping
    pairs, peptide bonds and angles off their flat bottoms, a cysteine pair, a proline, missing atoms, numbering gaps), two structures,
    with a movable set that holds the special rows and both ends of a chain."""
    from abx_amd import residue_constants as rc
    B, L = 2, 70
    ge = torch.Generator().manual_seed(90)
    aatype = torch.randint(0, 20, (B, L), generator=ge)
    aatype[:, 11] = 4; aatype[:, 40] = 4            # a cysteine pair (SG-SG excluded)
    aatype[:, 20] = 14                              # a proline after a peptide bond
    chain = torch.cat([torch.zeros(30), torch.ones(25), 17 * torch.ones(15)]).long()
    residx = torch.cat([torch.arange(30), torch.arange(25) + 512, torch.tensor([3, 4, 5, 9, 10, 11, 12, 40, 41, 42, 43, 44, 45, 46, 47])]).long()
    ca = torch.cumsum(1.6 * torch.randn(B, L, 3, generator=ge), dim=1)
    x = ca[:, :, None] + 1.2 * torch.randn(B, L, 14, 3, generator=ge)
    mask = torch.as_tensor(rc.restype_atom14_mask)[aatype].bool().clone()
    mask[1, 5] = False                               # a residue without atoms
    mask[0, 33, 4:] = False
    mask[1, 44, 1] = False                           # a missing CA: its angle terms drop out, the bond stays
    x[:, 1:, 0] = x[:, :-1, 2] + torch.tensor([1.33, 0., 0.]) + 0.25 * torch.randn(B, L - 1, 3, generator=ge) * (torch.rand(B, L - 1, 1, generator=ge) > 0.5)
    third = torch.rand(B, L - 1, 1, generator=ge) > 0.66
    x[:, :-1, 1] = torch.where(third, x[:, :-1, 2] + 1.52 * torch.tensor([-0.4473, 0.8944, 0.]) + 0.05 * torch.randn(B, L - 1, 3, generator=ge), x[:, :-1, 1])
    mov = torch.zeros(L, dtype=torch.bool)
    mov[[0, 5, 10, 11, 12, 19, 20, 29, 30, 33, 40, 44, 54, 55, 57, 58, 61, 62, 69]] = True
    return x.float(), mask, aatype, chain, residx, mov


def test_gradient_on_the_compact_random_complex(ops):
    """max_iter = 0: the three energies and the (B, M, 10) generalised gradient against float64 autograd of relax_host's energy with
    respect to (t, infinitesimal rotation about the C-alpha, chi) at the input state; weights and tolerances of
    test_clash_grad_vs_oracle_autograd (2e-5 energies, 5e-5 gradients); with and without the restraint (zero at the input state)."""
    from abx_amd import relax
    x, mask, aatype, chain, residx, mov = compact_complex()
    B, L = aatype.shape
    kw = dict(overlap_tolerance=1.5, between_chain_factor=0.2, bond_tolerance_factor=12.0, w_clash=0.7, w_bond=1.3, w_angle=0.9)
    d = lambda t: t.to(DEV)
    for rx in (None, residx):
        out, rep, G = ops.relax(d(x), d(aatype), d(x[0]), d(aatype[0]), d(mask[0]), d(chain.int()), d(mov), Lab=L, residx=None if rx is None else d(rx.int()),
                                mask=d(mask), max_iter=0, k_restraint=0.05, return_grad=True, **kw)
        assert torch.equal(out.cpu(), x) and G.shape == (B, int(mov.sum()), 10)
        rep = rep.cpu()
        assert rep[:, 7].tolist() == [1.0] * B and rep[:, 8].tolist() == [0.0] * B and torch.equal(rep[:, 0:3], rep[:, 3:6]) and rep[:, 6].tolist() == [0.0] * B
        for b in range(B):
            _, hrep, hG = relax.relax_host(x[b].double(), mask[b], aatype[b], chain, rx, mov, max_iter=0, return_grad=True, k_restraint=0.05, **kw)
            assert hrep[0] > 10 and hrep[1] > 0.1 and hrep[2] > 0.1, hrep                                  # all three terms are active
            for k, name in enumerate(('clash', 'bond', 'angle')):
                check(rep[b, k:k + 1], hrep[k:k + 1], 2e-5, f'compact b={b} residx={rx is not None}: {name} energy')
            assert float(hG[:, 6:].abs().max()) > 0.1
            check(G[b, :, 0:3].cpu(), hG[:, 0:3], 5e-5, f'compact b={b}: g_t')
            check(G[b, :, 3:6].cpu(), hG[:, 3:6], 5e-5, f'compact b={b}: torque')
            check(G[b, :, 6:10].cpu(), hG[:, 6:10], 5e-5, f'compact b={b}: g_chi')


@pytest.mark.parametrize('sel', ['h3', 'all'])
def test_gradient_on_the_perturbed_6qd7_loops(ops, sel):
    c = RC.load_complex('6qd7', sel)
    xs = torch.stack([RC.perturb(c, s) for s in RC.SEEDS])
    out, rep, G = gpu_relax(ops, c, xs, max_iter=0, return_grad=True)
    assert torch.equal(out.cpu(), xs.float())
    for b in range(len(RC.SEEDS)):
        hrep, hG = host_gradient(c, xs[b])
        assert hrep[0] > 0 and hrep[1] > 0 and hrep[2] > 0, hrep
        for k, name in enumerate(('clash', 'bond', 'angle')):
            check(rep[b, k:k + 1].cpu(), hrep[k:k + 1], 2e-5, f'6qd7 {sel} seed {RC.SEEDS[b]}: {name} energy')
        check(G[b, :, 0:3].cpu(), hG[:, 0:3], 5e-5, f'6qd7 {sel} seed {RC.SEEDS[b]}: g_t')
        check(G[b, :, 3:6].cpu(), hG[:, 3:6], 5e-5, f'6qd7 {sel} seed {RC.SEEDS[b]}: torque')
        check(G[b, :, 6:10].cpu(), hG[:, 6:10], 5e-5, f'6qd7 {sel} seed {RC.SEEDS[b]}: g_chi')


@pytest.mark.parametrize('code,sel', RC.MOVABLE_SETS)
def test_restricted_energy_differs_from_abx_clash_grad_by_a_constant(ops, code, sel):
    """abx_clash_grad (whole structure) of the output minus that of the input equals the report's after - before, to 2e-5 of the
    larger full energy - half-way through a relax (8 evaluations) and at its end."""
    c = RC.load_complex(code, sel)
    xs = torch.stack([RC.perturb(c, s) for s in RC.SEEDS])
    e_in = full_energy(ops, c, xs).sum(1)
    for iters in (8, 200):
        out, rep = gpu_relax(ops, c, xs, max_iter=iters)
        rep = rep.cpu()
        e_out = full_energy(ops, c, out.cpu().double()).sum(1)
        d_full, d_rep = e_out - e_in, rep[:, 3:6].sum(1) - rep[:, 0:3].sum(1)
        print(code, sel, iters, 'full', e_in.tolist(), e_out.tolist(), 'report delta', d_rep.tolist())
        assert bool((rep[:, 8] > 0).all()) and bool((d_rep < 0).all())
        assert bool(((d_full - d_rep).abs() <= 2e-5 * torch.maximum(e_in, e_out)).all()), (d_full, d_rep)


@pytest.mark.parametrize('code,sel', RC.MOVABLE_SETS)
def test_perturbed_loops_converge_and_keep_the_invariants(ops, code, sel):
    """The nine cases of the host test, one batch of three seeds per movable set, default parameters: E_after == 0 within the budget and
    all five count columns of abx_design_scores 0 where the input had violations; fixed rows bit-identical; rigid pieces rigid."""
    c = RC.load_complex(code, sel)
    xs = torch.stack([RC.perturb(c, s) for s in RC.SEEDS])
    before = gpu_counts(ops, c, xs)
    out, rep = gpu_relax(ops, c, xs)
    rep, out = rep.cpu(), out.cpu()
    after = gpu_counts(ops, c, out)
    print(code, sel, 'evaluations', rep[:, 7].tolist(), 'accepted', rep[:, 8].tolist(), 'counts before', before, 'after', after,
          'max CA shift', rep[:, 10].tolist())
    for b, seed in enumerate(RC.SEEDS):
        host = RC.counts(xs[b], c)
        assert before[b][:3] == host[:3] and min(before[b][:3]) > 0, (seed, before[b], host)
        assert (before[b][3] > 0) == (host[3] > 0) and abs(before[b][3] - host[3]) <= 1, (seed, before[b], host)
        assert after[b] == [0, 0, 0, 0, 0], (seed, after[b])
    assert bool((rep[:, 3:7] == 0).all()) and bool((rep[:, 7] <= 200).all()) and bool((rep[:, 7] > 5).all())
    assert bool((rep[:, 0:3].sum(1) > 0).all()) and bool((rep[:, 10] > 0.3).all()) and bool((rep[:, 10] < 3.0).all())
    check_invariants(c, xs, out, rep)


def check_invariants(c, xs, out, rep, k_restraint=0.0):
    """rows outside the movable set (every antigen row among them) bit-identical; E_after <= E_before; inside every movable residue the
    backbone + CB distances and the distances inside one rigid group preserved to 1e-3 A; the restraint bound."""
    from abx_amd import residue_constants as rc
    group = torch.as_tensor(rc.restype_atom14_to_rigid_group).long()
    mov = c['mov']
    assert out.shape == xs.shape
    assert torch.equal(out[:, ~mov], xs[:, ~mov].float())
    assert not bool(mov[c['Lab']:].any())
    assert bool((rep[:, 3:7].sum(1) <= rep[:, 0:3].sum(1)).all())
    worst = 0.0
    for b in range(xs.shape[0]):
        for i in torch.nonzero(mov)[:, 0].tolist():
            m = c['mask'][i]
            g = group[c['aa'][i]]
            piece = torch.arange(14) < 5                                    # N, CA, C, O, CB
            same = (piece[:, None] & piece[None]) | ((g[:, None] == g[None]) & (g[:, None] >= 4))
            same = same & m[:, None] & m[None]
            d0, d1 = torch.cdist(xs[b, i].double(), xs[b, i].double()), torch.cdist(out[b, i].double(), out[b, i].double())
            worst = max(worst, float(((d0 - d1).abs() * same).max()))
    print('largest change of a distance inside a rigid piece:', worst)
    assert worst <= 1e-3
    if k_restraint:
        shift2 = ((out.double() - xs.float().double())[:, mov, 1] ** 2).sum((1, 2))
        assert bool((k_restraint * shift2 <= rep[:, 0:3].sum(1) * (1 + 1e-5)).all()), (shift2, rep[:, 0:3].sum(1))
        assert bool(((k_restraint * shift2 - rep[:, 6]).abs() <= 1e-5 * rep[:, 0:3].sum(1)).all())


def mixed_batch(c):
    """B = 7: clean and perturbed structures side by side."""
    return torch.stack([c['x'].float().double(), RC.perturb(c, 5), RC.perturb(c, 6), c['x'].float().double(), RC.perturb(c, 7),
                        RC.perturb(c, 5, 0.35, 0.125, 0.25), c['x'].float().double()])


@pytest.mark.parametrize('k', [0.0, 0.05])
def test_invariants_on_a_mixed_batch(ops, k):
    """Clean structures come back bit-identical after one evaluation, beside perturbed ones that relax; with k_restraint = 0.05 the
    motion obeys k * sum |dCA|^2 <= E_viol(input) (1 + 1e-5)."""
    c = RC.load_complex('6qd7', 'h3')
    xs = mixed_batch(c)
    out, rep = gpu_relax(ops, c, xs, k_restraint=k)
    out, rep = out.cpu(), rep.cpu()
    print('k', k, 'report', rep.tolist())
    for b in (0, 3, 6):
        assert torch.equal(out[b], xs[b].float()) and rep[b].tolist() == [0.0] * 7 + [1.0, 0.0, float(np.float32(0.01)), 0.0]
    for b in (1, 2, 4, 5):
        assert rep[b, 8] > 0 and not torch.equal(out[b], xs[b].float())
        if k == 0.0:
            assert float(rep[b, 3:7].sum()) == 0.0
    check_invariants(c, xs, out, rep, k_restraint=k)
    # the antibody-only view (rows >= Lab from the ground truth) gives the same antibody and the same report
    out2, rep2 = gpu_relax(ops, c, xs, Lp=c['Lab'], k_restraint=k)
    assert torch.equal(out2.cpu(), out[:, :c['Lab']]) and torch.equal(rep2.cpu().view(torch.int64), rep.view(torch.int64))


def test_a_structure_does_not_depend_on_its_batch(ops):
    """L = 352 synthetic workload (the LDS-resident atom table at the headline size): a structure relaxed alone, in a batch of 7 and in
    a batch of 100 gives torch.equal coordinates and report rows."""
    from abx_amd import relax
    cx, _, x, sq, _ = l352_designs()
    B, Lab = sq.shape
    mov = cx['cdr_def'] == 5
    r = relax.ViolationRelaxer({k: v.to(DEV) for k, v in cx.items()}, movable=mov, flank=2)
    assert r.M == int(mov.sum()) + 4 == 17
    full, rep = r.relax(x, sq)
    assert full.shape == (B, Lab, 14, 3) and rep.shape == (B, len(relax.RELAX_COLUMNS)) and rep.dtype == torch.float64
    h = rep.cpu()
    print('L352 B=100: evaluations', h[:, 7].min().item(), h[:, 7].max().item(), 'E in', h[:, :3].sum(1).mean().item(), 'E out', h[:, 3:7].sum(1).mean().item())
    assert bool((h[:, :3].sum(1) > 0).all()) and bool((h[:, 8] > 0).all()) and bool((h[:, 3:7].sum(1) < h[:, :3].sum(1)).all())
    assert len({float(v) for v in h[:, 0]}) > 50
    idx7 = [1, 57, 2, 3, 99, 4, 5]
    seven, rep7 = r.relax(x[idx7], sq[idx7])
    for b in ALONE:
        alone, rep1 = r.relax(x[b:b + 1], sq[b:b + 1])
        assert torch.equal(alone[0], full[b]) and torch.equal(rep1[0].view(torch.int64), rep[b].view(torch.int64)), b
    for j, b in enumerate(idx7):
        assert torch.equal(seven[j], full[b]) and torch.equal(rep7[j].view(torch.int64), rep[b].view(torch.int64)), b
    assert torch.equal(full[:, ~mov_rows(r)], x[:, ~mov_rows(r)])


def mov_rows(r):
    return r.movable[:r.Lab].bool()


@pytest.mark.parametrize('use_graph', [False, True])
def test_sampler_relaxes_the_last_record_only(gpu_model, cfg, use_graph):
    """sample_fn(relaxer=, scorer=) on the tiny workload: the three new keys sit on the last record only; atom14_results, seq and scores
    equal a run without the relaxer (same seed).  Plumbing only: with the seeded test weights a design is a heap of clashing atoms."""
    from abx_amd import metrics, relax, sampler
    model, D = gpu_model
    b, sid = tiny_batch(gpu_model)
    B = sid.shape[0]
    scorer, relaxer = metrics.DesignScorer(b), relax.ViolationRelaxer(b)
    Lab = relaxer.Lab
    dm = ((1 - b['fixed_mask'][0]) * b['atom14_gt_exists'][0, :, 0]) != 0
    assert relaxer.M == int(dm.sum()) > 0 and torch.equal(relaxer.movable.bool(), dm)
    plain = sample_tiny(gpu_model, cfg, b, sid, scorer=scorer, use_graph=use_graph)
    relaxed = sample_tiny(gpu_model, cfg, b, sid, scorer=scorer, relaxer=relaxer, use_graph=use_graph)
    assert len(plain) == len(relaxed) == 5
    new = ('atom14_relaxed', 'relax', 'scores_relaxed')
    for k, (p, q) in enumerate(zip(plain, relaxed)):
        for key in SHARED:
            assert torch.equal(p[key], q[key]), (k, key)
        assert torch.equal(p['scores'].view(torch.int64), q['scores'].view(torch.int64)), k
        assert all(key not in p for key in new) and all((key in q) == (k == 4) for key in new), k
    last = relaxed[-1]
    assert last['atom14_relaxed'].shape == last['atom14_results'].shape == (B, Lab, 14, 3)
    assert last['relax'].shape == (B, len(relax.RELAX_COLUMNS)) and last['scores_relaxed'].shape == (B, len(metrics.SCORE_COLUMNS))
    rep = last['relax'].cpu()
    print('tiny workload, relax report', rep.tolist())
    assert bool((rep[:, 3:7].sum(1) <= rep[:, :3].sum(1)).all()) and bool((rep[:, 7] >= 1).all())
    fixed = ~relaxer.movable[:Lab].bool()
    assert torch.equal(last['atom14_relaxed'][:, fixed], last['atom14_results'][:, fixed])
    again, rep2 = relaxer.relax(last['atom14_results'], last['seq'])
    assert torch.equal(again, last['atom14_relaxed']) and torch.equal(rep2.view(torch.int64), last['relax'].view(torch.int64))
    assert torch.equal(scorer.score(again, last['seq']).view(torch.int64), last['scores_relaxed'].view(torch.int64))
    design = sampler.sample_fn(b, cfg, D, model, mode='design', num_t=5, sample_ids=sid, relaxer=relaxer, use_graph=use_graph)
    assert len(design) == 1 and 'atom14_relaxed' in design[0] and 'scores_relaxed' not in design[0]


def test_design_driver_writes_relaxed_files(tmp_path, monkeypatch):
    """`abx_amd.design --relax --score` on the shipped 6ct7 complex: four *_relaxed.pdb that read back to the relaxed coordinates within
    1e-3 A, <complex>_relax.tsv with one row per sample; without --relax the output directory is what it is today."""
    from abx_amd import design, metrics, relax
    from abx_amd.io import pdb_reader
    seen = spy_on_sampler(monkeypatch, lambda batch, kw, traj: traj)
    common = pdb_args(CODES[:1]) + ['--num_samples', '4', '--num_t', '4']
    files = design.main(common + ['--relax', '--score', '--output_dir', str(tmp_path / 'relaxed')])
    last = seen[-1][-1]
    plain_files = design.main(common + ['--score', '--output_dir', str(tmp_path / 'plain')])
    rel = [f for f in files if f.endswith('_relaxed.pdb')]
    assert names(rel) == [f'6ct7-{i:03d}_H_L_S_relaxed.pdb' for i in range(4)]
    assert names(set(files) - set(rel)) == sorted(names(plain_files) + ['6ct7_H_L_S_relax.tsv'])
    assert sorted(os.listdir(tmp_path / 'relaxed')) == names(files) and sorted(os.listdir(tmp_path / 'plain')) == names(plain_files)
    assert_same_bytes(plain_files, tmp_path / 'relaxed')                  # the design files themselves do not change
    x = last['atom14_relaxed'].cpu()
    assert not torch.equal(x, last['atom14_results'].cpu())
    for i in range(4):
        chains = pdb_reader.read_pdb(os.path.join(tmp_path / 'relaxed', f'6ct7-{i:03d}_H_L_S_relaxed.pdb'))
        h, l = pdb_reader.chain_feature(chains['H']), pdb_reader.chain_feature(chains['L'])
        coords = torch.from_numpy(np.concatenate([h['coords'], l['coords']]))
        m = torch.from_numpy(np.concatenate([h['coord_mask'], l['coord_mask']]))
        assert coords.shape == x[i].shape and int(m.sum()) > 1000
        err = float(((coords - x[i]).abs() * m[..., None]).max())
        print('sample', i, 'read-back error', err)
        assert err <= 1e-3
    lines = table_lines(tmp_path / 'relaxed', CODES[0], 'relax')
    assert lines[0] == ['sample'] + list(relax.RELAX_COLUMNS) + list(metrics.SCORE_COLUMNS) and len(lines) == 5
    rep, sc = last['relax'].cpu().tolist(), last['scores_relaxed'].cpu().tolist()
    for i, r in enumerate(lines[1:]):
        assert r[0] == str(i) and r[1:] == relax.format_report(rep[i]) + metrics.format_scores(sc[i]), (i, r)
    # without --score: the report columns alone
    files = design.main(common + ['--relax', '--relax_iters', '20', '--relax_flank', '1', '--relax_restraint', '0.05', '--output_dir', str(tmp_path / 'r2')])
    lines = table_lines(tmp_path / 'r2', CODES[0], 'relax')
    assert lines[0] == ['sample'] + list(relax.RELAX_COLUMNS) and len(lines) == 5 and all(int(r[8]) <= 20 for r in lines[1:])
    assert len([f for f in files if f.endswith('_relaxed.pdb')]) == 4
