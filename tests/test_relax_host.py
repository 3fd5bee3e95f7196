"""CPU-only checks of the violation relaxation (abx_relax, abx_amd.relax): the float64 host twin on the two shipped complexes, the
restricted energy against the full violation energy of the oracle, the C layout of the descriptor, argument checks without a GPU and
the plumbing of the sampler / the design driver, and the kernel's own source (csrc/relax.hip) compiled for the host and run on CPU threads
(tests/relax_emu) against the host twin."""
import ctypes
import inspect
import os
import subprocess
import tempfile

import pytest
import torch

import host_cases as HC
import relax_cases as RC

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))

# Evaluations relax_host needs to reach E == 0 on the nine perturbed cases (measured; the prototype of the algorithm needed the same).
# The GPU test relies on the default budget of 200 evaluations with a factor 4 of margin for float32 taking another accept / reject path.
N_HOST = {('6qd7', 'h3'): (22, 27, 22), ('6ct7', 'h3'): (15, 14, 26), ('6qd7', 'all'): (26, 23, 24)}


@pytest.fixture(scope='module')
def lib():
    return HC.load_lib()


def _relax(c, x, **kw):
    from abx_amd import relax
    return relax.relax_host(x, c['mask'], c['aa'], c['chain'], c['residx'], c['mov'], **kw)


@pytest.mark.parametrize('code,sel', RC.MOVABLE_SETS)
def test_crystal_structures_are_clean_and_do_not_move(code, sel):
    """E = 0 on the crystal structure with every movable set: one evaluation, the output is the input, and all five count columns of
    the whole complex are 0 (so E = 0 after a relax means a structure with zero counts)."""
    c = RC.load_complex(code, sel)
    assert int(c['mov'].sum()) == {('6qd7', 'h3'): 14, ('6ct7', 'h3'): 4, ('6qd7', 'all'): 48}[(code, sel)]
    x, rep = _relax(c, c['x'])
    assert rep[:7].tolist() == [0.0] * 7 and rep[7] == 1 and rep[8] == 0 and rep[10] == 0
    assert torch.equal(x, c['x'])
    assert RC.counts(c['x'], c) == [0, 0, 0, 0, 0]


@pytest.mark.parametrize('code,sel', RC.MOVABLE_SETS)
def test_perturbed_loops_relax_to_zero_within_a_quarter_of_the_budget(code, sel):
    """The nine cases (three movable sets x seeds 5 / 6 / 7; 0.7 A / 0.25 rad / 0.5 rad, inputs rounded to float32): E reaches exactly 0,
    all counts become 0, fixed rows are untouched, and 4 x the evaluations used fits the default budget."""
    from abx_amd import relax
    c = RC.load_complex(code, sel)
    used = []
    for seed in RC.SEEDS:
        xp = RC.perturb(c, seed)
        before = RC.counts(xp, c)
        x, rep = _relax(c, xp)
        r = dict(zip(relax.RELAX_COLUMNS, rep.tolist()))
        print(code, sel, seed, r, before)
        assert sum(before[:3]) > 0 and r['E_bond_in'] > 0 and r['E_angle_in'] > 0
        assert r['E_clash'] == 0 and r['E_bond'] == 0 and r['E_angle'] == 0 and r['E_restraint'] == 0
        assert RC.counts(x, c) == [0, 0, 0, 0, 0]
        assert torch.equal(x[~c['mov']], xp[~c['mov']])
        assert 0.3 < r['max_ca_shift'] < 3.0 and r['accepted'] < r['evaluations']
        used.append(int(r['evaluations']))
    assert tuple(used) == N_HOST[(code, sel)]
    assert 4 * max(max(v) for v in N_HOST.values()) <= relax.DEFAULTS['max_iter'] == 200


def test_energy_never_increases_and_restraint_bounds_the_motion():
    """With k_restraint = 0.05: E_after <= E_before and k * sum |dCA|^2 <= E_viol(input) (monotonicity), on 6ct7 H3."""
    c = RC.load_complex('6ct7', 'h3')
    xp = RC.perturb(c, 6)
    k = 0.05
    x, rep = _relax(c, xp, k_restraint=k, max_iter=60)
    e_in, e_out = float(rep[:3].sum()), float(rep[3:7].sum())
    assert e_out <= e_in and rep[8] > 0
    shift2 = float(((x - xp)[c['mov'], 1] ** 2).sum())
    assert abs(k * shift2 - float(rep[6])) <= 1e-9 * max(1.0, float(rep[6]))
    assert k * shift2 <= e_in


@pytest.mark.parametrize('code,sel,seed', [('6ct7', 'h3', 7), ('6qd7', 'h3', 5)])
def test_restricted_energy_is_the_full_energy_minus_a_constant(code, sel, seed):
    """The terms that touch no movable residue do not change in a relax: full (oracle.violation_energy) minus restricted is the same
    number before and after, per term, to 1e-9 relative."""
    from oracle import abx_oracle as O
    from abx_amd import relax
    c = RC.load_complex(code, sel)
    xp = RC.perturb(c, seed)
    x, rep = _relax(c, xp, max_iter=8)                       # a few accepted steps: a state with non-zero energy
    assert rep[8] > 0 and float(rep[3:6].sum()) > 0
    full = lambda y: [float(e[0]) for e in O.violation_energy(y[None], c['mask'][None], c['aa'][None], c['chain'][None], residx=c['residx'][None])]
    part = lambda y: [float(e) for e in relax.restricted_energy(y, c['mask'], c['aa'], c['chain'], c['residx'], c['mov'])[:3]]
    f0, f1, p0, p1 = full(xp), full(x), part(xp), part(x)
    for k in range(3):
        assert abs(p0[k] - float(rep[k])) <= 1e-12 * max(1.0, p0[k]) and abs(p1[k] - float(rep[3 + k])) <= 1e-12 * max(1.0, p1[k])
        assert abs((f0[k] - p0[k]) - (f1[k] - p1[k])) <= 1e-9 * max(f0[k], 1.0), (k, f0, p0, f1, p1)
    assert p0[0] > p1[0] or p0[1] > p1[1]


def test_relax_args_match_c_layout():
    """sizeof / offsetof of AbxRelaxArgs as gcc lays it out, ABX_RELAX_COLS against the Python side."""
    from abx_amd import _lib, relax
    st = _lib.AbxRelaxArgs
    c_layout = HC.assert_c_layout({'AbxRelaxArgs': st}, ['ABX_RELAX_COLS'])
    assert c_layout['ABX_RELAX_COLS'] == _lib.RELAX_COLS == len(relax.RELAX_COLUMNS)


def test_relax_exports_and_argument_checks_without_gpu(lib):
    """abx_relax / abx_relax_workspace_bytes are exported; every malformed descriptor comes back negative before any launch with the
    entry's name in the message; a structure that does not fit the LDS-resident atom table is such an error."""
    from abx_amd._lib import AbxRelaxArgs
    P = 0x1000                                      # any non-null "device pointer": nothing is dereferenced
    ptrs = ('pred_atom14', 'pred_seq', 'gt_atom14', 'gt_exists', 'gt_seq', 'chain_id', 'movable', 'radius', 'chi_axis', 'rigid_group',
            'out_atom14', 'report')

    def good():
        a = AbxRelaxArgs()
        for f in ptrs:
            setattr(a, f, P)
        a.B, a.L, a.Lab, a.Lpred, a.M = 4, 40, 30, 30, 6
        a.pred_sb, a.pred_seq_sb, a.out_sb, a.report_stride = 30 * 42, 30, 30 * 42, 11
        a.overlap_tolerance, a.between_chain_factor, a.bond_tolerance_factor, a.w_clash, a.w_bond, a.w_angle = 1.5, 0.2, 12.0, 1.0, 1.0, 1.0
        a.k_restraint, a.eta0, a.rho, a.grow, a.shrink, a.max_iter = 0.0, 0.01, 2.0, 1.2, 0.5, 200
        return a

    def bad(a, word=b''):
        rc = lib.abx_relax(ctypes.byref(a) if a is not None else None, None, None)
        msg = lib.abx_last_error_string()
        assert rc < 0 and b'abx_relax' in msg and word in msg, (rc, msg)

    assert hasattr(lib, 'abx_relax') and hasattr(lib, 'abx_relax_workspace_bytes')
    assert lib.abx_relax_workspace_bytes(100, 352, 48) >= 0
    assert lib.abx_relax_lds_bytes(352, 48) == 232 * 352 + 340 * 48 + 1024 <= 160 * 1024
    bad(None)
    bad(AbxRelaxArgs())
    for field in ptrs:
        a = good()
        setattr(a, field, None)
        bad(a, b'null')
    for field, v in (('B', 0), ('B', -3), ('L', 0), ('L', 1), ('L', -1), ('M', 0), ('M', -1), ('M', 31), ('Lab', 41), ('Lab', 0), ('Lpred', 29),
                     ('Lpred', 41), ('report_stride', 10), ('out_sb', 30 * 42 - 1), ('max_iter', -1), ('eta0', 0.0), ('rho', 0.0), ('grow', 0.9),
                     ('shrink', 1.0), ('shrink', 0.0), ('k_restraint', -1.0)):
        a = good()
        setattr(a, field, v)
        bad(a)
    a = good()                                      # L = 352 with 300 movable rows: 184 688 bytes of LDS
    a.L, a.Lab, a.Lpred, a.M = 352, 320, 320, 300
    a.pred_sb = a.out_sb = 320 * 42
    assert lib.abx_relax_lds_bytes(352, 300) > 160 * 1024
    bad(a, b'LDS')


def test_driver_and_sampler_plumbing():
    """The parser accepts the new flags and --relax is off by default; sample_fn takes relaxer=None; the relax TSV format; the flank
    of the movable set follows the link rule; ViolationRelaxer takes the sampler's diffuse mask by default."""
    from abx_amd import design, relax, sampler, metrics
    a = design.build_parser().parse_args([])
    assert a.relax is False and a.relax_iters == 200 and a.relax_flank == 0 and a.relax_restraint == 0.0
    a = design.build_parser().parse_args(['--relax', '--relax_iters', '50', '--relax_flank', '2', '--relax_restraint', '0.05', '--score'])
    assert a.relax and a.relax_iters == 50 and a.relax_flank == 2 and a.relax_restraint == 0.05 and a.score
    assert inspect.signature(sampler.sample_fn).parameters['relaxer'].default is None
    # flank: grows along links only (chain break between rows 3 | 4, numbering gap between rows 6 | 7), never beyond the limit
    chain = torch.tensor([0, 0, 0, 0, 1, 1, 1, 1, 1, 1])
    residx = torch.tensor([1, 2, 3, 4, 1, 2, 3, 9, 10, 11])
    mov = torch.zeros(10, dtype=torch.bool)
    mov[3] = mov[5] = True
    assert relax.expand_movable(mov, chain, residx, 0).tolist() == mov.tolist()
    assert torch.nonzero(relax.expand_movable(mov, chain, residx, 1))[:, 0].tolist() == [2, 3, 4, 5, 6]
    assert torch.nonzero(relax.expand_movable(mov, chain, residx, 3))[:, 0].tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert torch.nonzero(relax.expand_movable(mov, chain, None, 3))[:, 0].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8]
    assert torch.nonzero(relax.expand_movable(mov, chain, residx, 3, limit=5))[:, 0].tolist() == [0, 1, 2, 3, 4]
    c = RC.load_complex('6ct7', 'h3')
    L = c['aa'].shape[0]
    batch = {'seq': c['aa'][None], 'anchor_flag': torch.zeros(1, c['Lab']), 'atom14_gt_positions': c['x'][None].float(), 'atom14_gt_exists': c['mask'][None],
             'chain_id': c['chain'][None], 'residx': c['residx'][None], 'fixed_mask': (~c['mov'])[None].float()}
    r = relax.ViolationRelaxer(batch, max_iter=50)
    assert r.M == 4 and torch.equal(r.movable.bool(), c['mov']) and r.params['max_iter'] == 50 and r.params['eta0'] == 0.01 and r.movable.shape == (L,)
    assert relax.ViolationRelaxer(batch, flank=2).M == 8
    with pytest.raises(TypeError):
        relax.ViolationRelaxer(batch, step=1.0)
    with pytest.raises(ValueError):
        relax.ViolationRelaxer(batch, movable=torch.zeros(L))
    # the TSV
    rep = [27.0, 1.5, 0.25, 0.0, 0.0, 0.0, 0.0, 22.0, 19.0, 0.0799, 1.6361]
    sc = [0.5] * 14 + [0.0, 1.0, 2.0, 3.0, 0.0]
    with tempfile.TemporaryDirectory() as d:
        head, line = open(design._write_relax(d, 'x_H_L_A', [(3, rep)], False)).read().splitlines()
        assert head.split('\t') == ['sample'] + list(relax.RELAX_COLUMNS)
        f = line.split('\t')
        assert f[0] == '3' and f[8] == '22' and f[9] == '19' and float(f[1]) == 27.0 and abs(float(f[11]) - 1.6361) < 1e-6
        head, line = open(design._write_relax(d, 'x_H_L_A', [(0, rep + sc)], True)).read().splitlines()
        assert head.split('\t') == ['sample'] + list(relax.RELAX_COLUMNS) + list(metrics.SCORE_COLUMNS)
        assert line.split('\t')[12:] == metrics.format_scores(sc) and os.path.basename(design._write_relax(d, 'x_H_L_A', [], False)) == 'x_H_L_A_relax.tsv'


@pytest.fixture(scope='module')
def emulated_kernel(tmp_path_factory):
    """csrc/relax.hip compiled with g++ against the stand-in headers of tests/relax_emu: relax_kernel on 1024 CPU threads per workgroup.
    -> relax(c, xs, **kw) with the signature of ops.relax's results, on CPU tensors."""
    import shutil
    from abx_amd import _lib, ops
    d = tmp_path_factory.mktemp('relax_emu')
    emu = os.path.join(ROOT, 'tests', 'relax_emu')
    src = open(os.path.join(ROOT, 'abx_amd', 'csrc', 'relax.hip')).read()
    decl = 'extern __shared__ __align__(16) unsigned char lds[];'
    assert src.count(decl) == 1
    open(os.path.join(d, 'relax_emu.hip'), 'w').write(src.replace(decl, 'unsigned char* lds = emu_lds;'))
    shutil.copy(os.path.join(ROOT, 'abx_amd', 'csrc', 'peptide_dev.h'), d)
    shutil.copy(os.path.join(ROOT, 'abx_amd', 'csrc', 'structure_dev.h'), d)
    shutil.copy(os.path.join(emu, 'common.h'), d)
    shutil.copy(os.path.join(emu, 'emu.cpp'), d)
    so = os.path.join(d, 'librelax_emu.so')
    subprocess.check_call(['g++', '-std=c++20', '-O1', '-ffp-contract=off', '-fPIC', '-shared', '-w', '-x', 'c++', '-I' + str(d), '-I' + emu,
                           '-I' + os.path.join(ROOT, 'include'), os.path.join(d, 'emu.cpp'), '-o', so, '-lpthread'])
    lib = ctypes.CDLL(so)
    lib.emu_relax.restype = ctypes.c_int
    lib.emu_relax.argtypes = [ctypes.POINTER(_lib.AbxRelaxArgs)]
    axis, group = ops.chi_tables('cpu')
    rad = ops.vdw_radius_table('cpu')

    def run(c, xs, max_iter=200, k_restraint=0.0):
        B, L = xs.shape[0], c['aa'].shape[0]
        t = dict(x=xs.float().contiguous(), sq=c['aa'][None].repeat(B, 1).contiguous(), gt=c['x'].float().contiguous(), gseq=c['aa'].contiguous(),
                 ex=c['mask'].to(torch.uint8).contiguous(), pm=c['mask'][None].repeat(B, 1, 1).to(torch.uint8).contiguous(), ch=c['chain'].int().contiguous(),
                 ri=c['residx'].int().contiguous(), mv=c['mov'].to(torch.uint8).contiguous(), out=torch.empty(B, L, 14, 3),
                 rep=torch.empty(B, _lib.RELAX_COLS, dtype=torch.float64), g=torch.empty(B, int(c['mov'].sum()), 10))
        a = _lib.AbxRelaxArgs()
        a.pred_atom14, a.pred_sb, a.Lpred, a.pred_seq, a.pred_seq_sb, a.pred_mask = t['x'].data_ptr(), L * 42, L, t['sq'].data_ptr(), L, t['pm'].data_ptr()
        a.gt_atom14, a.gt_exists, a.gt_seq, a.chain_id, a.residx, a.movable = (t[k].data_ptr() for k in ('gt', 'ex', 'gseq', 'ch', 'ri', 'mv'))
        a.radius, a.chi_axis, a.rigid_group = rad.data_ptr(), axis.data_ptr(), group.data_ptr()
        a.overlap_tolerance, a.between_chain_factor, a.bond_tolerance_factor, a.w_clash, a.w_bond, a.w_angle = 1.5, 0.2, 12.0, 1.0, 1.0, 1.0
        a.k_restraint, a.eta0, a.rho, a.grow, a.shrink, a.max_iter = k_restraint, 0.01, 2.0, 1.2, 0.5, max_iter
        a.out_atom14, a.out_sb, a.report, a.report_stride, a.gen_grad = t['out'].data_ptr(), L * 42, t['rep'].data_ptr(), _lib.RELAX_COLS, t['g'].data_ptr()
        a.B, a.L, a.Lab, a.M = B, L, c['Lab'], int(c['mov'].sum())
        assert lib.emu_relax(ctypes.byref(a)) == 0
        return t['out'], t['rep'], t['g']

    return run


def test_kernel_source_on_cpu_threads_matches_the_host_twin(emulated_kernel):
    """relax_kernel itself (float32, its own reductions and barriers, NaN-filled LDS) on 6ct7 H3: energies and the generalised gradient
    of the input state against relax_host at the GPU test's tolerances (2e-5 / 5e-5); a full relax reaches E == 0 with all counts 0 and
    rigid residues; a clean structure comes back bit-identical after one evaluation; fixed rows are copies."""
    from abx_amd import relax
    c = RC.load_complex('6ct7', 'h3')
    xs = torch.stack([RC.perturb(c, 6), c['x'].float().double(), RC.perturb(c, 7)])
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))
    out, rep, G = emulated_kernel(c, xs, max_iter=0)
    assert torch.equal(out, xs.float())
    for b in (0, 2):
        _, hrep, hG = relax.relax_host(xs[b], c['mask'], c['aa'], c['chain'], c['residx'], c['mov'], max_iter=0, return_grad=True)
        assert min(hrep[:3].tolist()) > 0
        for k in range(3):
            assert abs(float(rep[b, k]) - float(hrep[k])) <= 2e-5 * float(hrep[k]), (b, k, rep[b], hrep)
        assert rel(G[b, :, 0:3], hG[:, 0:3]) <= 5e-5 and rel(G[b, :, 3:6], hG[:, 3:6]) <= 5e-5 and rel(G[b, :, 6:], hG[:, 6:]) <= 5e-5
    assert float(G[1].abs().max()) == 0.0
    out, rep, _ = emulated_kernel(c, xs)
    print(rep.tolist())
    assert torch.equal(out[1], xs[1].float()) and rep[1].tolist() == [0.0] * 7 + [1.0, 0.0, float(torch.tensor(0.01)), 0.0]
    mi = torch.nonzero(c['mov'])[:, 0]
    for b in (0, 2):
        assert float(rep[b, 3:7].sum()) == 0.0 and 5 < rep[b, 7] <= 4 * max(N_HOST[('6ct7', 'h3')]) and rep[b, 8] > 0
        assert RC.counts(xs[b], c)[:3] != [0, 0, 0] and RC.counts(out[b].double(), c) == [0, 0, 0, 0, 0]
        assert torch.equal(out[b][~c['mov']], xs[b][~c['mov']].float())
        d0, d1 = torch.cdist(xs[b][mi][:, :5], xs[b][mi][:, :5]), torch.cdist(out[b][mi][:, :5].double(), out[b][mi][:, :5].double())
        assert float(((d0 - d1).abs() * (c['mask'][mi][:, :5, None] & c['mask'][mi][:, None, :5])).max()) <= 1e-3
