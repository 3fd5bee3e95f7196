"""CPU-only checks of the interface guidance (abx_amd.guidance.InterfaceGuidance, abx_contact_grad): the descriptor's layout, the
argument checks, the float64 twin against central differences, the conditions that keep the GPU comparison from passing vacuously, the
residue / restraint parsers on a shipped complex, and the composition of guidance terms."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import contact_cases as CC
from conftest import GOLDEN

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
HEADER = os.path.join(ROOT, 'include', 'abx_hip.h')
PDB = os.path.join(GOLDEN, 'pdb', '6ct7_H_L_S.pdb')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from abx_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_contact_args_ctypes_layout_matches_the_header():
    from abx_amd._lib import AbxContactArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(){', 'printf("size %zu\\n", sizeof(AbxContactArgs));']
    lines += [f'printf("{f} %zu\\n", offsetof(AbxContactArgs, {f}));' for f, _ in AbxContactArgs._fields_] + ['return 0;}']
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, 'l.c'), os.path.join(d, 'l')
        open(src, 'w').write('\n'.join(lines))
        subprocess.check_call(['gcc', src, '-o', exe])
        c_layout = dict(ln.split() for ln in subprocess.check_output([exe]).decode().split('\n') if ln)
    assert int(c_layout['size']) == ctypes.sizeof(AbxContactArgs)
    assert len(c_layout) == len(AbxContactArgs._fields_) + 1
    for f, _ in AbxContactArgs._fields_:
        assert int(c_layout[f]) == getattr(AbxContactArgs, f).offset, f


def test_contact_grad_argument_checks_without_gpu(lib):
    """Every check of abx_contact_grad answers before any launch: a negative code and the entry point's name in the message.  The device
    pointers are never dereferenced (0x1000 stands in); the host tables are real."""
    from abx_amd._lib import AbxContactArgs
    P = 0x1000
    hot = np.array([30, 31], np.int32)
    idx = np.array([[0, 1, 5, 1], [2, 4, 30, 0]], np.int32)
    par = np.array([[2.0, 4.0, 1.0], [0.0, 9.0, 0.5]], np.float32)
    keep = [hot, idx, par]

    def fresh():
        a = AbxContactArgs()
        for f in ('atom14', 'atom_mask', 'moved', 'target', 'frame_trans', 'energy', 'grad_atom', 'grad_trans', 'grad_rot', 'hotspots', 'restr_idx', 'restr_par'):
            setattr(a, f, P)
        a.hotspots_host, a.restr_idx_host, a.restr_par_host = hot.ctypes.data, idx.ctypes.data, par.ctypes.data
        a.w_contact, a.d0, a.d1, a.w_hot, a.d_hot, a.beta = 1.0, 4.0, 8.0, 1.0, 8.0, 1.0
        a.B, a.L, a.H, a.R = 2, 37, 2, 2
        return a

    def refused(a, word, ws=P):
        rc = lib.abx_contact_grad(ctypes.byref(a) if a is not None else None, ws, None)
        msg = lib.abx_last_error_string().decode()
        assert rc < 0 and 'abx_contact_grad' in msg and word in msg, (rc, msg, word)

    refused(None, 'null')
    refused(fresh(), 'null operand', ws=None)
    for f in ('atom14', 'atom_mask', 'moved', 'target', 'frame_trans', 'energy', 'grad_atom', 'grad_trans', 'grad_rot'):
        a = fresh(); setattr(a, f, None); refused(a, 'null operand')
    for B, L in ((0, 37), (65536, 37), (2, 1), (2, 1 << 22)):
        a = fresh(); a.B, a.L = B, L; refused(a, 'bad sizes')
    for d0, d1 in ((-1.0, 8.0), (8.0, 8.0), (9.0, 8.0), (float('nan'), 8.0)):
        a = fresh(); a.d0, a.d1 = d0, d1; refused(a, 'd0 < d1')
    for beta in (0.0, -1.0, float('nan')):
        a = fresh(); a.beta = beta; refused(a, 'beta')
    a = fresh(); a.H = 65; refused(a, '64 hotspots')
    a = fresh(); a.R = 257; refused(a, '256 restraints')
    a = fresh(); a.hotspots_host = None; refused(a, 'hotspot table')
    a = fresh(); a.restr_par = None; refused(a, 'restraint table')
    hot[1] = 37
    refused(fresh(), 'hotspot row')
    hot[1] = 31
    for (r, c, v), word in (((0, 0, -1), 'restraint row'), ((1, 2, 37), 'restraint row'), ((0, 1, 14), 'restraint slot'), ((1, 3, -1), 'restraint slot')):
        old = idx[r, c]; idx[r, c] = v
        refused(fresh(), word)
        idx[r, c] = old
    idx[0] = [3, 1, 3, 1]
    refused(fresh(), 'one atom twice')
    idx[0] = [0, 1, 5, 1]
    par[1, 0] = 9.5
    refused(fresh(), 'lo <= hi')
    par[1, 0] = 0.0
    assert lib.abx_contact_grad_workspace_bytes(2, 37, 2) == 4 * (2 * 2 * 4 + 2 * 3)
    del keep


def _hinge_distance(c, b, frozen):
    """The smallest distance of any hinge variable of sample b from its hinge - pair distances from d0 and d1, m_h - d_hot and the restraint
    violations from 0 and 1 - over the variables that a displacement can change (pairs of two frozen atoms cannot)."""
    info, kw = c['info'], CC.KW
    ex, mv, tg = c['exists'][b], c['moved'][b], c['target']
    ids = torch.arange(c['L'] * 14).reshape(c['L'], 14)
    a_id = ids[ex & mv[:, None]]
    t_id = ids[ex & (tg & ~mv)[:, None]]
    fz = torch.zeros(c['L'] * 14, dtype=torch.bool)
    for (r, s) in frozen:
        fz[r * 14 + s] = True
    free = ~(fz[a_id][:, None] & fz[t_id][None]).reshape(-1)
    d = info['pair_d'][b][free]
    gaps = [(d - kw['d0']).abs().min(), (d - kw['d1']).abs().min()]
    m = info['m_h'][b]
    m = m[~torch.isnan(m)] - kw['d_hot']
    rd, par = info['restr_d'][b], c['restraints'][1].double()
    ok = ~torch.isnan(rd)
    for v in (m, (rd - par[:, 1])[ok], (par[:, 0] - rd)[ok]):
        if len(v):
            gaps += [v.abs().min(), (v - 1).abs().min()]
    return float(torch.stack(gaps).min())


def test_twin_gradient_equals_central_differences():
    """contact_energy_host's autograd gradient against central differences in float64, per term and sample, along three random directions.
    The step keeps every hinge variable on its side of its hinge (asserted: an atom moves by at most h, a distance by at most 2 h), except
    the two pairs set exactly to d0 / d1, whose four atoms stay where they are."""
    c = CC.small_case()
    h = 1e-5
    frozen = [a for pair in CC.EXACT.values() for a in pair]
    for b in (0, 1):
        assert _hinge_distance(c, b, frozen if b == 0 else []) > 2 * h
    g = torch.Generator().manual_seed(5)
    x0 = c['x'].double()
    for trial in range(3):
        dirn = torch.randn(x0.shape, generator=g, dtype=torch.float64)
        dirn = dirn / dirn.norm(dim=-1, keepdim=True).clamp(min=1.0)             # every atom moves by at most h
        for (r, s) in frozen:
            dirn[0, r, s] = 0
        e_p, e_m = CC.twin(c, x0 + h * dirn), CC.twin(c, x0 - h * dirn)
        fd = (e_p - e_m) / (2 * h)
        for term in range(3):
            xd = x0.clone().requires_grad_(True)
            e = CC.twin(c, xd)
            for b in (0, 1):
                (grad,) = torch.autograd.grad(e[b, term], xd, retain_graph=True)
                an = float((grad * dirn).sum())
                err = abs(an - float(fd[b, term])) / abs(an)
                print(f'trial {trial} term {term} sample {b}: analytic {an:.9e} differences {float(fd[b, term]):.9e} rel err {err:.2e}')
                assert abs(an) > 1e-3 and err <= 1e-6, (trial, term, b, an, float(fd[b, term]))
        assert float(fd[2].abs().max()) == 0.0


def test_small_case_exercises_every_branch():
    """What the GPU comparison on the small case relies on."""
    c = CC.small_case()
    info, kw = c['info'], CC.KW
    assert (c['B'], c['L'], c['Lab']) == (3, 37, 23)
    assert [torch.nonzero(m)[:, 0].tolist() for m in c['moved']] == [[0, 9, 10, 11, 22], [4, 5, 6, 17, 18, 30], []]
    d = info['pair_d'][0]
    assert int(((d > kw['d0']) & (d < kw['d1'])).sum()) >= 200 and int((d <= kw['d0']).sum()) >= 20 and int((d >= kw['d1']).sum()) >= 20
    x = c['x'].double()
    for key, ((ri, si), (rj, sj)) in CC.EXACT.items():                      # set exactly: the separation is the hinge's value in float32 too
        assert c['moved'][0, ri] and c['target'][rj] and c['exists'][0, ri, si] and c['exists'][0, rj, sj]
        assert float((x[0, ri, si] - x[0, rj, sj]).norm()) == kw[key]
        assert int(((d - kw[key]).abs() < 1e-9).sum()) >= 1
    # missing slots on both sides, a glycine hotspot, a moved row without CB
    assert not c['exists'][0][c['moved'][0]].all() and not c['exists'][0][c['target']].all()
    assert 27 in c['hotspots'] and not c['exists'][0, 27, 4] and c['exists'][0, 27, 1]
    assert c['moved'][0, 10] and not c['exists'][0, 10, 4] and c['moved'][1, 17] and not c['exists'][1, 17, 4]
    m = info['m_h']
    assert bool((m[0] < kw['d_hot']).any()) and bool((m[0] > kw['d_hot'] + 1).any()) and bool(((m[0] > kw['d_hot']) & (m[0] < kw['d_hot'] + 1)).any())
    assert torch.isnan(m[1, c['hotspots'].index(30)]) and c['moved'][1, 30]      # a hotspot that is moved takes no part
    assert torch.isnan(m[2]).all()
    idx, par = c['restraints'][0], c['restraints'][1].double()
    for b in (0, 1):
        rd = info['restr_d'][b]
        ok = ~torch.isnan(rd)
        v = torch.maximum(rd - par[:, 1], par[:, 0] - rd)[ok]
        ends = c['moved'][b][idx[:, 0].long()].int() + c['moved'][b][idx[:, 2].long()].int()
        assert bool(((v > 0) & (v < 1)).any()) and bool((v > 1).any()), v                     # both Huber branches
        assert bool(((v <= 0) & (ends[ok] > 0)).any())                                          # the flat bottom with a moving end
        viol = torch.nan_to_num(torch.maximum(rd - par[:, 1], par[:, 0] - rd)) > 0
        assert bool(((ends == 1) & ok & viol).any())                                            # one fixed end
        if b == 0:
            assert bool((rd - par[:, 1] > 0)[ok].any()) and bool((par[:, 0] - rd > 0)[ok].any())      # too long and too short
        assert bool(((ends == 2) & ok & viol).any())                                            # both ends moved
        assert bool((~ok).any())                                                                # a missing atom
    e = c['energy']
    assert bool((e[:2].abs() > 1e-2).all()) and float(e[2].abs().max()) == 0.0, e
    assert float(c['grad'][~c['moved']].abs().max()) == 0.0 and float(c['grad'][2].abs().max()) == 0.0
    # every term alone leaves the other two at zero
    for k, kw1 in enumerate((dict(w_hot=0.0, no_restraints=True), dict(w_contact=0.0, no_restraints=True), dict(w_contact=0.0, w_hot=0.0))):
        cc = dict(c, restraints=None) if kw1.pop('no_restraints', False) else c
        e1 = CC.twin(cc, **kw1)
        assert bool((e1[:2, k] != 0).all()) and float(e1[:, [j for j in range(3) if j != k]].abs().max()) == 0.0
        assert torch.allclose(e1[:, k], e[:, k], rtol=1e-12, atol=0)


def _one():
    from abx_amd.data.antibody import load_complex
    cb = load_complex(PDB, seed=0)
    return {k: v for k, v in cb.items() if torch.is_tensor(v)}


def test_parsers_on_a_shipped_complex(tmp_path):
    from abx_amd import guidance as G
    from abx_amd import residue_constants as rc
    one, chains = _one(), ['H', 'L', 'S']
    L, Lab = one['seq'].shape[1], one['anchor_flag'].shape[1]
    assert (L, Lab) == (231, 221)
    rows = G.parse_residues(['H:98', 'L:515', 'S:0', 'S:9'], one, chains)
    assert rows[0] == 98 and rows[2:] == [221, 230] and 113 <= rows[1] < Lab
    assert int(one['chain_id'][0, rows[1]]) == 1 and int(one['residx'][0, rows[1]]) == 515
    assert G.parse_residues('H:98, S:9', one, chains) == [98, 230]
    for bad in ('S:50', 'H:500', 'X:3', 'S9'):                            # not in the featurised complex: refused by name
        with pytest.raises(SystemExit, match=bad):
            G.parse_residues(['H:98', bad], one, chains)
    res3 = lambda r: rc.restype_1to3[rc.restypes[int(one['seq'][0, r])]]
    names = rc.restype_name_to_atom14_names[res3(230)]
    last = [n for n in names if n][-1]
    f = tmp_path / 'restraints.txt'
    f.write_text(f'# comment\nH:98 CA S:9 {last} 3.0 6.5\n\nH:99 N S:0 CA 0 8 2.5   # weight\n')
    idx, par = G.parse_restraints(str(f), one, chains)
    assert idx.dtype == torch.int32 and idx.tolist() == [[98, 1, 230, list(names).index(last)], [99, 0, 221, 1]]
    assert par.tolist() == [[3.0, 6.5, 1.0], [0.0, 8.0, 2.5]]
    f.write_text('H:98 CA S:9 QX 3.0 6.5\n')
    with pytest.raises(SystemExit, match='QX'):                           # an atom the residue type lacks
        G.parse_restraints(str(f), one, chains)
    f.write_text('H:98 CA S:77 CA 3.0 6.5\n')
    with pytest.raises(SystemExit, match='S:77'):
        G.parse_restraints(str(f), one, chains)
    f.write_text('H:98 CA S:9 CA 7.0 6.5\n')
    with pytest.raises(SystemExit, match='lo'):
        G.parse_restraints(str(f), one, chains)


def test_epitope_hotspots_of_a_shipped_complex():
    """'epitope' on 6ct7 with the H3 window the features diffuse (rows 98..100): the antigen rows the wild-type loop touches; tables on the
    constructor's device, here the host."""
    from abx_amd import guidance as G
    one = _one()
    L, Lab = one['seq'].shape[1], one['anchor_flag'].shape[1]
    fixed = torch.ones(1, L, dtype=torch.int32)
    fixed[0, 98:101] = 0
    batch = dict(one, fixed_mask=fixed)
    ig = G.InterfaceGuidance(batch, w_contact=1.0, hotspots='epitope')
    assert 0 < len(ig.hotspots) <= 64 and all(Lab <= h < L for h in ig.hotspots) and ig.hotspots == sorted(ig.hotspots)
    assert ig.tables.H == len(ig.hotspots) and ig.tables.hot_host.tolist() == ig.hotspots and ig.tables.R == 0
    assert ig.target.tolist() == [int(r >= Lab) for r in range(L)]
    # by hand: a ground-truth heavy atom within d0 of one of the moved rows
    x, ex = one['atom14_gt_positions'][0].double(), one['atom14_gt_exists'][0].bool()
    a = x[98:101][ex[98:101]]
    want = [r for r in range(Lab, L) if ex[r].any() and float(torch.cdist(x[r][ex[r]], a).min()) <= 4.0]
    assert ig.hotspots == want
    # more than the limit: the nearest ones
    wide = G.epitope_rows(x, ex, ~fixed[0].bool(), torch.arange(L) >= Lab, d0=30.0, limit=4)
    assert len(wide) == 4 and set(want) <= set(wide)
    with pytest.raises(ValueError):
        G.InterfaceGuidance(batch, hotspots='paratope')


def test_sum_applies_its_terms_in_turn():
    from abx_amd.guidance import Sum
    calls = []

    class Term:
        def __init__(self, k):
            self.k = k

        def __call__(self, batch, out, rot, trans, dm):
            calls.append((self.k, batch, out, dm))
            return rot * self.k + 1, trans - self.k * rot

    a, b = Term(2.0), Term(3.0)
    rot, trans, dm = torch.randn(2, 5, 3), torch.randn(2, 5, 3), torch.ones(2, 5)
    got = Sum(a, None, b)('batch', 'out', rot, trans, dm)
    want = b('batch', 'out', *a('batch', 'out', rot, trans, dm), dm)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert [c[0] for c in calls] == [2.0, 3.0, 2.0, 3.0] and all(c[1:3] == ('batch', 'out') and c[3] is dm for c in calls)
    r0, t0 = Sum()('batch', 'out', rot, trans, dm)
    assert r0 is rot and t0 is trans
