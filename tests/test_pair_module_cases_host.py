"""CPU checks of tests/pair_module_cases.py: the inputs and the reference do what tests/test_gpu_pair_modules.py relies on.  Nothing here is
tuned to a kernel: the conditions are properties of the seeded inputs and of the float64 / float32 host evaluations alone."""
import pytest
import torch

import pair_module_cases as PM

# the distinct (module, L, B, sharp) inputs of the case table: the routes of a module share inputs and reference
INPUTS = sorted({(c.module, c.L, c.B, c.sharp) for c in PM.CASES})
SENS_L, SENS_B = 37, 4          # the sensitivity checks: samples interior, tail, alternate, zero


def _case(module, L, B, sharp=False):
    return PM.inputs(PM.Case(module, '', L, B, sharp))


def test_weights_are_the_params_fixture(params):
    p = PM.block_params()
    assert len(p) == 82 and all(k.startswith(PM.P_BLK) for k in p)
    for k, v in p.items():
        assert v.dtype == torch.float32 and torch.equal(v, params[k]), k
    for m in PM.TRI_MUL:
        for n in ('norm', 'final_norm'):          # gamma is not 1 and beta is not 0: a dropped term of a fold shows
            assert float((p[PM.P_BLK + m + f'.{n}.weight'] - 1).abs().max()) > 0.1 and float(p[PM.P_BLK + m + f'.{n}.bias'].abs().max()) > 0.1
    sharp = PM.block_params(True)
    for k in p:
        if k.endswith('attn.proj_q.weight') and 'triangle_attention' in k:
            assert torch.equal(sharp[k], p[k] * 4)
        else:
            assert torch.equal(sharp[k], p[k]), k


@pytest.mark.parametrize('module,L,B,sharp', INPUTS)
def test_baseline_range_and_update_size(module, L, B, sharp):
    """The float32 evaluation of the reference sits a little under 1e-6 of the update from float64 - the unit of the GPU bound - and the
    update is not negligible beside z."""
    c = _case(module, L, B, sharp)
    ref = PM.reference(c)
    assert ref.dtype == torch.float64 and tuple(ref.shape) == (B, L, L, PM.C) and bool(torch.isfinite(ref).all())
    assert c['z'].dtype == torch.float32 and c['mask'].dtype == torch.float32
    e_max, e_mean = PM.baseline_err(c)
    u = ref - c['z'].double()
    u_max, u_rms = float(u.abs().max()), float(u.square().mean().sqrt())
    print(f'{module} L={L} B={B} sharp={sharp}: fp32 baseline err max {e_max:.3e} mean {e_mean:.3e}; update max {u_max:.3f} rms {u_rms:.3f}')
    assert 0 < e_max < 2e-6 and 0 < e_mean < e_max
    assert u_max > 1 and u_rms > 0.1


@pytest.mark.parametrize('module', PM.TRI_MUL + PM.TRI_ATTN)
def test_restatement_equals_the_oracle(module):
    c = _case(module, SENS_L, SENS_B)
    u = PM.reference(c) - c['z'].double()
    mine = PM.tri_mul_restated(c) if module in PM.TRI_MUL else PM.tri_attn_restated(c)
    assert float((mine - u).abs().max()) < 1e-11 * float(u.abs().max())


def _moves(c, right, wrong):
    """Per sample: max |wrong - right| / max |update| of the case."""
    return ((wrong - right).abs().flatten(1).max(dim=1).values / right.abs().max()).tolist()


MISTAKES = [(PM.TRI_MUL[0], 'exchange_einsum', None), (PM.TRI_MUL[1], 'exchange_einsum', None),
            (PM.TRI_MUL[0], 'mask_left_only', ('interior', 'tail')), (PM.TRI_MUL[1], 'mask_left_only', ('interior', 'tail')),
            (PM.TRI_ATTN[0], 'exchange_orientation', None), (PM.TRI_ATTN[1], 'exchange_orientation', None),
            (PM.TRI_ATTN[0], 'ignore_key_mask', ('interior', 'tail', 'alternate')), (PM.TRI_ATTN[1], 'ignore_key_mask', ('interior', 'tail', 'alternate')),
            (PM.TRI_ATTN[0], 'additive_mask', ('zero',)), (PM.TRI_ATTN[1], 'additive_mask', ('zero',)),
            (PM.TRI_ATTN[1], 'bias_not_transposed', None)]


@pytest.mark.parametrize('module,mistake,needs', MISTAKES)
def test_one_mistake_shows(module, mistake, needs):
    """A float64 restatement with one deliberate mistake differs from the correct one by more than 0.1 of max |update| on a sample that can
    show it: the error measure and the inputs would not let such a mistake through at a bound of a few 1e-6."""
    c = _case(module, SENS_L, SENS_B)
    assert c['patterns'] == ['interior', 'tail', 'alternate', 'zero']
    f = PM.tri_mul_restated if module in PM.TRI_MUL else PM.tri_attn_restated
    d = _moves(c, f(c), f(c, mistake))
    print(f'{module} {mistake}: ' + ', '.join(f'{pt} {x:.3f}' for pt, x in zip(c['patterns'], d)))
    can = [x for pt, x in zip(c['patterns'], d) if needs is None or pt in needs]
    assert max(can) > 0.1
    if mistake == 'additive_mask':          # a lowered logit and a replaced one differ on the all-masked sample ALONE
        assert all(x < 1e-12 for pt, x in zip(c['patterns'], d) if pt != 'zero')


@pytest.mark.parametrize('module,L,B,sharp', INPUTS)
def test_mask_patterns(module, L, B, sharp):
    c = _case(module, L, B, sharp)
    pat, m = c['patterns'], c['mask']
    assert pat == PM.sample_patterns(B) and len(pat) == B and tuple(m.shape) == (B, L)
    assert set(m.unique().tolist()) <= {0.0, 1.0}
    want = set(PM.CYCLE[:min(B, 4)]) if B < 4 else (set(PM.CYCLE[:min(B - 1, 4)]) | {'zero'})
    assert set(pat) == want
    for b, pt in enumerate(pat):
        r = m[b]
        if pt == 'ones':
            assert bool((r == 1).all())
        elif pt == 'zero':
            assert bool((r == 0).all()) and b == B - 1
        elif pt == 'tail':
            assert bool((r[:L - 5] == 1).all()) and bool((r[L - 5:] == 0).all())
        elif pt == 'alternate':
            assert bool((r[0::2] == 1).all()) and bool((r[1::2] == 0).all())
        else:
            assert r[0] == 0 and r[L - 1] == 1 and 0.05 * L < float((r == 0).sum()) < 0.3 * L


def test_shapes_reach_the_branches():
    """The residues of L and the launch sizes that csrc/blocks.hip and the kernels behind it branch on."""
    ceil4 = lambda L: (L + 3) // 4 * 4
    mul = sorted({(c.L, c.B) for c in PM.CASES if c.module in PM.TRI_MUL})
    assert mul == [(64, 8), (65, 8), (70, 7), (97, 4), (97, 7)]
    assert ceil4(64) == 64 and 64 % 16 == 0                                         # no padding, no pad k-tile
    assert 65 % 4 == 1 and ceil4(65) == 68 and 68 % 16 != 0 and 65 % 8 != 0
    assert ceil4(70) == 72 and ceil4(97) == 100
    blocks = lambda L, B: B * ((L * ceil4(L) + 63) // 64)                           # 64-row blocks of the tail
    assert blocks(97, 4) < 1024 <= blocks(97, 7)
    for m in PM.TRI_MUL + PM.TRI_ATTN:
        assert {c.route for c in PM.CASES if c.module == m} == ({'split'} if m in PM.TRI_MUL else {'rowfused', 'split', 'exact_gemm', 'exact'})
    for c in PM.CASES:
        if c.route in ('split', 'rowfused'):                                        # include/abx_hip.h: what exact = 0 serves
            assert c.L >= 64 and c.B * c.L * c.L >= 32768, c
        elif c.module != PM.TRANSITION:
            assert c.L < 64, c
        assert not c.sharp or (c.module in PM.TRI_ATTN and c.route == 'rowfused')
    assert 65 * 65 * 8 == 264 * 128 + 8                                             # the fused transition's ragged last tile
    assert {(c.L, c.B) for c in PM.CASES if c.route == 'rowfused'} == {(64, 8), (65, 8), (97, 4), (200, 1)}
    assert len({PM.case_id(c) for c in PM.CASES}) == len(PM.CASES)
