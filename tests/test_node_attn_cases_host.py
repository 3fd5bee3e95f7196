"""CPU checks of tests/node_attn_cases.py: the inputs and the references do what tests/test_gpu_node_attn.py relies on, and the case list
reaches what it is meant to reach by the library's own plan (abx_seq_attn_plan).  Nothing here is tuned to a kernel."""
import math

import pytest
import torch

import node_attn_cases as NA
from oracle import abx_oracle as O

ALL = NA.SEQ_CASES + NA.IPA_CASES


def test_case_lists_are_what_the_gpu_file_documents():
    assert len(set(ALL)) == len(ALL) and len({NA.case_id(c) for c in ALL}) == len(ALL)
    assert [c.L for c in NA.SEQ_CASES if not c.sharp] == [1, 3, 4, 5, 63, 64, 65, 128, 129, 256, 257, 352, 384, 385, 512, 513, 716]
    assert all(c.B == 2 for c in NA.SEQ_CASES if c.L != 716) and [c.B for c in NA.SEQ_CASES if c.L == 716] == [1]
    assert sum(c.sharp for c in NA.SEQ_CASES) == 1 and sum(c.sharp for c in NA.IPA_CASES) == 2
    plain = [c for c in NA.IPA_CASES if not c.sharp and all(m == 'random15' for m in c.masks)]
    assert sorted(c.L for c in plain if c.B == 2) == [1, 11, 12, 13, 16, 17, 24, 25, 31, 63, 64, 65, 96, 128, 192, 224, 225]
    assert sorted(c.B for c in plain if c.L == 13) == [1, 2, 7, 8, 9, 16, 17]
    assert NA.Case('ipa', 65, 13, ('random15',) * 13, False) in plain and NA.Case('ipa', 800, 1, ('random15',), False) in plain
    assert sorted(c.L for c in NA.IPA_CASES if c.sharp) == [65, 225]
    assert {c.masks[1] for c in NA.IPA_CASES if c.B == 2} == {'random15', 'zero', 'single'}


def test_ipa_weights_are_the_params_fixture(params):
    p = NA.ipa_params()
    assert len(p) == 11 and not any('final_proj' in k for k in p)
    for k, v in p.items():
        assert v.dtype == torch.float32 and torch.equal(v, params[k]), k
    sharp = NA.ipa_params(True)
    scaled = {'proj_q_scalar': 4.0, 'proj_q_point_local': 2.0, 'proj_kv_point_local': 2.0}
    for k in p:
        f = scaled.get(k[len(NA.PRE):].rsplit('.', 1)[0], 1.0)
        assert torch.equal(sharp[k], p[k] * f), k


@pytest.mark.parametrize('L,B,masks', [(13, 3, ('random15', 'zero', 'single')), (37, 2, ('random15', 'random15'))])
def test_ipa_restatement_equals_the_oracle(params, cfg, L, B, masks):
    """ipa_core in float64 - in row chunks smaller than L and in one piece - equals oracle.ipa_attention with an identity final_proj (the
    trick of test_ipa_core) to 1e-12."""
    c = NA.Case('ipa', L, B, masks, False)
    x = NA.inputs(c)
    p = {k: v.double() for k, v in params.items() if k.startswith(NA.PRE)}
    p[NA.PRE + 'final_proj.weight'] = torch.eye(NA.NFEAT, dtype=torch.float64)
    p[NA.PRE + 'final_proj.bias'] = torch.zeros(NA.NFEAT, dtype=torch.float64)
    d = lambda t: t.double()
    want = O.ipa_attention(p, d(x['s']), d(x['z']), d(x['mask']), d(x['rots']), d(x['trans']), cfg.model.heads.diffusion_module.IPA)
    assert tuple(want.shape) == (B, L, NA.NFEAT)
    for rows in (5, 128):
        got = NA.ipa_core(p, d(x['s']), d(x['z']), d(x['mask']), d(x['rots']), d(x['trans']), rows=rows)
        assert float((got - want).abs().max()) <= 1e-12, rows
    assert float((NA.reference(c) - want).abs().max()) <= 1e-12


def test_seq_restatement_equals_the_oracles_attention_part(params):
    """oracle.seq_attention on (seq, pair, mask) equals proj_out of seq_attn_core on the q | k | v rows, bias and gate that it projects."""
    B, L, pre = 2, 21, O.P_BLK + 'seq_attn.'
    gen = torch.Generator().manual_seed(5)
    p = {k: v.double() for k, v in params.items() if k.startswith(pre)}
    seq = torch.randn(B, L, 544, generator=gen).double()
    pair = torch.randn(B, L, L, 192, generator=gen).double()
    mask = torch.stack([NA.mask_row('random20', L, gen), NA.mask_row('zero', L, gen)]).double()
    x = O.lnorm(p, pre + 'seq_norm', seq)
    bias = O.lin(p, pre + 'proj_pair', O.lnorm(p, pre + 'pair_norm', pair), bias=False).permute(0, 3, 1, 2)
    qkv = O.lin(p, pre + 'attn.proj_in', x, bias=False).reshape(B, L, NA.H_SEQ, 3 * NA.D_SEQ)
    o = NA.seq_attn_core(qkv, bias, O.lin(p, pre + 'attn.gate', x), mask)
    want = O.seq_attention(p, seq, pair, mask)
    assert float((O.lin(p, pre + 'attn.proj_out', o) - want).abs().max()) <= 1e-12 and float(want.abs().max()) > 0.1


@pytest.mark.parametrize('c', ALL, ids=NA.case_id)
def test_baseline_error_is_finite_and_not_zero(c):
    """The float32 evaluation of the reference differs from float64 in every group of every case: the unit of the GPU bound exists.  The one
    exception is arithmetic, not chance: at L = 1 every softmax weight is exactly 1, so the IPA pair group is z itself in any precision -
    there the unit is 0 and the GPU bound asks for the exact value."""
    ref = NA.reference(c)
    assert ref.dtype == torch.float64 and tuple(ref.shape) == (c.B, c.L, 544 if c.family == 'seq' else NA.NFEAT) and bool(torch.isfinite(ref).all())
    e32 = NA.baseline_err(c)
    assert set(e32) == {n for n, _ in NA.groups(c)}
    for name, (e_max, e_mean) in e32.items():
        print(f'{NA.case_id(c)} {name}: fp32 baseline err max {e_max:.3e} mean {e_mean:.3e}')
        assert math.isfinite(e_max) and math.isfinite(e_mean)
        if c.family == 'ipa' and c.L == 1 and name == 'pair':
            assert e_max == 0.0
        else:
            assert 0 < e_mean <= e_max < 1e-3, name


@pytest.mark.parametrize('c', [c for c in ALL if 'zero' in c.masks], ids=NA.case_id)
def test_fully_masked_sample_is_the_uniform_average(c):
    """Every key masked: the reference replaces every logit by finfo.min and the softmax is uniform over all L keys."""
    ref = NA.reference(c)
    for b in [b for b, m in enumerate(c.masks) if m == 'zero']:
        assert float(NA.inputs(c)['mask'][b].abs().sum()) == 0
        for name, want in NA.uniform_average(c, b).items():
            sl = dict(NA.groups(c))[name]
            assert float((ref[b][:, sl] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (b, name)


def test_masks_are_what_their_names_say():
    for c in ALL:
        m = NA.inputs(c)['mask'] if c.L <= 128 else None
        if m is None:
            continue
        for b, name in enumerate(c.masks):
            n = int(m[b].sum())
            assert n == {'zero': 0, 'single': 1, 'two': min(2, c.L)}.get(name, n), (NA.case_id(c), b)
            if name.startswith('random') and c.L >= 63:
                assert 0 < n < c.L


def test_seq_cases_reach_every_instantiation_and_both_sides_of_the_query_split():
    """Through the library's own plan (abx_seq_attn_plan: the dispatch of csrc/attention.hip run up to the launch), no copy of the rule."""
    from abx_amd import ops
    reached = {}
    for c in NA.SEQ_CASES:
        name, qblk = ops.seq_attn_kernel_name(c.L, with_qblk=True)
        assert (name, qblk) == NA.SEQ_PLAN[c.L], c.L
        reached.setdefault(name, set()).add(qblk < c.L)
    assert sorted(reached) == sorted(f'seq_attn2_kernel<{nk}, {nt}>' for nk, nt in ((2, 1024), (4, 1024), (6, 1024), (8, 512), (12, 256)))
    assert set().union(*reached.values()) == {False, True}
    assert reached['seq_attn2_kernel<12, 256>'] == {True} and all(v == {False} for k, v in reached.items() if not k.startswith('seq_attn2_kernel<12'))
    assert NA.SEQ_PLAN[352][0] == 'seq_attn2_kernel<6, 1024>'       # the workload's own length
