"""The distogram head on the host (no GPU): the float64 twin `abx_amd.confidence.distogram_host` against the reference's own
DistogramHead / MetricDictHead outputs (tests/golden/distogram_head.npz, made by tests/golden/make_golden_distogram.py), the twin's
properties, and the wiring of the feature (module, driver flags, C ABI argument checks)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_npz
from distogram_cases import (LIP_PC, contact_precision, logit_bound, make_case, shape_case, twin_of, variant_case)


@pytest.fixture(scope='module')
def golden():
    return load_npz('distogram_head.npz')


@pytest.fixture(scope='module')
def golden_twin(golden):
    from abx_amd.confidence import distogram_host
    g = golden
    L = g['pair'].shape[1]
    return distogram_host(g['pair'], g['weight'], g['bias'], g['breaks'], g['positions'], np.ones(L, np.uint8), g['mask'], float(g['cutoff']))


def test_twin_logits_match_the_reference_head(golden, golden_twin):
    """|logits_twin - logits_ref| <= (K + 2) 2^-24 (0.5 sum_k (|z_ijk| + |z_jik|) |W_kn| + |b_n|) for every element: the bound of an
    fp32 dot product of length K = 192 in any summation order (not a tuned tolerance)."""
    g = golden
    assert g['pair'].shape == (2, 11, 11, 192) and g['logits'].shape == (2, 11, 11, 64) and g['breaks'].shape == (63,)
    z = np.abs(g['pair'].astype(np.float64))
    scale = 0.5 * (z + z.transpose(0, 2, 1, 3)) @ np.abs(g['weight'].astype(np.float64)).T + np.abs(g['bias'].astype(np.float64))
    err = np.abs(golden_twin['logits'] - g['logits'].astype(np.float64))
    bound = logit_bound(scale)
    print('max |twin - reference|', err.max(), 'largest share of the bound', (err / bound).max())
    assert (err <= bound).all()
    # the twin's own scale (of the symmetrised operand) is never larger: its bound is the tighter one the device test uses
    assert (golden_twin['bound_scale'] <= scale * (1 + 1e-12)).all()
    from abx_amd.confidence import distogram_breaks
    assert np.array_equal(distogram_breaks()[0].numpy(), g['breaks'])


def test_twin_p_contact_matches_the_metric_head(golden, golden_twin):
    """pred = sum softmax(logits)[..., :t+1], t = #{breaks <= 8} (head.py:99-102): within 2 delta of the stored tensor (a softmax sum is
    2-Lipschitz in the sup-norm of the logits; delta = the pair's largest logit bound), and the reference's contact_precision triples
    are reproduced from the twin's pred."""
    g = golden
    assert int(g['t']) == int((g['breaks'] <= np.float32(g['cutoff'])).sum()) == 19
    z = np.abs(g['pair'].astype(np.float64))
    scale = 0.5 * (z + z.transpose(0, 2, 1, 3)) @ np.abs(g['weight'].astype(np.float64)).T + np.abs(g['bias'].astype(np.float64))
    delta = logit_bound(scale).max(-1)
    err = np.abs(golden_twin['p_contact'] - g['pred'].astype(np.float64))
    print('max |p_contact - pred|', err.max(), 'largest share of the bound', (err / (LIP_PC * delta)).max())
    assert (err <= LIP_PC * delta).all()
    truth = np.sqrt(golden_twin['d2'].astype(np.float64))
    assert np.abs(truth - g['truth']).max() < 1e-4
    got = contact_precision(golden_twin['p_contact'], g['truth'], g['mask'], float(g['cutoff']))
    assert len(got) == len(g['triples']) == 12
    # (the reference divides in fp32: the stored precisions are float32 values)
    assert np.array_equal(np.array(got).astype(np.float32), g['triples'].astype(np.float32)), (got, g['triples'])
    assert g['triples'][:, 3].max() > 0                          # (the fixture holds correct contacts: the triples are not all zero)


def test_twin_planes_symmetric_and_batch_order_independent():
    """zs[i][j] and zs[j][i] hold equal bits, so every per-pair value is symmetric; a design's row does not depend on its batch mates
    (to 1e-12: the float64 matrix product of the host may round a row differently at another position of the operand)."""
    c = shape_case(65, 3)
    t = twin_of(c)
    for k in ('p_contact', 'exp_dist', 'entropy'):
        assert np.allclose(t[k], t[k].transpose(0, 2, 1), rtol=1e-12, atol=1e-12), k
    assert np.array_equal(t['bin_real'], t['bin_real'].transpose(0, 2, 1))
    from abx_amd.confidence import distogram_host
    perm = [2, 0, 1]
    t2 = distogram_host(c['pair'][perm], c['W'], c['b'], c['breaks'], c['pb'][perm], c['classes'], c['valid'][perm], c['cutoff'])
    assert np.allclose(t2['table'], t['table'][perm], rtol=1e-12, atol=1e-12)
    assert np.allclose(t2['rows'], t['rows'][perm], rtol=1e-12, atol=1e-12)
    assert np.array_equal(t2['table'][:, [7, 9]], t['table'][perm][:, [7, 9]])
    assert np.isfinite(t['table']).all() and (t['table'][:, 9] > 0).all()


def test_twin_empty_sets_give_zero_not_nan():
    from abx_amd.confidence import CONFIDENCE_COLUMNS as COLS
    col = {c: k for k, c in enumerate(COLS)}
    t = twin_of(variant_case('empty_region'))
    assert np.isfinite(t['table']).all() and np.isfinite(t['rows']).all()
    assert (t['table'][:, 2:] == 0).all() and (t['table'][:, :2] > 0).all()
    t = twin_of(variant_case('no_antigen'))
    assert np.isfinite(t['table']).all()
    for c in ('nll_antibody_antigen', 'nll_region_antigen', 'exp_contacts_region_antigen', 'n_contacts_region_antigen', 'p_on_contacts_region_antigen'):
        assert (t['table'][:, col[c]] == 0).all(), c
    assert (t['table'][:, col['n_pairs_region']] > 0).all() and (t['rows'][:, :, 1:3] == 0).all()
    # a masked residue enters nothing: its own row is zero and no partner counts it
    c = variant_case('one_residue')
    t = twin_of(c)
    assert (t['rows'][:, 9] == 0).all() and (t['rows'][:, 68] == 0).all()
    nvalid = c['valid'].sum(1).numpy()
    assert np.array_equal(t['table'][:, col['n_pairs_region']], nvalid - 1)
    # L = 1: no pair at all
    t = twin_of(shape_case(1, 1))
    assert (t['table'] == 0).all() and (t['rows'] == 0).all()


def test_every_case_keeps_its_distances_off_the_breaks():
    """What the GPU test's equal-counts assertion rests on: no pair within 1e-4 A of a break or of the cutoff, for the seeds in use."""
    from distogram_cases import SHAPES, VARIANTS
    for L in SHAPES:
        for B in (1, 3):
            assert shape_case(L, B)['min_margin'] > 1e-4
    for v in VARIANTS:
        assert variant_case(v)['min_margin'] > 1e-4


def _toy_batch(L=6, Lab=4):
    g = torch.Generator().manual_seed(3)
    seq = torch.tensor([0, 7, 5, 7, 7, 2])                      # Gly at 1, 3 (antibody) and 4 (antigen)
    exists = torch.ones(L, 14)
    exists[5, 4] = 0                                            # an antigen residue without CB
    return dict(seq=seq[None], anchor_flag=torch.zeros(1, Lab), atom14_gt_positions=torch.randn(1, L, 14, 3, generator=g),
                atom14_gt_exists=exists[None], mask=torch.ones(1, L), fixed_mask=torch.tensor([[1., 0., 0., 1., 1., 1.]]))


def test_scorer_takes_ca_for_a_designed_gly():
    """The pseudo-beta atom follows the DESIGN's own sequence: CB (slot 4), CA (slot 1) where the design holds a Gly; antigen rows come
    from the ground truth; the region defaults to (1 - fixed_mask) * exists."""
    from abx_amd.confidence import ANTIBODY, ANTIGEN, DESIGNED, DistogramScorer
    b = _toy_batch()
    sd = {'impl.distogram.proj.weight': torch.zeros(64, 192), 'impl.distogram.proj.bias': torch.zeros(64)}
    sc = DistogramScorer(b, sd)
    assert sc.classes.tolist() == [ANTIBODY, ANTIBODY | DESIGNED, ANTIBODY | DESIGNED, ANTIBODY, ANTIGEN, ANTIGEN]
    x = torch.randn(2, 4, 14, 3)
    seq = torch.tensor([[0, 7, 5, 3], [0, 4, 7, 7]])            # design 0: Gly at 1; design 1: Gly at 2, 3 (the ground truth's 1 is not one)
    pb, valid = sc.inputs(x, seq)
    assert torch.equal(pb[0, 1], x[0, 1, 1]) and torch.equal(pb[0, 2], x[0, 2, 4]) and torch.equal(pb[0, 3], x[0, 3, 4])
    assert torch.equal(pb[1, 1], x[1, 1, 4]) and torch.equal(pb[1, 2], x[1, 2, 1]) and torch.equal(pb[1, 3], x[1, 3, 1])
    gt = b['atom14_gt_positions'][0]
    assert torch.equal(pb[0, 4], gt[4, 1]) and torch.equal(pb[1, 5], gt[5, 4])
    assert valid.tolist() == [[True] * 5 + [False]] * 2
    pbw, vw = sc.inputs(gt[None], b['seq'], wild=True)
    assert torch.equal(pbw[0, 1], gt[1, 1]) and torch.equal(pbw[0, 2], gt[2, 4]) and vw.tolist() == [[True] * 5 + [False]]
    # zero weights: a uniform distribution over the 64 bins, whatever the pair representation holds
    t = sc.host(torch.randn(2, 6, 6, 192), x, seq)
    assert np.allclose(t['entropy'], np.log(64.0)) and np.allclose(t['table'][:, 0], np.log(64.0)) and np.allclose(t['p_contact'], 20 / 64)


def test_logits_request_above_one_gib_is_refused():
    from abx_amd.confidence import DistogramScorer
    b = _toy_batch()
    sc = DistogramScorer(b, {'impl.distogram.proj.weight': torch.zeros(64, 192), 'impl.distogram.proj.bias': torch.zeros(64)})
    sc.L = 352
    with pytest.raises(ValueError, match=r'3171942400 bytes'):
        sc.logits(torch.zeros(0), range(100))


def test_module_and_driver_wiring():
    """abx_amd.confidence imports, the driver lists --confidence, the sampler takes a scorer, the columns are the documented ones."""
    import inspect
    from abx_amd import confidence, design, sampler
    assert confidence.CONFIDENCE_COLUMNS == ('nll_all', 'nll_antibody_antigen', 'nll_region', 'nll_region_antigen', 'dist_err_region',
                                             'entropy_region', 'exp_contacts_region_antigen', 'n_contacts_region_antigen',
                                             'p_on_contacts_region_antigen', 'n_pairs_region')
    text = design.build_parser().format_help()
    for flag in ('--confidence', '--confidence_cutoff', '--confidence_planes'):
        assert flag in text
    a = design.build_parser().parse_args([])
    assert a.confidence is False and a.confidence_planes is False and a.confidence_cutoff == 8.0
    assert inspect.signature(sampler.sample_fn).parameters['confidence'].default is None


def test_entry_points_reject_bad_arguments_before_any_launch():
    from abx_amd import _lib
    lib = _lib.load()
    assert _lib.DISTO_COLS == len(__import__('abx_amd.confidence', fromlist=['x']).CONFIDENCE_COLUMNS)
    assert lib.abx_distogram_scores(None, None) < 0 and b'abx_distogram_scores' in lib.abx_last_error_string()
    assert lib.abx_distogram_logits(None, None, None) < 0
    a = _lib.AbxDistogramArgs()
    assert lib.abx_distogram_scores(ctypes.byref(a), None) < 0      # sizes
    a.B, a.L = 1, 4
    assert lib.abx_distogram_scores(ctypes.byref(a), None) < 0      # null operands
    P = 0x1000
    a.z = a.W = a.bias = P
    assert lib.abx_distogram_logits(ctypes.byref(a), None, None) < 0 and b'null output' in lib.abx_last_error_string()
    a.breaks = a.sq_breaks = a.pb = a.classes = a.valid = a.table = a.rowsums = P
    a.num_breaks, a.cutoff, a.table_stride = 62, 8.0, 10
    assert lib.abx_distogram_scores(ctypes.byref(a), None) < 0 and b'num_breaks' in lib.abx_last_error_string()
    a.num_breaks, a.cutoff = 63, 0.0
    assert lib.abx_distogram_scores(ctypes.byref(a), None) < 0 and b'cutoff' in lib.abx_last_error_string()
    a.cutoff, a.table_stride = 8.0, 9
    assert lib.abx_distogram_scores(ctypes.byref(a), None) < 0 and b'table_stride' in lib.abx_last_error_string()
    a.table_stride, a.z = 10, P + 4
    assert lib.abx_distogram_scores(ctypes.byref(a), None) < 0 and b'aligned' in lib.abx_last_error_string()
