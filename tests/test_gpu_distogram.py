"""abx_distogram_scores / abx_distogram_logits on an MI355X (`pytest -m gpu`) against the float64 host twin
(abx_amd.confidence.distogram_host) and the reference's own head outputs (tests/golden/distogram_head.npz).

Bounds (tests/distogram_cases.py): the logits per element by the fp32 dot-product bound; everything derived from them per pair by what
that bound implies (Lipschitz constants of nll, entropy, p_contact and E[d] in the sup-norm of a pair's logits) plus MARGIN, the room
for the device's expf against float64: four times the largest excess over the logit-implied bound measured on these cases (DESIGN.md
section 4l).  The measured excess is zero - the largest observed share of the logit-implied bound is printed by every test - so MARGIN is
zero: the device has to stay inside what the logit bound alone implies.  Tables and rows are means (or sums) of per-pair values
accumulated in float64 and take the mean (sum) of the per-pair bounds.  The fp32 planes add half an ulp of their own rounding."""
import os

import numpy as np
import pytest
import torch

from analysis_gpu_cases import CODES, DEV, pdb_args, table_lines
from conftest import load_npz, tt, feat_batch_from_golden
from distogram_cases import (EPS, LIP_ENT, LIP_NLL, LIP_PC, SHAPES, VARIANTS, logit_bound, shape_case, twin_of, variant_case)

pytestmark = pytest.mark.gpu
MARGIN = 0.0            # 4 x the measured excess over the logit-implied bound (see the module docstring)


def dev_inputs(c):
    from abx_amd import ops
    g = {k: c[k].to(DEV) for k in ('pair', 'W', 'b', 'breaks', 'pb', 'classes', 'valid')}
    g['wp'] = ops.distogram_pack_weight(g['W'])
    g['sq'] = torch.square(c['breaks']).to(DEV)
    return g


def run_scores(c, planes=True):
    from abx_amd import ops
    g = dev_inputs(c)
    table, rows, pl = ops.distogram_scores(g['pair'], g['wp'], g['b'], g['breaks'], g['sq'], g['pb'], g['classes'], g['valid'],
                                           cutoff=c['cutoff'], planes=planes)
    torch.cuda.synchronize()
    return table.cpu().numpy(), rows.cpu().numpy(), (tuple(p.cpu().numpy() for p in pl) if planes else None)


def run_logits(c):
    from abx_amd import ops
    g = dev_inputs(c)
    out = ops.distogram_logits(g['pair'], g['wp'], g['b'])
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_against_twin(name, table, rows, planes, t, classes, breaks):
    """The device's table / rows / planes against the twin `t` under the bounds of the module docstring.  Prints, per quantity, the largest
    error and its largest share of the bound."""
    from abx_amd.confidence import ANTIBODY, ANTIGEN, DESIGNED, bin_centres
    cen = bin_centres(breaks)
    delta = logit_bound(t['bound_scale']).max(-1)
    b_nll, b_ent, b_pc, b_ed = LIP_NLL * delta + MARGIN, LIP_ENT * delta + MARGIN, LIP_PC * delta + MARGIN, (cen[-1] - cen[0]) * delta + MARGIN
    cls = classes.cpu().numpy().astype(np.int64)
    ab, ag, des = (((cls & m) != 0) for m in (ANTIBODY, ANTIGEN, DESIGNED))
    ok = t['ok']
    okag, reg = ok & ag[None, None, :], ok & des[None, :, None]
    regag = okag & des[None, :, None]
    within = reg & (t['bin_real'] < 63)
    con = regag & t['contact']
    report = {}

    def cmp(what, got, want, bound):
        err = np.abs(got - want)
        assert np.isfinite(got).all(), f'{name} {what}: non-finite'
        share = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
        report[what] = (float(err.max()) if err.size else 0.0, share)
        assert (err <= bound).all(), f'{name} {what}: max err {err.max():.3e}, {share:.3f} of the bound'

    def mean_b(b, sel):
        n = sel.sum((1, 2))
        return np.where(n > 0, np.where(sel, b, 0.0).sum((1, 2)) / np.maximum(n, 1), 0.0)

    tw = t['table']
    # counts: equal integers (no pair of the inputs sits within 1e-4 A of a break or the cutoff)
    assert np.array_equal(table[:, [7, 9]], tw[:, [7, 9]]), f'{name}: counts {table[:, [7, 9]]} vs {tw[:, [7, 9]]}'
    assert np.array_equal(rows[:, :, 2], t['rows'][:, :, 2]), f'{name}: per-residue contact counts'
    cmp('nll_all', table[:, 0], tw[:, 0], mean_b(b_nll, ok))
    cmp('nll_antibody_antigen', table[:, 1], tw[:, 1], mean_b(b_nll, okag & ab[None, :, None]))
    cmp('nll_region', table[:, 2], tw[:, 2], mean_b(b_nll, reg))
    cmp('nll_region_antigen', table[:, 3], tw[:, 3], mean_b(b_nll, regag))
    cmp('dist_err_region', table[:, 4], tw[:, 4], mean_b(b_ed, within))
    cmp('entropy_region', table[:, 5], tw[:, 5], mean_b(b_ent, reg))
    cmp('exp_contacts_region_antigen', table[:, 6], tw[:, 6], np.where(regag, b_pc, 0.0).sum((1, 2)))
    cmp('p_on_contacts_region_antigen', table[:, 8], tw[:, 8], mean_b(b_pc, con))
    n_i = np.maximum(ok.sum(2), 1)
    cmp('rows.nll_mean', rows[:, :, 0], t['rows'][:, :, 0], np.where(ok, b_nll, 0.0).sum(2) / n_i)
    cmp('rows.exp_contacts_antigen', rows[:, :, 1], t['rows'][:, :, 1], np.where(okag, b_pc, 0.0).sum(2))
    cmp('rows.entropy_mean', rows[:, :, 3], t['rows'][:, :, 3], np.where(ok, b_ent, 0.0).sum(2) / n_i)
    if planes is not None:
        pc, ed = planes
        assert np.array_equal(pc, pc.transpose(0, 2, 1)) and np.array_equal(ed, ed.transpose(0, 2, 1)), f'{name}: planes not exactly symmetric'
        cmp('plane.p_contact', pc.astype(np.float64), t['p_contact'], b_pc + EPS * np.abs(t['p_contact']))
        cmp('plane.exp_dist', ed.astype(np.float64), t['exp_dist'], b_ed + EPS * np.abs(t['exp_dist']))
    print(f'\n{name}: ' + ', '.join(f'{k} err {e:.2e} share {s:.4f}' for k, (e, s) in report.items()))
    return report


CASES = [(L, B) for L in SHAPES for B in (1, 3)]


@pytest.mark.parametrize('L,B', CASES)
def test_logits_match_twin_and_are_bit_symmetric(L, B):
    c = shape_case(L, B)
    t = twin_of(c)
    lg = run_logits(c)
    assert lg.shape == (B, L, L, 64) and np.isfinite(lg).all()
    err = np.abs(lg.astype(np.float64) - t['logits'])
    bound = logit_bound(t['bound_scale'])
    print(f'\nL={L} B={B}: max |logits - twin| {err.max():.3e}, largest share of the bound {(err / bound).max():.4f}, logit range {lg.min():.1f} .. {lg.max():.1f}')
    assert (err <= bound).all()
    assert np.array_equal(lg.view(np.uint32), lg.transpose(0, 2, 1, 3).view(np.uint32))


def test_logits_match_the_reference_head():
    """The golden fixture through abx_distogram_logits against the reference's logits, under the bound of the host test."""
    from abx_amd import ops
    g = load_npz('distogram_head.npz')
    z, W, b = (tt(g[k]).to(DEV) for k in ('pair', 'weight', 'bias'))
    lg = ops.distogram_logits(z, ops.distogram_pack_weight(W), b).cpu().numpy().astype(np.float64)
    za = np.abs(g['pair'].astype(np.float64))
    scale = 0.5 * (za + za.transpose(0, 2, 1, 3)) @ np.abs(g['weight'].astype(np.float64)).T + np.abs(g['bias'].astype(np.float64))
    err = np.abs(lg - g['logits'].astype(np.float64))
    print(f'\nmax |logits - reference| {err.max():.3e}, largest share of the bound {(err / logit_bound(scale)).max():.4f}')
    assert (err <= logit_bound(scale)).all()


@pytest.mark.parametrize('L,B', CASES)
def test_scores_match_twin(L, B):
    c = shape_case(L, B)
    assert c['min_margin'] > 1e-4
    table, rows, planes = run_scores(c)
    check_against_twin(f'L={L} B={B}', table, rows, planes, twin_of(c), c['classes'], c['breaks'])
    # without the planes the table and the rows keep their bits (rows of masked residues skip the tile walk then)
    table2, rows2, _ = run_scores(c, planes=False)
    assert np.array_equal(table, table2) and np.array_equal(rows, rows2)


@pytest.mark.parametrize('name', list(VARIANTS))
def test_pair_set_edge_cases(name):
    """An empty region, a region of one residue, no antigen (Lab = L): the defined zeros, no NaN, and the twin's values."""
    c = variant_case(name)
    assert c['min_margin'] > 1e-4
    table, rows, planes = run_scores(c)
    t = twin_of(c)
    check_against_twin(name, table, rows, planes, t, c['classes'], c['breaks'])
    assert np.array_equal(table == 0, t['table'] == 0) and np.array_equal(rows == 0, t['rows'] == 0)
    if name == 'empty_region':
        assert (table[:, 2:] == 0).all()
    if name == 'no_antigen':
        assert (table[:, [1, 3, 6, 7, 8]] == 0).all() and (rows[:, :, 1:3] == 0).all()
    if name == 'one_residue':
        assert np.array_equal(table[:, 9], c['valid'].sum(1).numpy() - 1)


def test_a_design_does_not_depend_on_its_batch():
    """Sample 1 of a B = 3 call has the bits of the same sample run alone: table, rows, planes and logits."""
    c = shape_case(130, 3)
    table, rows, planes = run_scores(c)
    one = {k: (v[1:2] if k in ('pair', 'pb', 'valid') else v) for k, v in c.items()}
    t1, r1, p1 = run_scores(one)
    assert np.array_equal(table[1:2], t1) and np.array_equal(rows[1:2], r1)
    assert np.array_equal(planes[0][1:2], p1[0]) and np.array_equal(planes[1][1:2], p1[1])
    assert np.array_equal(run_logits(c)[1:2], run_logits(one))


@pytest.fixture(scope='module')
def gpu_model(params, cfg, oracle_diffuser):
    """Not analysis_gpu_cases.gpu_model: the IGSO(3) tables are the oracle's (set_tables), not the product's own from a fresh cache."""
    from abx_amd.model.abx import ScoreNetwork
    from abx_amd.diffuser.full_diffuser import FullDiffuser
    so3 = oracle_diffuser.so3
    D = FullDiffuser(cfg.diffuser)
    D.set_tables(so3._pdf, so3._cdf, so3._score_norms, DEV)
    m = ScoreNetwork(cfg.model, D)
    m.load_state_dict(params, strict=True)
    return m.to(DEV).eval(), D


def test_scorer_on_a_real_model_call(gpu_model, cfg):
    """One network call at L = 48 (the masked-tail complex of modules_L48.npz): DistogramScorer.score on its representations['pair'] against
    the twin on the same buffer copied to the host; the wild type and the logits of the same call too."""
    from abx_amd.confidence import DistogramScorer
    model, D = gpu_model
    m = load_npz('modules_L48.npz')
    b = feat_batch_from_golden(m)
    for k in ('seq_t', 'rigids_t', 't', 'rot_score_scaling', 'trans_score_scaling'):
        b[k] = tt(m['in.' + k])
    b = {k: (v.to(DEV) if torch.is_tensor(v) else tuple(x.to(DEV) for x in v) if isinstance(v, tuple) else v) for k, v in b.items()}
    model.max_chunk = None
    ret = model(b)
    Lab = b['anchor_flag'].shape[1]
    pair = ret['representations']['pair']
    atom14 = ret['heads']['folding']['final_atom14_positions'][:, :Lab]
    seq = torch.clamp(ret['heads']['sequence_module']['seq_0'][:, :Lab], min=0, max=19).long()
    sc = DistogramScorer(b, model, conf=cfg.model.heads.distogram)
    assert int((sc.classes & 4).ne(0).sum()) > 0 and not bool(sc.res_mask.all())        # a region, and the padded tail is masked
    table, rows, planes = sc.score(pair, atom14, seq, planes=True)
    wt, wr = sc.wild(pair)
    lg = sc.logits(pair, [0])
    torch.cuda.synchronize()
    t = sc.host(pair, atom14, seq)
    check_against_twin('model L=48', table.cpu().numpy(), rows.cpu().numpy(), tuple(p.cpu().numpy() for p in planes), t, sc.classes, sc.breaks.cpu())
    tw = sc.host(pair, sc.gt_atom14[None], sc.gt_seq[None], wild=True)
    check_against_twin('model L=48 wild', wt.cpu().numpy(), wr.cpu().numpy(), None, tw, sc.classes, sc.breaks.cpu())
    assert (np.abs(lg['logits'].cpu().numpy().astype(np.float64) - t['logits'][:1]) <= logit_bound(t['bound_scale'][:1])).all()
    assert lg['breaks'].shape == (63,) and float(table[0, 9]) > 0


def test_design_driver_writes_the_confidence_table(tmp_path):
    """`design --confidence` on the shipped 6ct7 complex: a TSV with a `wild` line, one line per design, the documented columns and finite
    values; without the flag no such file, and every other output file keeps its bytes."""
    from abx_amd import design
    from abx_amd.confidence import CONFIDENCE_COLUMNS, DELTA_COLUMNS
    common = pdb_args(CODES[:1]) + ['--num_samples', '3', '--mode', 'design', '--num_t', '2']
    out_a, out_b = str(tmp_path / 'with'), str(tmp_path / 'without')
    files_a = design.main(common + ['--output_dir', out_a, '--confidence', '--confidence_planes'])
    files_b = design.main(common + ['--output_dir', out_b])
    tsv = os.path.join(out_a, '6ct7_H_L_S_confidence.tsv')
    assert tsv in files_a and not [f for f in os.listdir(out_b) if 'confidence' in f]
    lines = table_lines(out_a, CODES[0], 'confidence')
    assert lines[0] == ['sample'] + list(CONFIDENCE_COLUMNS) + ['delta_' + c for c in DELTA_COLUMNS]
    assert [ln[0] for ln in lines[1:]] == ['wild', '0', '1', '2'] and all(len(ln) == len(lines[0]) for ln in lines)
    vals = np.array([[float(v) for v in ln[1:]] for ln in lines[1:]])
    assert np.isfinite(vals).all() and (vals[:, 9] > 0).all() and (vals[:, 0] > 0).all()
    assert (vals[0, 10:] == 0).all()                                # the wild line's own deltas
    plane = np.load(os.path.join(out_a, '6ct7_H_L_S_confidence_contacts.npy'))
    assert plane.ndim == 2 and plane.shape[0] == plane.shape[1] and np.isfinite(plane).all() and 0 <= plane.min() and plane.max() <= 1 + 1e-6
    assert np.allclose(plane, plane.T, atol=1e-7)
    names_b = sorted(os.path.relpath(f, out_b) for f in files_b)
    assert names_b == sorted(os.path.relpath(f, out_a) for f in files_a if 'confidence' not in os.path.basename(f))
    for n in names_b:
        assert open(os.path.join(out_a, n), 'rb').read() == open(os.path.join(out_b, n), 'rb').read(), n
