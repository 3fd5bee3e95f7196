"""Model-level parity on an MI355X (`pytest -m gpu`): the HIP ScoreNetwork / FullDiffuser / sampler against
(1) the committed golden vectors produced by the reference itself, (2) the oracle on larger seeded inputs, and
(3) size-independent properties at BASELINE-scale lengths."""
import os

import numpy as np
import pytest
import torch

from conftest import load_npz, tt, feat_batch_from_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def close(a, b, atol, rtol, name):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    err = np.abs(a - b)
    assert np.all(np.isfinite(a)), f'{name}: non-finite output'
    assert np.all(err <= atol + rtol * np.abs(b)), f'{name}: max err {err.max():.3e} (atol {atol} rtol {rtol}), max|ref| {np.abs(b).max():.3e}'


def to_dev(b):
    out = {}
    for k, v in b.items():
        if torch.is_tensor(v):
            out[k] = v.to(DEV)
        elif isinstance(v, tuple):
            out[k] = tuple(x.to(DEV) for x in v)
        else:
            out[k] = v
    return out


@pytest.fixture(scope='module')
def gpu_model(params, cfg, oracle_diffuser):
    from abx_amd.model.abx import ScoreNetwork
    from abx_amd.diffuser.full_diffuser import FullDiffuser
    g = load_npz('igso3_small.npz')
    so3 = oracle_diffuser.so3
    sn, cdf = so3._score_norms.clone(), so3._cdf.clone()
    sn[g['rows']] = tt(g['rows_score_norms'])
    cdf[g['rows']] = tt(g['rows_cdf'])
    so3._score_norms, so3._cdf = sn, cdf                 # oracle and product use identical (reference-pinned) tables
    D = FullDiffuser(cfg.diffuser)
    D.set_tables(so3._pdf, cdf, sn, DEV)
    m = ScoreNetwork(cfg.model, D)
    m.load_state_dict(params, strict=True)
    m = m.to(DEV).eval()
    return m, D


def test_full_call_matches_reference_golden(gpu_model, cfg):
    """One in-loop ScoreNetwork call (2 recycles + final pass, fp64 t): HIP path vs the reference's own outputs."""
    model, D = gpu_model
    m = load_npz('modules_tiny.npz')
    b = feat_batch_from_golden(load_npz('feat_tiny.npz'))
    for k in ('seq_t', 'rigids_t', 't', 'prev_pos', 'prev_seq', 'prev_pair', 'rot_score_scaling', 'trans_score_scaling'):
        b[k] = tt(m['in.' + k])
    b = to_dev(b)
    ret = model(b)
    torch.cuda.synchronize()
    f = ret['heads']['folding']
    assert torch.equal(b['seq_t'].cpu(), tt(m['final.seq_t_after']))
    assert torch.equal(ret['heads']['sequence_module']['seq_0'].cpu(), tt(m['out.seq_0']))
    close(ret['representations']['seq'], m['out.seq'], 1e-4, 1e-5, 'trunk seq')
    close(ret['representations']['pair'], m['out.pair'], 2e-4, 1e-5, 'trunk pair')
    close(f['rigids'], m['out.rigids'], 1e-4, 1e-4, 'rigids')                       # north_star: 1e-4 on frames
    close(f['representations']['structure_module'], m['out.structure_module'], 2e-4, 1e-5, 'structure_module')
    close(f['sidechains'][-1]['angles_sin_cos'], m['out.angles'], 2e-4, 0, 'angles')
    close(f['final_atom14_positions'], m['out.atom14'], 5e-4, 1e-5, 'atom14')
    close(f['final_atom_positions'], m['out.atom37'], 5e-4, 1e-5, 'atom37')
    close(ret['heads']['sequence_module']['logits'], m['out.logits'], 2e-4, 1e-5, 'logits')
    close(ret['heads']['predicted_lddt']['pLDDT'], m['out.pLDDT'], 2e-3, 1e-5, 'pLDDT')
    assert f['trans_score'].dtype == torch.float64 and f['rot_score'].dtype == torch.float32
    close(f['trans_score'], m['out.trans_score'], 2e-4, 1e-5, 'trans_score')
    rs, ref = f['rot_score'].cpu().numpy(), m['out.rot_score']
    dif = (b['fixed_mask'].cpu().numpy() == 0).reshape(-1)      # fixed residues: rot_score is rounding noise, masked out later
    bad = (np.abs(rs - ref) > 2e-4 + 1e-4 * np.abs(ref)).reshape(-1, 3).any(axis=1)[dif].mean()
    assert bad <= 0.02, f'rot_score bucket mismatches {bad}'
    from abx_amd.model.abx import get_prev
    prev = get_prev(b, ret, cfg.model)
    assert (prev['prev_pos'].cpu().numpy() != m['out.prev_pos']).mean() < 1e-3
    assert prev['prev_pair'].data_ptr() == ret['representations']['pair'].data_ptr()


def test_static_embeddings_match_oracle(gpu_model, params, cfg):
    from oracle import abx_oracle as O
    model, D = gpu_model
    b = feat_batch_from_golden(load_npz('feat_tiny.npz'))
    ss, ps = O.static_embeddings(params, b, cfg)
    eng = model._get_engine(torch.device(DEV))
    s2, p2 = eng.static_embeddings(to_dev(b), shared=False)
    close(s2, ss, 3e-5, 1e-5, 'static seq')
    close(p2, ps, 3e-5, 1e-5, 'static pair')


def test_warmup_call_fp32_t(gpu_model, cfg):
    model, D = gpu_model
    from abx_amd import sampler
    m = load_npz('modules_tiny.npz')
    b = to_dev(feat_batch_from_golden(load_npz('feat_tiny.npz')))
    ones = torch.ones(b['seq'].shape[0], device=DEV)
    b = sampler.set_t_feats(b, D, float(np.linspace(0.01, 1.0, 100)[::-1][0]), ones)
    assert b['t'].dtype == torch.float32
    ret = model(b)
    assert ret['heads']['folding']['trans_score'].dtype == torch.float32
    close(ret['heads']['folding']['rigids'], m['warm.rigids'], 1e-4, 1e-4, 'warm rigids')
    close(ret['heads']['sequence_module']['logits'], m['warm.logits'], 2e-4, 1e-5, 'warm logits')
    close(ret['heads']['folding']['trans_score'], m['warm.trans_score'], 2e-4, 1e-4, 'warm trans_score')
    assert torch.equal(ret['heads']['sequence_module']['seq_0'].cpu(), tt(m['warm.seq_0']))


def test_short_trajectory_matches_reference_golden(gpu_model, cfg):
    """The reference's sample_fn (num_t=4, trajectory mode) vs the HIP sampler under the recorded noise:
    tokens exact at every step, frames / atoms within tolerance."""
    from abx_amd import sampler
    model, D = gpu_model
    tj = load_npz('traj_tiny.npz')
    b = to_dev(feat_batch_from_golden(load_npz('feat_tiny.npz')))

    def noise_fn(k):
        return dict(z_rot=tt(tj[f'n{k}.z_rot']).to(DEV), z_trans=tt(tj[f'n{k}.z_trans']).to(DEV), jumps=tt(tj[f'n{k}.jumps']).to(DEV))

    traj = sampler.sample_fn(b, cfg, D, model, mode='trajectory', num_t=4, noise_fn=noise_fn)
    assert len(traj) == 4
    for k, d in enumerate(traj):
        assert float(d['time']) == float(tj[f'k{k}.time'])
        assert np.array_equal(d['seq'].cpu().numpy(), tj[f'k{k}.seq']), f'step {k}: tokens differ'
        close(d['atom14_results'], tj[f'k{k}.atom14'], 5e-3, 1e-4, f'step {k} atom14')
        close(d['pLDDT'], tj[f'k{k}.pLDDT'], 1e-2, 1e-4, f'step {k} pLDDT')
    close(traj[-1]['rigids_t'], tj['final.rigids_t'], 2e-3, 1e-4, 'final rigids')
    only_last = sampler.sample_fn(b, cfg, D, model, mode='design', num_t=4, noise_fn=noise_fn)
    assert len(only_last) == 1 and torch.equal(only_last[0]['seq'], traj[-1]['seq'])


def test_hip_built_igso3_tables_run_the_golden_trajectory(params, cfg, tmp_path):
    """every other model-level test injects reference-pinned IGSO(3) tables (set_tables).  Here the tables come
    from abx_igso3_tables (the product's default path: FullDiffuser.to(device) with an empty cache directory) and the reference's
    recorded num_t = 4 trajectory is replayed under its own noise: tokens exact at every step, frames / atoms at the tolerance of
    the pinned-table test (the table entries a trajectory visits are the well-conditioned ones)."""
    import copy
    from abx_amd import sampler
    from abx_amd.model.abx import ScoreNetwork
    from abx_amd.diffuser.full_diffuser import FullDiffuser
    dc = copy.deepcopy(cfg.diffuser)
    dc.so3.cache_dir = str(tmp_path / 'igso3_cache')            # empty: the tables are built by the HIP kernel
    D = FullDiffuser(dc).to(DEV)
    assert os.path.exists(os.path.join(D._cache_path(), 'score_norms.npy'))
    model = ScoreNetwork(cfg.model, D)
    model.load_state_dict(params, strict=True)
    model = model.to(DEV).eval()
    tj = load_npz('traj_tiny.npz')
    b = to_dev(feat_batch_from_golden(load_npz('feat_tiny.npz')))

    def noise_fn(k):
        return dict(z_rot=tt(tj[f'n{k}.z_rot']).to(DEV), z_trans=tt(tj[f'n{k}.z_trans']).to(DEV), jumps=tt(tj[f'n{k}.jumps']).to(DEV))

    traj = sampler.sample_fn(b, cfg, D, model, mode='trajectory', num_t=4, noise_fn=noise_fn)
    for k, d in enumerate(traj):
        assert np.array_equal(d['seq'].cpu().numpy(), tj[f'k{k}.seq']), f'step {k}: tokens differ'
        close(d['atom14_results'], tj[f'k{k}.atom14'], 5e-3, 1e-4, f'step {k} atom14')
    close(traj[-1]['rigids_t'], tj['final.rigids_t'], 2e-3, 1e-4, 'final rigids')


def _synthetic_batch(D, name, B, seed=3, n_masked_tail=0, dev=DEV):
    from abx_amd import synthetic, features
    w = synthetic.WORKLOADS[name] if isinstance(name, str) else name
    cx = synthetic.make_complex(seed=seed, n_masked_tail=n_masked_tail, **w)
    raw = {k: v.to(dev) for k, v in synthetic.replicate(cx, B).items()}
    torch.manual_seed(11)
    return features.build_features(raw, D)


def test_medium_complex_vs_oracle(gpu_model, params, cfg, oracle_diffuser):
    """L = 72 (not a multiple of any tile), 3 samples with different noise, chunked 2+1, padded antigen tail:
    one full call (3 passes) HIP vs oracle."""
    from oracle import abx_oracle as O
    model, D = gpu_model
    w = dict(L_heavy=30, L_light=26, L_antigen=16, cdr=(20, 27))
    b = _synthetic_batch(D, w, B=3, n_masked_tail=2)
    t_ = torch.full((3,), 0.6060606060606061, dtype=torch.float64, device=DEV)
    from abx_amd import sampler
    b = sampler.set_t_feats(b, D, t_, torch.ones(3, device=DEV))
    cpu = {k: (v.cpu() if torch.is_tensor(v) else tuple(x.cpu() for x in v) if isinstance(v, tuple) else v) for k, v in b.items()}
    model.max_chunk = 2
    ret = model(b)
    model.max_chunk = None
    ref = O.score_network(params, cpu, cfg, oracle_diffuser)
    f, fr = ret['heads']['folding'], ref['heads']['folding']
    agree = (ret['heads']['sequence_module']['seq_0'].cpu() == ref['heads']['sequence_module']['seq_0']).float().mean()
    assert agree == 1.0, f'seq_0 agreement {agree}'
    close(ret['representations']['pair'], ref['representations']['pair'], 3e-4, 1e-4, 'pair')
    close(f['rigids'], fr['rigids'], 1e-4, 1e-4, 'rigids')
    close(f['final_atom14_positions'], fr['final_atom14_positions'], 1e-3, 1e-4, 'atom14')
    close(ret['heads']['sequence_module']['logits'], ref['heads']['sequence_module']['logits'], 3e-4, 1e-4, 'logits')
    close(f['trans_score'], fr['trans_score'], 3e-4, 1e-4, 'trans_score')
    close(ret['heads']['predicted_lddt']['pLDDT'], ref['heads']['predicted_lddt']['pLDDT'], 5e-3, 1e-4, 'pLDDT')


def test_split_f16_contraction_path_vs_oracle(gpu_model, params, cfg, oracle_diffuser):
    """L = 120 (k padding: 120 -> 128), 5 samples in one chunk: large enough for the split-f16 GEMM kernels, so the triangle
    multiplication runs through the f16-image projections (C_split), the pair-transposed row gather of the incoming variant
    and the plane contraction.  One full call (3 passes) HIP vs oracle, then the same call on the exact fp32 MFMA kernels."""
    from oracle import abx_oracle as O
    from abx_amd import sampler, ops
    model, D = gpu_model
    w = dict(L_heavy=50, L_light=44, L_antigen=26, cdr=(30, 39))
    B = 5
    assert ops.gemm_split_eligible(120 * 120, 128, 192, B)
    b = _synthetic_batch(D, w, B=B, n_masked_tail=3)
    t_ = torch.full((B,), 0.4040404040404041, dtype=torch.float64, device=DEV)
    b = sampler.set_t_feats(b, D, t_, torch.ones(B, device=DEV))
    cpu = {k: (v.cpu() if torch.is_tensor(v) else tuple(x.cpu() for x in v) if isinstance(v, tuple) else v) for k, v in b.items()}

    def run(exact):
        bb = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}
        ops.GEMM_EXACT = exact
        try:
            model.max_chunk = None
            r = model(bb)
            torch.cuda.synchronize()
        finally:
            ops.GEMM_EXACT = False
        # the returned tensors live in the model's ping-pong buffers: copy them before the next call overwrites them
        cp = lambda d: {k: (cp(v) if isinstance(v, dict) else v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}
        return cp(r)

    ret, rex = run(False), run(True)
    ref = O.score_network(params, cpu, cfg, oracle_diffuser)
    for tag, r in (('exact', rex), ('split', ret)):
        f, fr = r['heads']['folding'], ref['heads']['folding']
        agree = (r['heads']['sequence_module']['seq_0'].cpu() == ref['heads']['sequence_module']['seq_0']).float().mean()
        assert agree == 1.0, f'{tag}: seq_0 agreement {agree}'
        close(r['representations']['pair'], ref['representations']['pair'], 3e-4, 1e-4, tag + ' pair')
        close(f['rigids'], fr['rigids'], 1e-4, 1e-4, tag + ' rigids')
        close(f['final_atom14_positions'], fr['final_atom14_positions'], 1e-3, 1e-4, tag + ' atom14')
        close(r['heads']['sequence_module']['logits'], ref['heads']['sequence_module']['logits'], 3e-4, 1e-4, tag + ' logits')
    assert not torch.equal(ret['representations']['pair'], rex['representations']['pair']), 'both runs took the same kernels'


def test_out_of_range_activations_fall_back_to_the_exact_kernels(params, cfg, oracle_diffuser, gpu_model):
    """No range contract reaches the caller (the reference's fp32 contractions have none, seqformer.py:260-312, 443-504):
    with one key channel of the starting-node triangle attention and one right-operand channel of the outgoing triangle
    multiplication rescaled beyond 4095 (the plane range of the split-f16 kernels), a network call still returns the oracle's numbers: the kernels flag the op at the source (ops.range_word), ScoreNetwork repeats the flagged passes on the exact
    fp32-MFMA kernels and logs which op classes left the range."""
    from collections import OrderedDict
    from oracle import abx_oracle as O
    from abx_amd import sampler, ops
    from abx_amd.model.abx import ScoreNetwork
    _, D = gpu_model
    big = OrderedDict((k, v.clone()) for k, v in params.items())
    blk = 'impl.seqformer.seqformer.blocks.0.'
    # one key channel per head x 6000 with its query channel / 6000, one right tri-mul channel x 5000 with its left channel / 5000:
    # the network computes the same function (logits and products unchanged), but those key / right-operand values pass 4095
    ta, tm = blk + 'triangle_attention_starting_node.attn.', blk + 'triangle_multiplication_outgoing.'
    for h in range(4):
        big[ta + 'proj_k.weight'][h * 48 + 3] *= 6000.0
        big[ta + 'proj_q.weight'][h * 48 + 3] /= 6000.0
    big[tm + 'right_proj.weight'][5] *= 5000.0
    big[tm + 'left_proj.weight'][5] /= 5000.0
    for side, fac in (('right', 5000.0), ('left', 1 / 5000.0)):
        if big.get(tm + side + '_proj.bias') is not None:
            big[tm + side + '_proj.bias'][5] *= fac
    model = ScoreNetwork(cfg.model, D)
    model.load_state_dict(big, strict=True)
    model = model.to(DEV).eval()
    w = dict(L_heavy=50, L_light=44, L_antigen=26, cdr=(30, 39))
    B = 3
    b = _synthetic_batch(D, w, B=B)
    t_ = torch.full((B,), 0.4040404040404041, dtype=torch.float64, device=DEV)
    b = sampler.set_t_feats(b, D, t_, torch.ones(B, device=DEV))
    cpu = _cpu_copy(b)
    cp = lambda d: {k: (cp(v) if isinstance(v, dict) else v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}
    ret = cp(model({k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}))
    assert len(model.range_log) >= 1, 'the scaled projections did not leave the split range: the test does not test'
    seen = set(sum((e['ops'] for e in model.range_log), []))
    assert 'tri_attn' in seen and ('contraction' in seen or 'tri_mul_tail' in seen), model.range_log
    # per op class (round 5): only the classes that left the range went exact - the triangle multiplication's contraction first (its
    # repeat still flagged the attention, which joined) - never the pair transition, the IPA tail or the heads
    ex = set(model.range_log[-1]['exact_ops'])
    assert 'tri_attn' in ex and ex & {'contraction', 'plane_projection', 'tri_mul_tail'}, model.range_log
    assert not ex & {'pair_transition', 'ipa_tail', 'heads_tail', 'ipa_pair_init', 'gemm'}, model.range_log
    assert model.range_log[-1]['repeats'] == len(model.range_log[-1]['exact_ops'])
    ops.GEMM_EXACT = True
    try:
        rex = cp(model({k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}))
    finally:
        ops.GEMM_EXACT = False
    ref = O.score_network(big, cpu, cfg, oracle_diffuser)
    f, fe, fr = ret['heads']['folding'], rex['heads']['folding'], ref['heads']['folding']
    assert torch.isfinite(f['rigids']).all() and torch.isfinite(ret['representations']['pair']).all()
    # the flagged passes ran on the exact kernels in both runs (a pass that stayed in range kept the split kernels: not the same bits)
    close(f['rigids'], fe['rigids'], 1e-4, 1e-4, 'rigids vs forced exact')
    close(ret['representations']['pair'], rex['representations']['pair'], 3e-4, 1e-4, 'pair vs forced exact')
    assert torch.equal(ret['heads']['sequence_module']['seq_0'], rex['heads']['sequence_module']['seq_0'])
    assert (ret['heads']['sequence_module']['seq_0'].cpu() == ref['heads']['sequence_module']['seq_0']).all()
    close(f['rigids'], fr['rigids'], 1e-4, 1e-4, 'rigids')
    close(ret['heads']['sequence_module']['logits'], ref['heads']['sequence_module']['logits'], 3e-4, 1e-4, 'logits')
    # and the in-range model of the other tests logs nothing
    m0, _ = gpu_model
    n0 = len(m0.range_log)
    m0({k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()})
    assert len(m0.range_log) == n0 == 0, m0.range_log


def test_range_fallback_per_op_class_sticky_and_without_a_length_limit(params, cfg, oracle_diffuser, gpu_model):
    """VERDICT r4 #4 / ADVICE r4: L = 416 (> 389: the exact attention kernel walks such rows in key chunks now - the reference's attention
    has no length limit, seqformer.py:272-312).  (a) a key channel x 6000 flags the triangle attention: ONE repeat with only that class
    exact, results = the oracle's; the second flagged call makes the class sticky (logged), the third runs without a repeat.
    (b) a pair-transition hidden channel beyond 4094 flags that class only (the attention stays on the split-f16 kernel; round 4 aborted
    here with 'L too large'); results = the forced-exact run of the same model."""
    from collections import OrderedDict
    from oracle import abx_oracle as O
    from abx_amd import sampler, ops
    from abx_amd.model.abx import ScoreNetwork
    _, D = gpu_model
    blk = 'impl.seqformer.seqformer.blocks.0.'
    w = dict(L_heavy=120, L_light=110, L_antigen=186, cdr=(30, 39))
    B = 1
    b = _synthetic_batch(D, w, B=B)
    assert b['seq'].shape[1] == 416
    t_ = torch.full((B,), 0.4040404040404041, dtype=torch.float64, device=DEV)
    b = sampler.set_t_feats(b, D, t_, torch.ones(B, device=DEV))
    fresh = lambda: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}
    cp = lambda d: {k: (cp(v) if isinstance(v, dict) else v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}

    # ---- (a) attention
    big = OrderedDict((k, v.clone()) for k, v in params.items())
    ta = blk + 'triangle_attention_starting_node.attn.'
    for h in range(4):
        big[ta + 'proj_k.weight'][h * 48 + 3] *= 6000.0
        big[ta + 'proj_q.weight'][h * 48 + 3] /= 6000.0
    model = ScoreNetwork(cfg.model, D)
    model.load_state_dict(big, strict=True)
    model = model.to(DEV).eval()
    ret = cp(model(fresh()))
    assert len(model.range_log) == 1, model.range_log
    e = model.range_log[0]
    assert e['exact_ops'] == ['tri_attn'] and e['repeats'] == 1 and not e.get('sticky'), e
    ref = O.score_network(big, _cpu_copy(b), cfg, oracle_diffuser)
    close(ret['heads']['folding']['rigids'], ref['heads']['folding']['rigids'], 1e-4, 1e-4, 'rigids vs oracle (chunked exact attention)')
    assert (ret['heads']['sequence_module']['seq_0'].cpu() == ref['heads']['sequence_module']['seq_0']).all()
    ret2 = cp(model(fresh()))
    assert len(model.range_log) == 2 and model.range_log[1].get('sticky') and model.range_log[1]['repeats'] == 1, model.range_log
    ret3 = cp(model(fresh()))
    assert len(model.range_log) == 2, 'a sticky class must not be flagged (or repeated) again'
    for r in (ret2, ret3):
        assert torch.equal(r['heads']['folding']['rigids'], ret['heads']['folding']['rigids'])
    assert model.range_sticky_ops == ['tri_attn'] and model.range_log[1].get('sticky_set') == ['tri_attn']
    # the sticky set belongs to ONE complex.  Another complex (other coordinates and sequence, same model) starts clean: its first
    # flagged call is repeated once with only the flagged class exact and is not sticky - whatever ran before it on this module
    b2 = _synthetic_batch(D, w, B=B, seed=5)
    b2 = sampler.set_t_feats(b2, D, t_, torch.ones(B, device=DEV))
    n_log = len(model.range_log)
    model({k: (v.clone() if torch.is_tensor(v) else v) for k, v in b2.items()})
    assert len(model.range_log) == n_log + 1, model.range_log[n_log:]
    e2 = model.range_log[-1]
    assert e2['exact_ops'] == ['tri_attn'] and e2['repeats'] == 1 and not e2.get('sticky'), e2
    assert model.range_sticky_ops == []

    # ---- (b) pair transition: hidden channel 7 scaled up in the first layer, down in the second (the same function)
    big = OrderedDict((k, v.clone()) for k, v in params.items())
    tr = blk + 'pair_transition.transition.'
    big[tr + '1.weight'][7] *= 3.0e4
    big[tr + '1.bias'][7] *= 3.0e4
    big[tr + '3.weight'][:, 7] /= 3.0e4
    model = ScoreNetwork(cfg.model, D)
    model.load_state_dict(big, strict=True)
    model = model.to(DEV).eval()
    ret = cp(model(fresh()))
    assert len(model.range_log) == 1 and model.range_log[0]['exact_ops'] == ['pair_transition'], model.range_log
    ops.GEMM_EXACT = True
    try:
        rex = cp(model(fresh()))
    finally:
        ops.GEMM_EXACT = False
    close(ret['heads']['folding']['rigids'], rex['heads']['folding']['rigids'], 1e-4, 1e-4, 'rigids vs forced exact')
    assert torch.equal(ret['heads']['sequence_module']['seq_0'], rex['heads']['sequence_module']['seq_0'])


def test_split_f16_short_trajectory_vs_oracle(gpu_model, params, cfg, oracle_diffuser):
    """Driver-level parity with the split-f16 kernels active (L = 112, 3 samples: every GEMM, the plane contraction and the
    triangle attention run on the float16 matrix cores), TEACHER-FORCED (SURVEY §7 hard part 1a): the warm-up call and every grid
    point of a 3-point trajectory start from the ORACLE's state (rigids_t, seq_t, self-conditioning tensors), so each call and
    each reverse step is compared on identical inputs at 1e-4-class tolerances, for both HIP arithmetic paths.  Inside a call the
    two recycles feed DISCRETE decisions back (distogram bins of prev_pos, argmax tokens): both sides are traced, and a sample whose
    recycle decisions differ from the oracle's is excused from the tight comparison only if every difference is a genuine tie (a
    pseudo-beta distance within 1e-3 A of a bin boundary / a logit margin below 1e-3) and at most one sample per call is affected.
    Then the free-running HIP sampler against the free-running oracle under the same injected noise: tokens exact at every step."""
    from oracle import abx_oracle as O
    from abx_amd import sampler, ops
    from abx_amd.model.abx import get_prev
    model, D = gpu_model
    w = dict(L_heavy=46, L_light=40, L_antigen=26, cdr=(28, 36))
    B, L = 3, 112
    assert ops.gemm_mode(L) == 2
    b = _synthetic_batch(D, w, B=B)
    cpu0 = _cpu_copy(b)
    gen = torch.Generator().manual_seed(5)
    num_t = 3
    noise = [dict(z_rot=torch.randn(B, L, 3, generator=gen), z_trans=torch.randn(B, L, 3, generator=gen),
                  jumps=torch.poisson(torch.full((B, L, 20), 0.02), generator=gen)) for _ in range(num_t - 1)]
    model.max_chunk = None
    pp = cfg.model.embeddings_and_seqformer.prev_pos
    breaks = torch.linspace(pp.min_bin, pp.max_bin, steps=pp.num_bins - 1).double()
    dm_cpu = (1 - cpu0['fixed_mask']) * cpu0['atom14_gt_exists'][..., 0]
    dt = torch.tensor(1 / num_t)
    steps = np.linspace(0.01, 1.0, num_t)[::-1]

    import abx_amd.model.abx as abx_mod

    class trace_recycles:
        """Records (distogram bins, argmax tokens, + for the oracle: pseudo-beta distances and logits) at every get_prev of a call."""
        def __init__(self, mod, oracle):
            self.mod, self.oracle, self.rec = mod, oracle, []

        def __enter__(self):
            self.orig = self.mod.get_prev

            def wrapped(batch, value, conf):
                out = self.orig(batch, value, conf)
                item = dict(bins=out['prev_pos'].detach().cpu().clone(), seq_0=value['heads']['sequence_module']['seq_0'].detach().cpu().clone())
                if self.oracle:
                    pb = O.pseudo_beta_v2(value['heads']['folding']['final_atom_positions']).double()
                    item['dist'] = (pb[:, :, None] - pb[:, None]).norm(dim=-1)
                    item['logits'] = value['heads']['sequence_module']['logits'].double().clone()
                self.rec.append(item)
                return out
            self.mod.get_prev = wrapped
            return self

        def __exit__(self, *exc):
            self.mod.get_prev = self.orig

    def oracle_call(state):
        with trace_recycles(O, True) as tr:
            r = O.score_network(params, state, cfg, oracle_diffuser)
        return r, tr.rec

    def hip_call(state, exact):
        """One HIP ScoreNetwork call on a device copy of the oracle's state."""
        bb = to_dev({k: (v.clone() if torch.is_tensor(v) else v) for k, v in state.items()})
        ops.GEMM_EXACT = exact
        try:
            with trace_recycles(abx_mod, False) as tr:
                r = model(bb)
            torch.cuda.synchronize()
        finally:
            ops.GEMM_EXACT = False
        return bb, r, tr.rec

    def tied_samples(name, htrace, otrace):
        """Samples whose recycle decisions differ from the oracle's; every difference must be a tie."""
        assert len(htrace) == len(otrace) == cfg.model.num_recycle
        tied = torch.zeros(B, dtype=torch.bool)
        for r, (hh, oo) in enumerate(zip(htrace, otrace)):
            mism = hh['bins'] != oo['bins']
            if mism.any():
                assert float((oo['dist'][mism][:, None] - breaks[None]).abs().min(dim=1).values.max()) < 1e-3, f'{name}: recycle {r} bins'
                assert int((hh['bins'][mism] - oo['bins'][mism]).abs().max()) == 1
                tied |= mism.flatten(1).any(dim=1)
            ms = hh['seq_0'] != oo['seq_0']
            if ms.any():
                top2 = oo['logits'][ms].topk(2, dim=-1).values
                assert float((top2[:, 0] - top2[:, 1]).max()) < 1e-3, f'{name}: recycle {r} tokens'
                tied |= ms.any(dim=1)
        assert int(tied.sum()) <= 1, f'{name}: {int(tied.sum())} samples hit a tie inside the call'
        return tied

    def compare_call(tag, state_before_all, ro_all, state_after_all, otrace):
        for exact in (False, True):
            bb_all, rh_all, htrace = hip_call(state_before_all, exact)
            name = f'{tag} {"exact" if exact else "split"}'
            keep = ~tied_samples(name, htrace, otrace)

            def pick(tree):
                return {k: (pick(v) if isinstance(v, dict) else
                            (v[keep.to(v.device)] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == B else v)) for k, v in tree.items()}
            rh, ro, bb = pick(rh_all), pick(ro_all), pick(bb_all)
            state_before, state_after = pick(state_before_all), pick(state_after_all)
            f, fr = rh['heads']['folding'], ro['heads']['folding']
            assert torch.equal(rh['heads']['sequence_module']['seq_0'].cpu(), ro['heads']['sequence_module']['seq_0']), name + ' seq_0'
            assert torch.equal(bb['seq_t'].cpu(), state_after['seq_t']), name + ' seq_t after the call'
            close(f['rigids'], fr['rigids'], 1e-4, 1e-4, name + ' rigids')
            close(f['final_atom14_positions'], fr['final_atom14_positions'], 5e-4, 1e-4, name + ' atom14')
            close(rh['heads']['sequence_module']['logits'], ro['heads']['sequence_module']['logits'], 2e-4, 1e-4, name + ' logits')
            close(f['trans_score'], fr['trans_score'], 2e-4, 1e-4, name + ' trans_score')
            close(rh['heads']['predicted_lddt']['pLDDT'], ro['heads']['predicted_lddt']['pLDDT'], 3e-3, 1e-4, name + ' pLDDT')
            rs, ref = f['rot_score'].cpu().numpy(), fr['rot_score'].numpy()
            dif = (state_before['fixed_mask'].numpy() == 0).reshape(-1)
            bad = (np.abs(rs - ref) > 2e-4 + 1e-4 * np.abs(ref)).reshape(-1, 3).any(axis=1)[dif].mean()
            assert bad <= 0.05, f'{name}: rot_score bucket mismatches {bad}'
            # self-conditioning distogram: index work; only pairs whose predicted distance sits on a bin boundary may differ
            hip_bins = get_prev(bb, rh, cfg.model)['prev_pos'].cpu()
            ora_bins = O.get_prev(state_after, ro, cfg)['prev_pos']
            mism = hip_bins != ora_bins
            assert float(mism.float().mean()) < 2e-4, f'{name}: {int(mism.sum())} distogram bins differ'
            if mism.any():
                pb = O.pseudo_beta_v2(fr['final_atom_positions']).double()
                dist = (pb[:, :, None] - pb[:, None]).norm(dim=-1)
                assert float((dist[mism][:, None] - breaks[None]).abs().min(dim=1).values.max()) < 1e-3
                assert int((hip_bins[mism] - ora_bins[mism]).abs().max()) == 1

    clone = lambda d: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}
    # ---- warm-up call (inference.py:209-211): fp32 t, no self-conditioning state yet
    st = O.set_t_feats(clone(cpu0), oracle_diffuser, steps[0], torch.ones(B))
    before = clone(st)
    ro, otr = oracle_call(st)
    compare_call('warm-up', before, ro, st, otr)
    st.update(O.get_prev(st, ro, cfg))
    # ---- grid points
    for k, t in enumerate(steps):
        if t > 0.01:
            t_ = torch.tile(torch.tensor(t), (B,))
            st = O.set_t_feats(st, oracle_diffuser, t_, torch.ones(B))
        before = clone(st)
        ro, otr = oracle_call(st)
        compare_call(f'grid point {k}', before, ro, st, otr)
        if t > 0.01:
            fo = ro['heads']['folding']
            st.update(O.get_prev(st, ro, cfg))
            rig_o, seq_o = oracle_diffuser.reverse(rigid_t=st['rigids_t'], seq_t=st['seq_t'], rot_score=fo['rot_score'],
                                                   trans_score=fo['trans_score'], logits_t=ro['heads']['sequence_module']['logits'],
                                                   diffuse_mask=dm_cpu, t=t_, dt=dt, noise=noise[k])
            rig_h, seq_h = D.reverse(rigid_t=st['rigids_t'].to(DEV), seq_t=st['seq_t'].to(DEV), rot_score=fo['rot_score'].to(DEV),
                                     trans_score=fo['trans_score'].to(DEV), logits_t=ro['heads']['sequence_module']['logits'].to(DEV),
                                     diffuse_mask=dm_cpu.to(DEV), t=t_.to(DEV), dt=float(dt),
                                     noise={kk: v.to(DEV) for kk, v in noise[k].items()})
            assert torch.equal(seq_h.cpu(), seq_o.long()), f'reverse step {k}: tokens'
            close(rig_h, rig_o, 2e-6, 1e-6, f'reverse step {k} rigids')
            st['rigids_t'], st['seq_t'] = rig_o, seq_o
    # ---- free-running samplers under the same noise: tokens exact at every step
    nf = lambda k: {kk: v.to(DEV) for kk, v in noise[k].items()}
    traj = sampler.sample_fn(b, cfg, D, model, mode='trajectory', num_t=num_t, noise_fn=nf)
    ref = O.sample_fn(params, cpu0, cfg, oracle_diffuser, mode='trajectory', num_t=num_t, noise_fn=lambda k: noise[k])
    assert len(traj) == len(ref) == num_t
    for k, (d, r) in enumerate(zip(traj, ref)):
        assert torch.equal(d['seq'].cpu(), r['seq']), f'step {k}: tokens differ'
        assert torch.equal(d['seq_t'].cpu().long(), r['seq_t'].long()), f'step {k}: seq_t differs'
        assert torch.isfinite(d['rigids_t']).all()


def test_full_size_properties(gpu_model, cfg):
    """BASELINE-scale length (L = 352): finite outputs, sample-permutation equivariance, shared-context == per-sample
    context, chunking invariance (bit-exact: every kernel is batch-independent)."""
    model, D = gpu_model
    from abx_amd import sampler
    B = 3
    b = _synthetic_batch(D, 'L352', B=B)
    t_ = torch.full((B,), 0.5050505050505051, dtype=torch.float64, device=DEV)
    b = sampler.set_t_feats(b, D, t_, torch.ones(B, device=DEV))

    def run(batch, chunk, shared):
        bb = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}
        if shared:
            bb['_shared_context'] = True
        model.max_chunk = chunk
        r = model(bb)
        torch.cuda.synchronize()
        return {'rigids': r['heads']['folding']['rigids'].clone(), 'logits': r['heads']['sequence_module']['logits'].clone(),
                'pair': r['representations']['pair'][:, :8, :8].clone(), 'seq_0': r['heads']['sequence_module']['seq_0'].clone()}

    a = run(b, 3, False)
    for v in a.values():
        assert torch.isfinite(v.double()).all()
    c = run(b, 1, True)
    for k in a:
        assert torch.equal(a[k], c[k]), f'chunking / shared-context changed {k}'
    perm = [2, 0, 1]
    pb = {k: (v[perm] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == B else v) for k, v in b.items()}
    pb['rigidgroups_gt_frames'] = tuple(x[perm] for x in b['rigidgroups_gt_frames'])
    d = run(pb, 3, False)
    for k in a:
        assert torch.equal(a[k][perm], d[k]), f'sample permutation changed {k}'
    model.max_chunk = None


def test_device_rng_sampling_is_shard_invariant(gpu_model, cfg):
    """4 samples run as one batch == the same samples run as two 'ranks' of 2 (per-sample Philox keys): the multi-GPU
    sharding changes nothing but where a sample runs."""
    from abx_amd import sampler, synthetic, features
    model, D = gpu_model
    cx = {k: v.to(DEV) for k, v in synthetic.make_complex(seed=5, **synthetic.WORKLOADS['tiny']).items()}

    def feats_fn(batch, sid):
        g = torch.Generator(device='cpu')
        outs = []
        for s in sid.tolist():                         # per-sample CPU generator: init noise independent of batching
            g.manual_seed(1000 + s)
            L = batch['seq'].shape[1]
            outs.append(dict(rot_axis=torch.randn(1, L, 3, generator=g), rot_u=torch.rand(1, L, generator=g),
                             trans_z=torch.randn(1, L, 3, generator=g), seq=torch.randint(0, 20, (1, L), generator=g)))
        noise = {k: torch.cat([o[k] for o in outs]).to(DEV) for k in outs[0]}
        return features.build_features(batch, D, noise=noise)

    full = sampler.design_samples(cx, cfg, D, model, num_samples=4, num_t=3, seed=9, features_fn=feats_fn)
    parts = []
    for r in range(2):
        ids = sampler.shard_sample_ids(4, r, 2)
        batch = {k: v[None].expand(len(ids), *v.shape).contiguous() for k, v in cx.items()}
        sid = torch.tensor(ids, device=DEV)
        batch = feats_fn(batch, sid)
        batch['_shared_context'] = True
        D.seed = 9
        parts.append(sampler.sample_fn(batch, cfg, D, model, num_t=3, sample_ids=sid)[-1])
    seq = torch.cat([p['seq'] for p in parts])
    atoms = torch.cat([p['atom14_results'] for p in parts])
    assert torch.equal(full['seq'], seq)
    assert torch.equal(full['atom14'], atoms)
    assert len(set(map(tuple, full['seq'].cpu().tolist()))) >= 1


def test_init_features_match_reference_golden(gpu_model, cfg):
    """Row I of SURVEY §8a on the device: the feature pipeline + FullDiffuser.sample_ref (design) and .forward_marginal
    (optimize, incl. the x_tilde token jump) under the reference's recorded draws."""
    from abx_amd import features
    model, D = gpu_model
    f = load_npz('feat_tiny.npz')
    raw = {k[4:]: tt(v).to(DEV) for k, v in f.items() if k.startswith('raw.')}
    noise = {k[6:]: tt(v).to(DEV) for k, v in f.items() if k.startswith('noise.')}
    b = features.build_features(dict(raw), D, generate_area='H3', noise=noise)
    assert torch.equal(b['seq_t'].cpu(), tt(f['feat.seq_t'])) and torch.equal(b['fixed_mask'].cpu(), tt(f['feat.fixed_mask']))
    close(b['rigids_t'], f['feat.rigids_t'], 2e-5, 1e-6, 'design rigids_t')
    close(b['torsion_angles_sin_cos'], f['feat.torsion_angles_sin_cos'], 2e-5, 0, 'torsions')   # torch-on-GPU vs CPU rounding of the feature pipeline
    close(b['rigids_0'], f['feat.rigids_0'], 2e-5, 0, 'rigids_0')
    g = load_npz('optimize_tiny.npz')
    noise = {k[6:]: tt(v).to(DEV) for k, v in g.items() if k.startswith('noise.')}
    b = features.build_features(dict(raw), D, generate_area='H3', opt_step=4, noise=noise)
    assert torch.equal(b['seq_t'].cpu(), tt(g['feat.seq_t']))
    close(b['t'], g['feat.t'], 0, 0, 't')
    close(b['rigids_t'], g['feat.rigids_t'], 2e-5, 1e-6, 'optimize rigids_t')
    close(b['trans_score'], g['feat.trans_score'], 2e-5, 1e-5, 'optimize trans_score')


def test_optimize_mode_trajectory_matches_reference_golden(gpu_model, cfg):
    """The reference's sample_fn(mode='optimize', opt_step=4): 4 grid points, HIP sampler under the recorded noise."""
    from abx_amd import sampler
    model, D = gpu_model
    g = load_npz('optimize_tiny.npz')
    b = feat_batch_from_golden(load_npz('feat_tiny.npz'))
    for k in ('rigids_t', 'seq_t', 't', 'fixed_mask', 'rigids_0'):
        b[k] = tt(g['feat.' + k])
    b = to_dev(b)

    def noise_fn(k):
        return dict(z_rot=tt(g[f'n{k}.z_rot']).to(DEV), z_trans=tt(g[f'n{k}.z_trans']).to(DEV), jumps=tt(g[f'n{k}.jumps']).to(DEV))

    traj = sampler.sample_fn(b, cfg, D, model, mode='optimize', num_t=100, noise_fn=noise_fn)
    assert len(traj) == 1 and float(traj[0]['time']) == float(g['last.time'])
    assert np.array_equal(traj[0]['seq'].cpu().numpy(), g['last.seq'])
    close(traj[0]['atom14_results'], g['last.atom14'], 5e-3, 1e-4, 'optimize atom14')
    close(traj[0]['pLDDT'], g['last.pLDDT'], 1e-2, 1e-4, 'optimize pLDDT')
    close(traj[0]['rigids_t'], g['final.rigids_t'], 2e-3, 1e-4, 'optimize final rigids')


def test_design_driver_trajectory_dump(tmp_path):
    """End to end through the driver: trajectory mode writes one PDB per sample and per step through the
    asynchronous writer; the files carry the coordinates / sequences of the returned trajectory."""
    from abx_amd import design
    out = str(tmp_path / 'traj')
    files = design.main(['--workload', 'tiny', '--num_samples', '2', '--mode', 'trajectory', '--num_t', '3', '--output_dir', out])
    assert [os.path.basename(f) for f in files if f.endswith('.tsv')] == ['tiny_H_L_A_designs.tsv']
    names = sorted(os.path.basename(f) for f in files if f.endswith('.pdb'))
    assert len(names) == 6 and names[0] == 'tiny-000_H_L_A@0.0100.pdb' and names[-1] == 'tiny-001_H_L_A@1.0000.pdb'
    txt = open(os.path.join(out, names[0])).read().splitlines()
    assert txt[0].startswith('ATOM      1  N  ') and txt[-1] == 'END   '
    assert sum(ln.startswith('TER') for ln in txt) == 2          # heavy + light chain (synthetic complex: no antigen records)


def _cpu_copy(b, sl=slice(None)):
    out = {}
    for k, v in b.items():
        if k.startswith('_'):
            continue
        if torch.is_tensor(v):
            out[k] = (v[sl] if v.dim() > 0 else v).cpu()
        elif isinstance(v, tuple):
            out[k] = tuple(x[sl].cpu() for x in v)
        else:
            out[k] = v
    return out


class _GemmSpy:
    """Counts the abx_gemm calls whose A operand is a f16-image tensor (the triangle-multiplication contraction on the
    split-f16 kernels) and those that use the padded pair-row maps."""

    def __enter__(self):
        from abx_amd import ops
        self.ops, self.orig, self.orig_blk, self.plane, self.padded = ops, ops.gemm, ops.tri_mul_fwd, 0, 0

        def spy(A, B, C, **kw):
            self.plane += int(A.dtype == torch.int16)
            self.padded += int(kw.get('pair') is not None)
            return self.orig(A, B, C, **kw)

        def spy_blk(*a, **kw):          # the op-group entry point abx_tri_mul_fwd IS the image -> plane contraction route (one per tri-mul)
            self.plane += 1
            return self.orig_blk(*a, **kw)
        ops.gemm, ops.tri_mul_fwd = spy, spy_blk
        return self

    def __exit__(self, *exc):
        self.ops.gemm, self.ops.tri_mul_fwd = self.orig, self.orig_blk


@pytest.mark.parametrize('w,B', [(dict(L_heavy=55, L_light=47, L_antigen=29, cdr=(30, 41)), 4),      # L = 131 (odd)
                                 (dict(L_heavy=50, L_light=44, L_antigen=24, cdr=(30, 39)), 4),      # L = 118 (L % 4 == 2)
                                 # L = 402 > 384: the 4-slot triangle-attention instantiation (4 query tiles per wave, 4 key
                                 # chunks), 7 key tasks per head and 34 query blocks in the IPA weights kernel
                                 (dict(L_heavy=126, L_light=110, L_antigen=166, cdr=(100, 112)), 1),
                                 # L = 65: the first length of the split-f16 arithmetic class, single partial tiles everywhere
                                 (dict(L_heavy=30, L_light=25, L_antigen=10, cdr=(15, 22)), 4),
                                 (dict(L_heavy=80, L_light=70, L_antigen=41, cdr=(50, 61)), 2)])         # L = 191
def test_any_length_takes_the_plane_path_vs_oracle(gpu_model, params, cfg, oracle_diffuser, w, B):
    """residue counts that are not multiples of 4 (the real complexes are L = 230 and 261) run the triangle
    multiplication on the same glu -> f16 operand images -> plane contraction route as L = 352, through the padded pair-row maps.
    One full call (3 passes), 4 samples with different noise and a masked antigen tail, HIP vs oracle."""
    from oracle import abx_oracle as O
    from abx_amd import sampler, ops
    model, D = gpu_model
    L = w['L_heavy'] + w['L_light'] + w['L_antigen']
    assert L % 4 != 0 and ops.gemm_mode(L) == 2
    b = _synthetic_batch(D, w, B=B, n_masked_tail=2)
    t_ = torch.full((B,), 0.4040404040404041, dtype=torch.float64, device=DEV)
    b = sampler.set_t_feats(b, D, t_, torch.ones(B, device=DEV))
    cpu = _cpu_copy(b)
    model.max_chunk = None
    # which kernels run is visible on the descriptor-level path (the op-group entry points issue the same launches from C:
    # test_op_group_entry_points_equal_the_descriptor_level_path); the values below come from the default path
    eng = model._get_engine(torch.device(DEV))
    eng.block_api = False
    try:
        with _GemmSpy() as spy:
            ret0 = model({k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()})
            torch.cuda.synchronize()
            pair0 = ret0['representations']['pair'].clone()
    finally:
        eng.block_api = True
    assert spy.plane == 6 and spy.padded == 12, (spy.plane, spy.padded)     # 2 tri-muls x 3 passes: contraction; glu + proj_out
    ret = model(b)
    torch.cuda.synchronize()
    assert torch.equal(ret['representations']['pair'], pair0)
    ref = O.score_network(params, cpu, cfg, oracle_diffuser)
    f, fr = ret['heads']['folding'], ref['heads']['folding']
    assert torch.equal(ret['heads']['sequence_module']['seq_0'].cpu(), ref['heads']['sequence_module']['seq_0'])
    close(ret['representations']['pair'], ref['representations']['pair'], 3e-4, 1e-4, 'pair')
    close(f['rigids'], fr['rigids'], 1e-4, 1e-4, 'rigids')
    close(f['final_atom14_positions'], fr['final_atom14_positions'], 1e-3, 1e-4, 'atom14')
    close(ret['heads']['sequence_module']['logits'], ref['heads']['sequence_module']['logits'], 3e-4, 1e-4, 'logits')
    close(f['trans_score'], fr['trans_score'], 3e-4, 1e-4, 'trans_score')


def test_complex_of_exactly_64_residues_vs_oracle(gpu_model, params, cfg, oracle_diffuser):
    """L = 64 is the first length of the split-f16 arithmetic class (ops.gemm_mode), and its tri-mul contraction is the one plane x plane
    product with N = 64: the dispatch of csrc/gemm3.hip used to turn every N <= 64 away to the exact kernel, which a product of operand
    images cannot take, and a network call on such a complex failed.  One full call, 2 samples with a masked tail, HIP vs oracle."""
    from oracle import abx_oracle as O
    from abx_amd import sampler, ops
    model, D = gpu_model
    w, B = dict(L_heavy=28, L_light=24, L_antigen=12, cdr=(16, 23)), 2
    assert w['L_heavy'] + w['L_light'] + w['L_antigen'] == 64 and ops.gemm_mode(64) == 2
    b = _synthetic_batch(D, w, B=B, n_masked_tail=2)
    t_ = torch.full((B,), 0.4040404040404041, dtype=torch.float64, device=DEV)
    b = sampler.set_t_feats(b, D, t_, torch.ones(B, device=DEV))
    cpu = _cpu_copy(b)
    model.max_chunk = None
    ret = model(b)
    torch.cuda.synchronize()
    ref = O.score_network(params, cpu, cfg, oracle_diffuser)
    f, fr = ret['heads']['folding'], ref['heads']['folding']
    assert torch.equal(ret['heads']['sequence_module']['seq_0'].cpu(), ref['heads']['sequence_module']['seq_0'])
    close(ret['representations']['pair'], ref['representations']['pair'], 3e-4, 1e-4, 'pair')
    close(f['rigids'], fr['rigids'], 1e-4, 1e-4, 'rigids')
    close(f['final_atom14_positions'], fr['final_atom14_positions'], 1e-3, 1e-4, 'atom14')
    close(ret['heads']['sequence_module']['logits'], ref['heads']['sequence_module']['logits'], 3e-4, 1e-4, 'logits')


@pytest.mark.parametrize('name,B,chunk', [('6ct7like', 100, 40), ('6qd7like', 32, 32)])
def test_real_complex_lengths_full_batch(gpu_model, params, cfg, oracle_diffuser, name, B, chunk):
    """BASELINE configs 2 and 5 at their real (cropped) lengths, L = 230 x 100 samples and L = 261 x 32 samples of one complex:
    the whole batch on the plane path; sample 0 of the batch against the oracle (values, not only properties); results
    independent of the chunking of the batch."""
    from oracle import abx_oracle as O
    from abx_amd import sampler
    model, D = gpu_model
    b = _synthetic_batch(D, name, B=B)
    b['_shared_context'] = True
    L = b['seq'].shape[1]
    assert L in (230, 261)
    t_ = torch.full((B,), 0.7070707070707071, dtype=torch.float64, device=DEV)
    b = sampler.set_t_feats(b, D, t_, torch.ones(B, device=DEV))
    cpu = _cpu_copy(b, slice(0, 1))

    def run(ch):
        bb = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}
        model.max_chunk = ch
        with _GemmSpy() as spy:
            r = model(bb)
            torch.cuda.synchronize()
        assert spy.plane == 6 * -(-B // ch)
        return {'rigids': r['heads']['folding']['rigids'].clone(), 'logits': r['heads']['sequence_module']['logits'].clone(),
                'seq_0': r['heads']['sequence_module']['seq_0'].clone(), 'atom14': r['heads']['folding']['final_atom14_positions'].clone(),
                'trans_score': r['heads']['folding']['trans_score'].clone(), 'pLDDT': r['heads']['predicted_lddt']['pLDDT'].clone()}

    a = run(B)
    for k, v in a.items():
        assert torch.isfinite(v.double()).all(), k
    c = run(chunk)
    for k in a:
        assert torch.equal(a[k], c[k]), f'chunking changed {k}'
    model.max_chunk = None
    ref = O.score_network(params, cpu, cfg, oracle_diffuser)
    fr = ref['heads']['folding']
    assert torch.equal(a['seq_0'][:1].cpu(), ref['heads']['sequence_module']['seq_0'])
    close(a['rigids'][:1], fr['rigids'], 1e-4, 1e-4, 'rigids')
    close(a['atom14'][:1], fr['final_atom14_positions'], 1e-3, 1e-4, 'atom14')
    close(a['logits'][:1], ref['heads']['sequence_module']['logits'], 3e-4, 1e-4, 'logits')
    close(a['trans_score'][:1], fr['trans_score'], 3e-4, 1e-4, 'trans_score')
    close(a['pLDDT'][:1], ref['heads']['predicted_lddt']['pLDDT'], 5e-3, 1e-4, 'pLDDT')


def test_trajectory_mode_real_length(gpu_model, cfg):
    """BASELINE config 5 shape (L = 261, trajectory mode, device Philox noise): every grid point is recorded, tokens stay in
    range, fixed residues never move, and the run is reproducible for the same (seed, sample ids)."""
    from abx_amd import sampler
    model, D = gpu_model
    B = 8
    b = _synthetic_batch(D, '6qd7like', B=B)
    b['_shared_context'] = True
    sid = torch.arange(B, device=DEV) + 40
    D.seed = 17
    model.max_chunk = None
    t1 = sampler.sample_fn(b, cfg, D, model, mode='trajectory', num_t=4, sample_ids=sid)
    D.seed = 17
    t2 = sampler.sample_fn(b, cfg, D, model, mode='trajectory', num_t=4, sample_ids=sid)
    assert len(t1) == 4 and [r['time'] for r in t1] == pytest.approx([1.0, 0.67, 0.34, 0.01])
    fixed = b['fixed_mask'].bool()
    for r1, r2 in zip(t1, t2):
        assert torch.isfinite(r1['rigids_t'].double()).all() and torch.isfinite(r1['atom14_results']).all()
        assert int(r1['seq'].min()) >= 0 and int(r1['seq'].max()) <= 19
        assert torch.equal(r1['seq'], r2['seq']) and torch.equal(r1['rigids_t'], r2['rigids_t'])
    for r1 in t1[:-1]:          # reverse() keeps fixed residues (the last record takes the model's own frames)
        assert torch.equal(r1['seq_t'][fixed], b['seq_t'][fixed])
        assert (r1['rigids_t'][..., 4:][fixed].double() - b['rigids_t'][..., 4:][fixed].double()).abs().max() < 1e-4
    assert int((~fixed).sum()) == 13 * B


def _check_call_gpu(ret, m, fixed, pair_key, S, tol_scale=1.0):
    f = ret['heads']['folding']
    assert torch.equal(ret['heads']['sequence_module']['seq_0'].cpu(), tt(m['out.seq_0']))
    close(f['rigids'], m['out.rigids'], 1e-4 * tol_scale, 1e-4, 'rigids')                   # north_star: 1e-4 on frames
    close(f['final_atom14_positions'], m['out.atom14'], 5e-4 * tol_scale, 1e-5, 'atom14')
    close(ret['heads']['sequence_module']['logits'], m['out.logits'], 2e-4 * tol_scale, 1e-5, 'logits')
    close(ret['heads']['predicted_lddt']['pLDDT'], m['out.pLDDT'], 2e-3 * tol_scale, 1e-5, 'pLDDT')
    close(f['trans_score'], m['out.trans_score'], 2e-4 * tol_scale, 1e-5, 'trans_score')
    close(ret['representations']['seq'], m['out.seq'], 2e-4 * tol_scale, 1e-5, 'trunk seq')
    pr = ret['representations']['pair']
    close(pr[:, ::S, ::S], m[pair_key], 3e-4 * tol_scale, 2e-5, 'trunk pair (sub-grid)')
    assert abs(float(pr.double().sum()) - float(m['out.pair.sum'])) <= 2e-5 * float(m['out.pair.abssum']), 'trunk pair sum'
    rs, ref = f['rot_score'].cpu().numpy(), m['out.rot_score']
    dif = (fixed.cpu().numpy() == 0).reshape(-1)
    bad = (np.abs(rs - ref) > 2e-4 + 1e-4 * np.abs(ref)).reshape(-1, 3).any(axis=1)[dif].mean()
    assert bad <= 0.1, f'rot_score bucket mismatches {bad}'


def test_full_call_matches_reference_golden_L48(gpu_model, cfg):
    """One in-loop call at L = 48 with a 3-residue padded antigen tail, from a zero self-conditioning state: HIP path vs the
    reference's own outputs (tests/golden/make_golden_sizes.py)."""
    model, D = gpu_model
    m = load_npz('modules_L48.npz')
    b = feat_batch_from_golden(m)
    for k in ('seq_t', 'rigids_t', 't', 'rot_score_scaling', 'trans_score_scaling'):
        b[k] = tt(m['in.' + k])
    b = to_dev(b)
    model.max_chunk = None
    ret = model(b)
    torch.cuda.synchronize()
    assert torch.equal(b['seq_t'].cpu(), tt(m['final.seq_t_after']))
    _check_call_gpu(ret, m, b['fixed_mask'], 'out.pair', int(m['sub']))
    from abx_amd.model.abx import get_prev
    assert (get_prev(b, ret, cfg.model)['prev_pos'].cpu().numpy() != m['out.prev_pos']).mean() < 1e-3


@pytest.mark.parametrize('name', ['L256', 'L352'])
def test_large_shape_digest_vs_reference(gpu_model, cfg, name):
    """the HIP path against outputs of the REFERENCE ITSELF at the benchmark's sizes (the bench's synthetic
    complexes, B = 1, one in-loop call = 3 passes on the split-f16 kernels)."""
    from abx_amd import features
    from conftest import digest_batch
    model, D = gpu_model
    g = load_npz(f'{name}_digest.npz')
    b, _ = digest_batch(g, name, D, features.build_features, device=DEV)
    model.max_chunk = None
    ret = model(b)
    torch.cuda.synchronize()
    assert torch.equal(b['seq_t'].cpu(), tt(g['final.seq_t_after']))
    _check_call_gpu(ret, g, b['fixed_mask'], 'out.pair_sub', int(g['pair_sub']))
    from abx_amd.model.abx import get_prev
    assert (get_prev(b, ret, cfg.model)['prev_pos'].cpu().numpy() != g['out.prev_pos']).mean() < 1e-4


def test_design_driver_on_the_shipped_pdb(tmp_path):
    """BASELINE configs 1 / 2 / 5 on real coordinates: `design --pdb_file` reads the reference's 6ct7 example
    (chains H, L + antigen S), samples 3 designs of CDR-H3 and writes PDB files that contain the antibody (designed H3, fixed
    framework at its input coordinates up to the rigid-frame rebuild) and the antigen chain."""
    from abx_amd import design
    from abx_amd.io.pdb_reader import read_pdb, chain_feature
    from conftest import GOLDEN
    src = os.path.join(GOLDEN, 'pdb', '6ct7_H_L_S.pdb')
    out = str(tmp_path / 'd6ct7')
    files = design.main(['--pdb_file', src, '--num_samples', '3', '--mode', 'design', '--num_t', '3', '--output_dir', out])
    tsv = [f for f in files if f.endswith('.tsv')]
    files = [f for f in files if f.endswith('.pdb')]
    assert sorted(os.path.basename(f) for f in files) == [f'6ct7-{i:03d}_H_L_S.pdb' for i in range(3)]
    rows = [ln.split('\t') for ln in open(tsv[0]).read().splitlines()[1:]]
    assert [r[0] for r in rows] == ['0', '1', '2'] and all(len(r[2]) == 113 + 108 for r in rows)
    ref = read_pdb(src)
    ref_h = chain_feature(ref['H'])['str_seq'][:113]
    for f in files:
        ch = read_pdb(f)
        assert list(ch) == ['H', 'L', 'S']
        h, l, s = (chain_feature(ch[c]) for c in 'HLS')
        assert len(h['str_seq']) == 113 and len(l['str_seq']) == 108 and s['str_seq'] == 'MDVFMKGLSK'
        # only the diffused window (3 residues of CDR-H3 = TSAH) may change
        diff = [i for i in range(113) if h['str_seq'][i] != ref_h[i]]
        assert all(98 <= i <= 100 for i in diff), diff
        assert np.isfinite(h['coords']).all() and float(np.abs(h['coords']).max()) < 500


def test_inference_style_driver_on_npz_entries(tmp_path):
    """VERDICT r2 missing #3: the command line of the reference's inference.py (--name_idx --data_dir --model_features --gpu_list
    --batch_size, inference.py:398-416) on the two shipped complexes as make_pdb_npz entries: the output layout of inference.py
    (<mode>/reference/<name>.pdb = ground truth with pLDDT 100, <mode>/<k:04d>/<name>.pdb per sample), optimize mode looping over the
    optimize_steps of the feature JSON (OPT-<step>/...), BASELINE configs 3 / 4 in miniature."""
    import json
    from abx_amd import design
    from abx_amd.io.pdb_reader import read_pdb, chain_feature
    from conftest import GOLDEN
    idx = tmp_path / 'test.idx'
    idx.write_text('6ct7_H_L_S\n6qd7_X_Z_F|E\n')
    feats = tmp_path / 'feats.json'
    json.dump([["make_to_device", {"fields": ["seq"], "device": "%(device)s"}], ["make_diffuser_features", {"generate_area": "H3", "optimize_steps": [3, 5]}]],
              open(feats, 'w'))
    common = ['--name_idx', str(idx), '--data_dir', os.path.join(GOLDEN, 'npz'), '--model_features', str(feats), '--gpu_list', '0', '--batch_size', '1',
              '--num_samples', '2']
    out = str(tmp_path / 'inf')
    files = design.main(common + ['--mode', 'design', '--num_t', '3', '--output_dir', out])
    rel = sorted(os.path.relpath(f, out) for f in files if f.endswith('.pdb'))
    assert rel == sorted([f'design/{d}/{n}.pdb' for d in ('reference', '0000', '0001') for n in ('6ct7_H_L_S', '6qd7_X_Z_F|E')])
    ref = chain_feature(read_pdb(os.path.join(out, 'design/reference/6ct7_H_L_S.pdb'))['H'])
    src = chain_feature(read_pdb(os.path.join(GOLDEN, 'pdb', '6ct7_H_L_S.pdb'))['H'])
    assert ref['str_seq'] == src['str_seq'][:113]                                    # the reference batch is the ground truth
    d0 = chain_feature(read_pdb(os.path.join(out, 'design/0000/6ct7_H_L_S.pdb'))['H'])
    assert [i for i in range(113) if d0['str_seq'][i] != ref['str_seq'][i]] == [] or all(98 <= i <= 100 for i in range(113) if d0['str_seq'][i] != ref['str_seq'][i])
    # optimize mode: one tree per optimize step of the feature JSON
    out2 = str(tmp_path / 'opt')
    files = design.main(common[:2] + ['--data_dir', os.path.join(GOLDEN, 'npz'), '--model_features', str(feats), '--num_samples', '1', '--mode', 'optimize',
                                      '--output_dir', out2])
    rel = sorted(os.path.relpath(f, out2) for f in files if f.endswith('.pdb'))
    # inference.py:321-322: the ground truth goes to <output_dir>/optimize/reference/ (ref_dir is built from output_dir, not from the
    # OPT-<step> directory), the samples of a step to optimize/OPT-<step>/<k:04d>/
    names2 = ('6ct7_H_L_S', '6qd7_X_Z_F|E')
    assert rel == sorted([f'optimize/reference/{n}.pdb' for n in names2] + [f'optimize/OPT-{st}/0000/{n}.pdb' for st in (3, 5) for n in names2])


def test_guidance_off_is_bit_identical_and_on_follows_the_formula(gpu_model, cfg):
    """Row G driver semantics: guidance=None executes the un-guided sampler (bit-identical to a run without the argument); with a
    ViolationGuidance the scores handed to reverse() are the model's scores minus the scaled frame gradients on diffused residues,
    and fixed residues stay where they are."""
    from abx_amd import sampler
    from abx_amd.guidance import ViolationGuidance, quat_to_rot
    model, D = gpu_model
    B = 3
    b = _synthetic_batch(D, dict(L_heavy=30, L_light=26, L_antigen=16, cdr=(20, 27)), B=B)
    b['_shared_context'] = True
    sid = torch.arange(B, device=DEV)
    D.seed = 3
    t_plain = sampler.sample_fn(b, cfg, D, model, mode='trajectory', num_t=3, sample_ids=sid)
    D.seed = 3
    t_none = sampler.sample_fn(b, cfg, D, model, mode='trajectory', num_t=3, sample_ids=sid, guidance=None)
    for r1, r2 in zip(t_plain, t_none):
        assert torch.equal(r1['rigids_t'], r2['rigids_t']) and torch.equal(r1['seq'], r2['seq']) and torch.equal(r1['atom14_results'], r2['atom14_results'])
    seen = []

    class Spy(ViolationGuidance):
        def __call__(self, batch, out, rot_score, trans_score, diffuse_mask):
            rot, trans = super().__call__(batch, out, rot_score, trans_score, diffuse_mask)
            e, _, g_t, g_r = self.energy_and_grads(batch, out)
            R = quat_to_rot(out['heads']['folding']['rigids'][..., :4])
            m = diffuse_mask.float()[..., None]
            exp_t = trans_score - (self.scale_trans / 0.1) * g_t * m
            exp_r = rot_score - self.scale_rot * torch.einsum('...ji,...j->...i', R, g_r) * m
            seen.append((float((trans - exp_t).abs().max()), float((rot - exp_r).abs().max()), float(e.sum()),
                         float((trans - trans_score).abs().max())))
            return rot, trans

    D.seed = 3
    t_g = sampler.sample_fn(b, cfg, D, model, mode='trajectory', num_t=3, sample_ids=sid, guidance=Spy(scale_trans=0.02, scale_rot=0.02))
    assert len(seen) == 2 and all(s[0] < 1e-9 and s[1] < 1e-5 for s in seen)
    assert seen[0][2] > 0 and seen[0][3] > 0                                   # random weights: the prediction does violate; guidance acts
    assert not torch.equal(t_g[0]['rigids_t'], t_plain[0]['rigids_t'])
    fixed = b['fixed_mask'].bool()
    assert torch.equal(t_g[0]['rigids_t'][fixed], t_plain[0]['rigids_t'][fixed])   # mask merge: fixed residues untouched
    assert torch.isfinite(t_g[-1]['rigids_t']).all()


def test_esm_hook_matches_reference_golden(esm_setup, oracle_diffuser):
    """ESM2 embedding hook on the HIP path (8f-3) against the reference run with esm.enabled (ESM module = seeded stand-in tensor):
    fixed tensor through batch['esm_embed'] and through an esm_provider callable; a reference-style checkpoint that also carries
    the ESM2 weights loads with strict=True."""
    from conftest import esm_tensor
    from abx_amd.model.abx import ScoreNetwork
    from abx_amd.diffuser.full_diffuser import FullDiffuser
    cfg, params = esm_setup
    gi = load_npz('igso3_small.npz')
    so3 = oracle_diffuser.so3
    D = FullDiffuser(cfg.diffuser)
    D.set_tables(so3._pdf, so3._cdf, so3._score_norms, DEV)
    model = ScoreNetwork(cfg.model, D)
    ckpt = dict(params)
    ckpt['impl.seqformer.encode_esm_emb.model.embed_tokens.weight'] = torch.zeros(33, 8)      # belongs to the external provider
    model.load_state_dict(ckpt, strict=True)
    model = model.to(DEV).eval()
    g = load_npz('esm_tiny.npz')

    def batch():
        b = feat_batch_from_golden(load_npz('feat_tiny.npz'))
        for k in ('seq_t', 'rigids_t', 't', 'rot_score_scaling', 'trans_score_scaling'):
            b[k] = tt(g['in.' + k])
        return to_dev(b)

    b = batch()
    E = esm_tensor(g, b['seq'].shape[0], b['anchor_flag'].shape[1]).to(DEV)
    with pytest.raises(RuntimeError):
        model(batch())                                   # esm.enabled without an embedding source fails loudly
    b['esm_embed'] = E
    ret = model(b)
    torch.cuda.synchronize()
    f = ret['heads']['folding']
    assert torch.equal(ret['heads']['sequence_module']['seq_0'].cpu(), tt(g['out.seq_0']))
    close(ret['representations']['seq'], g['out.seq'], 2e-4, 1e-5, 'trunk seq')
    close(ret['representations']['pair'], g['out.pair'], 2e-4, 1e-5, 'trunk pair')
    close(f['rigids'], g['out.rigids'], 1e-4, 1e-4, 'rigids')
    close(ret['heads']['sequence_module']['logits'], g['out.logits'], 2e-4, 1e-5, 'logits')
    close(f['final_atom14_positions'], g['out.atom14'], 5e-4, 1e-5, 'atom14')
    rig = f['rigids'].clone()
    calls = []
    model.esm_provider = lambda bb: (calls.append(bb['seq_t'].clone()), E)[1]
    ret2 = model(batch())
    assert len(calls) == 3 and torch.equal(ret2['heads']['folding']['rigids'], rig)      # once per pass (seq_t changes with the recycles)


@pytest.mark.parametrize('w,B', [(dict(L_heavy=10, L_light=6, L_antigen=4, cdr=(4, 8)), 3), (dict(L_heavy=46, L_light=40, L_antigen=26, cdr=(28, 36)), 2)])
def test_graph_replay_equals_eager(gpu_model, cfg, w, B):
    """hipGraph capture of the step (abx_amd.graph.GraphedSteps): one eager step, two captured graphs (even / odd steps: the
    self-conditioning buffers ping-pong), replays afterwards.  A 7-point trajectory with the device Philox noise is
    bit-identical to the eager loop, record by record."""
    from abx_amd import sampler
    model, D = gpu_model
    b = _synthetic_batch(D, w, B=B)
    b['_shared_context'] = True
    sid = torch.arange(B, device=DEV) + 5
    model.max_chunk = None
    D.seed = 21
    eager = sampler.sample_fn(b, cfg, D, model, mode='trajectory', num_t=7, sample_ids=sid)
    D.seed = 21
    graphed = sampler.sample_fn(b, cfg, D, model, mode='trajectory', num_t=7, sample_ids=sid, use_graph=True)
    assert len(eager) == len(graphed) == 7
    for k, (e, g) in enumerate(zip(eager, graphed)):
        assert torch.equal(e['seq'], g['seq']), f'step {k} tokens'
        assert torch.equal(e['rigids_t'].double(), g['rigids_t'].double()), f'step {k} rigids'
        assert torch.equal(e['atom14_results'], g['atom14_results']) and torch.equal(e['pLDDT'], g['pLDDT']), f'step {k} outputs'


def test_graph_replay_with_guidance_equals_eager(gpu_model, cfg):
    """the guided step inside hipGraph capture (no host-to-device copy, no allocation of host data on the step path):
    bit-identical to the eager guided loop."""
    from abx_amd import sampler
    from abx_amd.guidance import ViolationGuidance
    model, D = gpu_model
    B = 2
    b = _synthetic_batch(D, dict(L_heavy=30, L_light=26, L_antigen=16, cdr=(20, 27)), B=B)
    b['_shared_context'] = True
    sid = torch.arange(B, device=DEV) + 2
    runs = []
    for use_graph in (False, True):
        D.seed = 8
        runs.append(sampler.sample_fn(b, cfg, D, model, mode='trajectory', num_t=6, sample_ids=sid, use_graph=use_graph,
                                      guidance=ViolationGuidance(scale_trans=0.02, scale_rot=0.02)))
    D.seed = 8
    plain = sampler.sample_fn(b, cfg, D, model, mode='trajectory', num_t=6, sample_ids=sid)
    for k, (e, g) in enumerate(zip(*runs)):
        assert torch.equal(e['seq'], g['seq']) and torch.equal(e['rigids_t'].double(), g['rigids_t'].double()), f'step {k}'
        assert torch.equal(e['atom14_results'], g['atom14_results'])
    assert not torch.equal(runs[0][1]['rigids_t'], plain[1]['rigids_t'])             # and the guidance did act


def _reference_style_loop(data_init, config, diffuser, model, mode, num_t, min_t=0.01):
    """The CALL PATTERN of the reference's sample_fn (inference.py:180-273), written against the drop-in import paths: what a user who
    switches packages executes.  deepcopy of the batch, dt as a 0-dim device tensor, t from a NumPy float64, diffuser.reverse with
    the reference's keyword set only, per-step .to('cpu') of the outputs."""
    import copy
    from abx.model.abx import get_prev
    batch = copy.deepcopy(data_init)
    device = batch['rigids_t'].device
    bb_mask = batch['atom14_gt_exists'][..., 0]
    diffuse_mask = (1 - batch['fixed_mask']) * bb_mask
    Lab = batch['anchor_flag'].shape[1]
    n = batch['rigids_t'].shape[0]
    t_placeholder = torch.ones(n, device=device, dtype=torch.float32)
    grid = np.linspace(min_t, 1.0, num_t)[::-1]
    dt = torch.tensor(1 / num_t, device=device)
    if mode == 'optimize':
        opt_step = batch['t'][0].cpu().numpy()
        if opt_step < 1.0:
            grid = grid[grid <= opt_step + 1e-8]

    def set_t(feats, t):
        feats['t'] = t * t_placeholder
        rs, ts = diffuser.score_scaling(feats['t'])
        feats['rot_score_scaling'] = rs * t_placeholder
        feats['trans_score_scaling'] = ts * t_placeholder
        return feats

    traj = []
    with torch.no_grad():
        batch = set_t(batch, grid[0])
        batch.update(get_prev(batch, model(batch), config.model))
        for t in grid:
            if t > min_t:
                t_ = torch.tile(torch.tensor(t, device=device), (n,))
                batch = set_t(batch, t_)
                out = model(batch)
                batch.update(get_prev(batch, out, config.model))
                rigids_t, seq_t = diffuser.reverse(
                    rigid_t=batch['rigids_t'], seq_t=batch['seq_t'], rot_score=out['heads']['folding']['rot_score'],
                    trans_score=out['heads']['folding']['trans_score'], logits_t=out['heads']['sequence_module']['logits'],
                    diffuse_mask=diffuse_mask, t=t_, dt=dt, center=True, noise_scale=1.0)
            else:
                out = model(batch)
                rigids_t, seq_t = out['heads']['folding']['rigids'], out['heads']['sequence_module']['seq_0']
            batch['rigids_t'], batch['seq_t'] = rigids_t, seq_t
            pl = out['heads']['predicted_lddt']['pLDDT']
            pl = torch.sum(pl * diffuse_mask, dim=1) / torch.sum(diffuse_mask, dim=1)
            traj.append({'seq': torch.clamp(seq_t[:, :Lab], min=0, max=19).long().to('cpu').numpy(),
                         'atom14_results': out['heads']['folding']['final_atom14_positions'][:, :Lab].to('cpu').numpy(),
                         'pLDDT': torch.tile(pl[:, None], (1, Lab)).to('cpu').numpy(), 'time': t,
                         'rigids_t': rigids_t.to('cpu').numpy()})
    return traj if mode == 'trajectory' else traj[-1:]


def test_reference_call_pattern_through_the_alias_packages(params, cfg, gpu_model, tmp_path, monkeypatch):
    """VERDICT r2 weak #7a / INTEGRATION.md section A: `abx.model.abx` / `diffuser.full_diffuser` driven exactly the way the reference's
    own loop drives them (see _reference_style_loop): singleton FullDiffuser.get(conf) that loads its IGSO(3) tables from the .npy
    cache, no extension keyword anywhere; the recorded noise of traj_tiny.npz / optimize_tiny.npz reaches the kernel through a
    monkey-patched reverse() only.  Tokens exact at every step, frames / atoms at the tolerance of the sampler tests."""
    import copy
    import abx.model.abx as ref_abx
    import diffuser.full_diffuser as ref_fd
    _, pinned = gpu_model
    dc = copy.deepcopy(cfg.diffuser)
    dc.so3.cache_dir = str(tmp_path / 'cache') + '/'
    monkeypatch.delitem(ref_fd.diffuser_obj_dict, 'diffuser', raising=False)      # a fresh process-wide singleton for this test
    D = ref_fd.FullDiffuser.get(dc)
    assert ref_fd.FullDiffuser.get(dc) is D                                          # the reference's process-wide singleton
    os.makedirs(D._cache_path(), exist_ok=True)                                      # so3_diffuser.py:131-174 cache contract
    for name, tab in (('pdf_vals.npy', pinned._pdf), ('cdf_vals.npy', pinned._cdf), ('score_norms.npy', pinned.score_norms)):
        np.save(os.path.join(D._cache_path(), name), tab.cpu().numpy())
    model = ref_abx.ScoreNetwork(model_conf=cfg.model, diffuser=D)
    model.load_state_dict(params, strict=True)
    model = model.to(DEV).eval()
    orig_reverse = ref_fd.FullDiffuser.reverse
    for fixture, mode, feat in (('traj_tiny.npz', 'trajectory', 'feat_tiny.npz'), ('optimize_tiny.npz', 'optimize', None)):
        tj = load_npz(fixture)
        if feat is not None:
            b = to_dev(feat_batch_from_golden(load_npz(feat)))
            num_t = 4
        else:
            b = feat_batch_from_golden(load_npz('feat_tiny.npz'))
            for k in ('rigids_t', 'seq_t', 't', 'fixed_mask', 'rigids_0'):
                b[k] = tt(tj['feat.' + k])
            b = to_dev(b)
            num_t = 100
        calls = []

        def patched(self, *a, **kw):
            assert not a and set(kw) == {'rigid_t', 'seq_t', 'rot_score', 'trans_score', 'logits_t', 'diffuse_mask', 't', 'dt', 'center', 'noise_scale'}
            k = len(calls)
            calls.append(k)
            return orig_reverse(self, noise=dict(z_rot=tt(tj[f'n{k}.z_rot']).to(DEV), z_trans=tt(tj[f'n{k}.z_trans']).to(DEV),
                                                 jumps=tt(tj[f'n{k}.jumps']).to(DEV)), **kw)

        monkeypatch.setattr(ref_fd.FullDiffuser, 'reverse', patched)
        traj = _reference_style_loop(b, cfg, D, model, mode, num_t)
        monkeypatch.setattr(ref_fd.FullDiffuser, 'reverse', orig_reverse)
        if mode == 'trajectory':
            assert len(traj) == 4 and len(calls) == 3
            for k, d in enumerate(traj):
                assert float(d['time']) == float(tj[f'k{k}.time'])
                assert np.array_equal(d['seq'], tj[f'k{k}.seq']), f'step {k}: tokens differ'
                close(d['atom14_results'], tj[f'k{k}.atom14'], 5e-3, 1e-4, f'step {k} atom14')
                close(d['pLDDT'], tj[f'k{k}.pLDDT'], 1e-2, 1e-4, f'step {k} pLDDT')
            close(traj[-1]['rigids_t'], tj['final.rigids_t'], 2e-3, 1e-4, 'final rigids')
        else:
            assert len(traj) == 1 and len(calls) == 3 and float(traj[0]['time']) == float(tj['last.time'])
            assert np.array_equal(traj[0]['seq'], tj['last.seq'])
            close(traj[0]['atom14_results'], tj['last.atom14'], 5e-3, 1e-4, 'optimize atom14')
            close(traj[0]['pLDDT'], tj['last.pLDDT'], 1e-2, 1e-4, 'optimize pLDDT')
            close(traj[0]['rigids_t'], tj['final.rigids_t'], 2e-3, 1e-4, 'optimize final rigids')


def test_design_driver_two_ranks_shard_the_samples(tmp_path):
    """BASELINE config 3 shape (a list of complexes on several ranks): `abx_amd.design` under torch.distributed.run with 2 ranks on the
    two shipped complexes, 3 samples each, in both multi-rank schemes: --shard_samples (every complex's samples sharded: rank 0 takes
    samples 0-1, rank 1 sample 2; one gather per complex) and the default SET-LEVEL schedule (--min_block 3: whole (complex, block)
    units dealt longest-first, 6qd7 to rank 0 and 6ct7 to rank 1; one gather of the designs table at the end of the set).  Every rank
    writes its own PDB files, rank 0 the designs tables.  Both ranks share cuda:0 here (gloo, --debug_one_gpu),
    which is plumbing only: two PROCESSES time-slicing one MI355X did not reproduce a solo run's last digits in 3 of 10 trials
    (any kernel, also the fp64 geometry ones; never with one process per GPU), so the files are compared
    for structure, and bit-for-bit placement invariance is asserted in-process by test_device_rng_sampling_is_shard_invariant."""
    import subprocess
    import sys
    from abx_amd import design
    from abx_amd.io.pdb_reader import read_pdb, chain_feature
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pdbs = os.path.join(root, 'tests', 'golden', 'pdb')
    lst = tmp_path / 'set.txt'
    lst.write_text('6ct7_H_L_S\n# the multi-antigen complex of config 5\n6qd7_X_Z_F|E.pdb\n')
    names = design.complex_list(None, str(lst), pdbs)
    assert all(os.path.exists(n) for n in names), names
    common = ['--pdb_list', str(lst), '--pdb_dir', pdbs, '--num_samples', '3', '--num_t', '3', '--mode', 'design']
    one = str(tmp_path / 'one')
    design.main(common + ['--output_dir', one])
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''), HSA_ENABLE_IPC_MODE_LEGACY='0')
    for tag, extra in (('shard', ['--shard_samples']), ('set', ['--min_block', '3'])):
        two = str(tmp_path / tag)
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
               '--master-port', '29541', '-m', 'abx_amd.design', '--debug_one_gpu'] + common + extra + ['--output_dir', two]
        r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert ('set-level schedule: 2 units' in r.stdout) == (tag == 'set'), r.stdout[-2000:]
        fa, fb = sorted(os.listdir(one)), sorted(os.listdir(two))
        assert fa == fb and len([f for f in fa if f.endswith('.pdb')]) == 3 * len(names), (tag, fa, fb)
        for f in fa:
            if f.endswith('.tsv'):
                ra, rb = ([ln.split('\t') for ln in open(os.path.join(d, f)).read().splitlines()] for d in (one, two))
                assert [x[0] for x in ra] == [x[0] for x in rb] == ['sample', '0', '1', '2'], tag
                assert [len(x[2]) for x in ra] == [len(x[2]) for x in rb], tag
            else:
                ca, cb_ = (read_pdb(os.path.join(d, f)) for d in (one, two))
                assert sorted(ca) == sorted(cb_), (tag, f)
                for ch in ca:
                    assert len(chain_feature(ca[ch])['str_seq']) == len(chain_feature(cb_[ch])['str_seq']), (tag, f, ch)


def test_rccl_collective_path_on_one_gpu(tmp_path):
    """The one collective of the path on real hardware before the 8-GPU run (the reference only initialises NCCL,
    inference.py:59-82): a 1-rank RCCL process group (`init_process_group('nccl', device_id=...)`), the padded all_gather of DEVICE
    tensors in sampler.gather_results / gather_rows, the barrier and the MAX all_reduce of bench.py, through torch.distributed.run.
    bench.py --force-collective reports rccl_ranks == 1 and the same result digest as the plain single-process run; the design driver
    under the launcher with --force_collective writes the same files as without (set-level schedule on the two shipped complexes)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''), HSA_ENABLE_IPC_MODE_LEGACY='0')
    launch = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr', '127.0.0.1', '--master-port', '29543']
    args = ['--gpus', '1', '--steps', '1', '--warmup', '0', '--samples', '4', '--workload', 'L256', '--no-cpu-baseline', '--no-op-profile']
    out = {}
    for tag, cmd in (('plain', [sys.executable, 'bench.py'] + args), ('rccl', launch + ['bench.py'] + args + ['--force-collective'])):
        r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, tag + r.stdout[-2000:] + r.stderr[-4000:]
        out[tag] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert out['rccl']['rccl_ranks'] == 1 and out['rccl']['gather_ms'] is not None and out['plain']['gather_ms'] is None
    assert out['rccl']['result_digest'] == out['plain']['result_digest'] and len(out['plain']['result_digest']) == 64
    # the design driver: --gpu_list 0 through the launcher, RCCL initialised, set-level gather through a 1-rank all_gather
    from conftest import GOLDEN
    idx = tmp_path / 'test.idx'
    idx.write_text('6ct7_H_L_S\n6qd7_X_Z_F|E\n')
    common = ['--name_idx', str(idx), '--data_dir', os.path.join(GOLDEN, 'npz'), '--gpu_list', '0', '--num_samples', '2', '--num_t', '3', '--mode', 'design',
              '--min_block', '1']
    trees = {}
    for tag, cmd in (('plain', [sys.executable, '-m', 'abx_amd.design'] + common), ('rccl', launch + ['-m', 'abx_amd.design'] + common + ['--force_collective'])):
        od = str(tmp_path / tag)
        r = subprocess.run(cmd + ['--output_dir', od], env=env, cwd=root, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, tag + r.stdout[-2000:] + r.stderr[-4000:]
        trees[tag] = {os.path.relpath(os.path.join(dp, f), od): open(os.path.join(dp, f), 'rb').read() for dp, _, fs in os.walk(od) for f in fs}
    assert 'set-level schedule' in r.stdout
    assert sorted(trees['plain']) == sorted(trees['rccl']) and len(trees['plain']) == 2 * 3 + 2
    assert trees['plain'] == trees['rccl'], [k for k in trees['plain'] if trees['plain'][k] != trees['rccl'][k]]


def test_configs_3_and_4_at_workload_shape_on_one_gpu(tmp_path):
    """BASELINE configs 3 / 4 at their per-complex workload (100 samples per complex) on the one GPU a test box has.
    Config 3 (inference.py:296-373 over a set): `design --name_idx` on the two shipped complexes x 100 samples with the SET-LEVEL schedule
    (50-sample work units, RCCL initialised through torch.distributed.run, the designs table through the all-gather) writes the same file
    tree - every PDB and TSV byte - as the sample-sharded scheme of a plain single process: a sample's trajectory does not depend on
    which unit, block size or gather carried it.  Config 4 (optimize_steps = 10, guidance on, 100 samples of 6ct7): all coordinates
    finite, only the diffused CDR-H3 window changes against the input, and the guided run differs from the un-guided one."""
    import subprocess
    import sys
    from abx_amd.io.pdb_reader import read_pdb, chain_feature
    from conftest import GOLDEN
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''), HSA_ENABLE_IPC_MODE_LEGACY='0')
    launch = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr', '127.0.0.1', '--master-port', '29547']
    idx = tmp_path / 'test.idx'
    idx.write_text('6ct7_H_L_S\n6qd7_X_Z_F|E\n')
    common = ['--name_idx', str(idx), '--data_dir', os.path.join(GOLDEN, 'npz'), '--gpu_list', '0', '--num_samples', '100', '--num_t', '8', '--mode', 'design']
    trees, outs = {}, {}
    for tag, cmd in (('set', launch + ['-m', 'abx_amd.design'] + common + ['--min_block', '50', '--force_collective']),
                     ('shard', [sys.executable, '-m', 'abx_amd.design'] + common + ['--shard_samples'])):
        od = str(tmp_path / tag)
        r = subprocess.run(cmd + ['--output_dir', od], env=env, cwd=root, capture_output=True, text=True, timeout=1800)
        assert r.returncode == 0, tag + r.stdout[-2000:] + r.stderr[-4000:]
        outs[tag] = r.stdout
        trees[tag] = {os.path.relpath(os.path.join(dp, f), od): open(os.path.join(dp, f), 'rb').read() for dp, _, fs in os.walk(od) for f in fs}
    assert 'set-level schedule: 4 units' in outs['set'], outs['set'][-1500:]
    assert sorted(trees['set']) == sorted(trees['shard']) and len(trees['set']) == 2 * 101 + 2
    assert trees['set'] == trees['shard'], [k for k in trees['set'] if trees['set'][k] != trees['shard'][k]][:5]
    tsvs = [k for k in trees['set'] if k.endswith('.tsv')]
    assert len(tsvs) == 2
    for k in tsvs:
        rows = trees['set'][k].decode().splitlines()
        assert len(rows) == 101 and [r.split('\t')[0] for r in rows[1:]] == [str(i) for i in range(100)]

    # ---- config 4: one complex of the set, optimize mode from t = 0.10 with the violation guidance
    from abx_amd import design
    src = os.path.join(GOLDEN, 'pdb', '6ct7_H_L_S.pdb')
    ref_h = chain_feature(read_pdb(src)['H'])
    coords = {}
    for tag, extra in (('guided', ['--guidance']), ('plain', [])):
        out = str(tmp_path / ('opt_' + tag))
        files = [f for f in design.main(['--pdb_file', src, '--num_samples', '100', '--mode', 'optimize', '--optimize_steps', '10', '--output_dir', out] + extra)
                 if f.endswith('.pdb')]
        assert len(files) == 100
        hs = []
        for f in files[::9]:
            ch = read_pdb(f)
            h = chain_feature(ch['H'])
            assert list(ch) == ['H', 'L', 'S'] and len(h['str_seq']) == 113
            assert np.isfinite(h['coords']).all() and float(np.abs(h['coords']).max()) < 500
            diff = [i for i in range(113) if h['str_seq'][i] != ref_h['str_seq'][i]]
            assert all(98 <= i <= 100 for i in diff), diff                    # only the diffused window of CDR-H3 may change
            hs.append(h['coords'][:113, :4].copy())
        coords[tag] = np.stack(hs)
    fixed = [i for i in range(113) if not 98 <= i <= 100]
    # fixed residues stay where they are: the same backbone in every sample, with and without guidance (3 decimals of a PDB file)
    for tag in coords:
        assert float(np.nanmax(np.abs(coords[tag][:, fixed] - coords['plain'][:1, fixed]))) < 2.1e-3, tag
    coords = {k: v[:, 98:101] for k, v in coords.items()}
    assert np.abs(coords['guided'] - coords['plain']).max() > 1e-3, 'the guidance changed nothing on the diffused residues'


def test_results_do_not_depend_on_stale_lds(gpu_model, cfg):
    """No kernel may read LDS it has not written: one ScoreNetwork call (L = 112: split-f16 GEMMs, plane contraction, both
    attentions, IPA) is repeated with the LDS of every CU overwritten (abx_debug_poison_lds: NaN pattern, then large finite
    garbage) before EVERY launch of the library; every output must be bit-identical to the un-poisoned call."""
    import ctypes as C
    from abx_amd import _lib, ops, sampler
    model, D = gpu_model
    w = dict(L_heavy=46, L_light=40, L_antigen=26, cdr=(28, 36))
    b0 = _synthetic_batch(D, w, B=2, n_masked_tail=2)
    b0 = sampler.set_t_feats(b0, D, torch.full((2,), 0.5, dtype=torch.float64, device=DEV), torch.ones(2, device=DEV))
    real = _lib.load()
    pattern = [None]
    count = [0]

    class Poisoning:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith('abx_') or name in ('abx_debug_poison_lds', 'abx_last_error_string', 'abx_version') or 'bytes' in name:
                return fn

            def call(*a):
                if pattern[0] is not None:
                    assert real.abx_debug_poison_lds(pattern[0], C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
                    count[0] += 1
                return fn(*a)
            return call

    def run(pat):
        pattern[0] = pat
        try:
            bb = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b0.items()}
            r = model(bb)
            torch.cuda.synchronize()
        finally:
            pattern[0] = None
        f = r['heads']['folding']
        return [r['representations']['pair'].clone(), r['representations']['seq'].clone(), f['rigids'].clone(), f['rot_score'].clone(),
                f['final_atom14_positions'].clone(), r['heads']['sequence_module']['logits'].clone()]

    orig = _lib.load
    _lib.load = lambda: Poisoning()
    try:
        ref = run(None)
        for pat in (0x7fc00000, 0x7f7fffff):
            got = run(pat)
            assert all(torch.equal(x, y) for x, y in zip(ref, got)), hex(pat)
    finally:
        _lib.load = orig
    assert count[0] > 500


def test_design_driver_optimize_mode_with_guidance(tmp_path):
    """BASELINE config 4 shape on the shipped complex: mode = optimize, optimize_steps = 10 (10 reverse steps from t = 0.1 of the
    forward-noised ground truth) with the violation guidance on.  With seeded random weights the designed loop itself means nothing;
    checked: the fixed context is returned unchanged, every output is finite, and the guided run differs from the un-guided one
    (the gradients are applied)."""
    from abx_amd import design
    from abx_amd.io.pdb_reader import read_pdb, chain_feature
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pdb', '6ct7_H_L_S.pdb')
    common = ['--pdb_file', src, '--num_samples', '2', '--mode', 'optimize', '--optimize_steps', '10']
    plain = [f for f in design.main(common + ['--output_dir', str(tmp_path / 'plain')]) if f.endswith('.pdb')]
    guided = [f for f in design.main(common + ['--guidance', '--output_dir', str(tmp_path / 'guided')]) if f.endswith('.pdb')]
    assert len(plain) == len(guided) == 2
    ref_h = chain_feature(read_pdb(src)['H'])
    moved = 0.0
    for fp, fg in zip(sorted(plain), sorted(guided)):
        hp, hg = chain_feature(read_pdb(fp)['H']), chain_feature(read_pdb(fg)['H'])
        assert np.isfinite(hg['coords']).all() and len(hg['str_seq']) == 113
        ca_ref, ca_g = ref_h['coords'][:113, 1], hg['coords'][:, 1]
        # same frame up to the writer's re-centring: compare internal CA-CA distances of the heavy chain
        d_ref = np.linalg.norm(ca_ref[:, None] - ca_ref[None], axis=-1)
        d_g = np.linalg.norm(ca_g[:, None] - ca_g[None], axis=-1)
        fixed = np.r_[0:90, 110:113]                           # everything but the neighbourhood of CDR-H3 (diffused: residues 98-100)
        assert np.abs(d_ref - d_g)[np.ix_(fixed, fixed)].max() < 2e-2          # the fixed context comes back as it went in
        moved = max(moved, float(np.abs(hp['coords'] - hg['coords']).max()))
    assert moved > 1e-4, 'the guidance terms left the trajectory unchanged'


def test_fused_heads_equal_the_separate_launches(gpu_model, cfg):
    """the torsion ResNet, the SequenceHead MLP and the PredictedLDDTHead MLP of a pass in one launch (abx_heads_tail,
    Engine.fused_heads, the default on the split-f16 path) against the 13 - 18 launches it replaces: same tokens, torsion angles,
    logits, pLDDT and frames within fp32 rounding of the different accumulation orders (the narrow last projections move from the exact
    fp32 kernel to split-f16).  L = 120: the split-f16 path (gemm_mode 2)."""
    from abx_amd import sampler
    model, D = gpu_model
    w, B = dict(L_heavy=50, L_light=44, L_antigen=26, cdr=(30, 39)), 3
    b = _synthetic_batch(D, w, B=B, n_masked_tail=2)
    t_ = torch.full((B,), 0.4040404040404041, dtype=torch.float64, device=DEV)
    b = sampler.set_t_feats(b, D, t_, torch.ones(B, device=DEV))
    eng = model._get_engine(torch.device(DEV))
    assert eng.P.heads_pack() is not None
    outs = []
    for fused in (True, False):
        eng.fused_heads = fused
        try:
            r = model({k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}, compute_loss=True)
            f = r['heads']['folding']
            outs.append({'logits': r['heads']['sequence_module']['logits'].clone(), 'seq_0': r['heads']['sequence_module']['seq_0'].clone(),
                         'angles': f['sidechains'][-1]['angles_sin_cos'].clone(), 'rigids': f['rigids'].clone(),
                         'atom14': f['final_atom14_positions'].clone(), 'pLDDT': r['heads']['predicted_lddt']['pLDDT'].clone()})
        finally:
            eng.fused_heads = True
    assert torch.equal(outs[0]['seq_0'], outs[1]['seq_0'])
    assert torch.equal(outs[0]['rigids'], outs[1]['rigids'])                   # (the frames do not depend on the heads)
    for k, tol in (('logits', 2e-5), ('angles', 2e-5), ('atom14', 2e-4), ('pLDDT', 2e-3)):
        assert float((outs[0][k] - outs[1][k]).abs().max()) < tol, (k, float((outs[0][k] - outs[1][k]).abs().max()))


def test_op_group_entry_points_equal_the_descriptor_level_path(gpu_model, cfg):
    """SURVEY 8b / VERDICT r3 #7: abx_tri_mul_fwd, abx_tri_attn_block_fwd and abx_transition_fwd (csrc/blocks.hip: one C call per
    reference module, weights packed by abx_pack_linear) issue the same kernels with the same descriptors as the Python orchestration
    of model/forward.py: a network call through them (Engine.block_api, the default) equals the descriptor-level call BIT FOR BIT, on
    the split-f16 path (L = 120, padded pair rows: L % 16 != 0) and on the exact path (L = 56 < 64); and the packs hold what the host
    packing holds (LayerNorm fold in float64, (value, gate) column pairs, k-permuted planes)."""
    from abx_amd import sampler, ops
    model, D = gpu_model
    for w, B in ((dict(L_heavy=50, L_light=44, L_antigen=26, cdr=(30, 39)), 3), (dict(L_heavy=24, L_light=20, L_antigen=12, cdr=(10, 16)), 2)):
        b = _synthetic_batch(D, w, B=B, n_masked_tail=2)
        t_ = torch.full((B,), 0.4040404040404041, dtype=torch.float64, device=DEV)
        b = sampler.set_t_feats(b, D, t_, torch.ones(B, device=DEV))
        eng = model._get_engine(torch.device(DEV))
        outs = []
        for blk in (True, False):
            eng.block_api = blk
            try:
                r = model({k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()})
                outs.append({'pair': r['representations']['pair'].clone(), 'seq': r['representations']['seq'].clone(),
                             'rigids': r['heads']['folding']['rigids'].clone(), 'logits': r['heads']['sequence_module']['logits'].clone()})
            finally:
                eng.block_api = True
        for k in outs[0]:
            assert torch.equal(outs[0][k], outs[1][k]), (w, k, float((outs[0][k] - outs[1][k]).abs().max()))
    # the packs against an independent host evaluation (float64 torch): LayerNorm fold, (value, gate) column pairs, k-permuted planes
    P = eng.P
    blk = P.block_packs()
    sd = {k: v.double().cpu() for k, v in model.state_dict().items()}
    pre = 'impl.seqformer.seqformer.blocks.0.triangle_multiplication_outgoing.'
    glu = blk['triangle_multiplication_outgoing']._keep[0]
    Wv = torch.cat([sd[pre + 'left_proj.weight'], sd[pre + 'right_proj.weight']], 0)           # (256, 192) value rows
    Wg = torch.cat([sd[pre + 'left_gate.weight'], sd[pre + 'right_gate.weight']], 0)
    bv = torch.cat([sd[pre + 'left_proj.bias'], sd[pre + 'right_proj.bias']])
    bg = torch.cat([sd[pre + 'left_gate.bias'], sd[pre + 'right_gate.bias']])
    Wc = torch.stack([Wv.view(8, 32, 192), Wg.view(8, 32, 192)], 1).reshape(512, 192)          # [v0 | g0 | v1 | g1 ...] blocks of 32
    bc = torch.stack([bv.view(8, 32), bg.view(8, 32)], 1).reshape(512)
    gam, bet = sd[pre + 'norm.weight'], sd[pre + 'norm.bias']
    Wt_ref = (gam[:, None] * Wc.t())
    assert torch.equal(glu.Wt.cpu(), Wt_ref.float())
    assert float((glu.csum.cpu().double() - Wt_ref.sum(0)).abs().max()) < 1e-6 * float(Wt_ref.sum(0).abs().max())
    assert float((glu.bias.cpu().double() - (bet @ Wc.t() + bc)).abs().max()) < 1e-6
    got = ops.weights_to_float(glu.planes).cpu().double()[:192]
    assert float((got - glu.Wt.cpu().double()).abs().max()) <= 2.0 ** -22 * float(glu.Wt.abs().max())
    pre = 'impl.seqformer.seqformer.blocks.0.pair_transition.transition.'
    l1, l2 = blk['pair_transition']
    W2t = sd[pre + '3.weight'].t().float()                                                      # (768, 192)
    assert torch.equal(l2.Wt.cpu(), W2t) and torch.equal(l2.bias.cpu(), sd[pre + '3.bias'].float())
    perm = torch.tensor([0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15])
    W2p = W2t.view(48, 16, 192)[:, perm, :].reshape(768, 192).double()
    got = ops.weights_to_float(l2.planes).cpu().double()
    assert float((got - W2p).abs().max()) <= 2.0 ** -22 * float(W2p.abs().max())


def _visible_gpus():
    try:
        return torch.cuda.device_count()
    except Exception:          # noqa: BLE001 (no driver: 0 devices)
        return 0


@pytest.mark.skipif(_visible_gpus() < 2, reason='needs >= 2 MI355X (one rank per device over RCCL); skipped on 1-GPU boxes')
def test_multi_gpu_rccl_one_rank_per_device(tmp_path):
    """the N-rank RCCL path on REAL devices (the reference only stubs it: inference.py:59-82, 389-394).  Wakes up on a box
    with >= 2 GPUs (N = min(count, 8)), one device per rank, backend 'nccl' (= RCCL over xGMI):
      * `bench.py --gpus N` (it starts its own ranks) reports rccl_ranks == N, per-rank shards that add up, and the result digest of the
        1-GPU run of the same 16 samples - per-sample noise keys make a sample's trajectory independent of where it runs, and the
        arithmetic class of every kernel is fixed by L, not by the batch, so the gathered final state must be byte-identical;
      * `abx_amd.design --gpu_list 0 .. N-1` on the two shipped complexes (npz entries), set-level schedule and --shard_samples: the
        output tree is byte-for-byte the single-process tree."""
    import json
    import subprocess
    import sys
    from conftest import GOLDEN
    N = min(_visible_gpus(), 8)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''), HSA_ENABLE_IPC_MODE_LEGACY='0')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        env.pop(k, None)
    args = ['--steps', '1', '--warmup', '0', '--samples', '16', '--workload', 'L256', '--no-cpu-baseline', '--no-op-profile', '--no-weak']
    out = {}
    for tag, n in (('one', 1), ('many', N)):
        r = subprocess.run([sys.executable, 'bench.py', '--gpus', str(n)] + args, env=env, cwd=root, capture_output=True, text=True, timeout=1800)
        assert r.returncode == 0, tag + r.stdout[-2000:] + r.stderr[-4000:]
        out[tag] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    many = out['many']
    assert many['n_gpus'] == N and many['rccl_ranks'] == N and many['gather_ms'] is not None, many
    assert sum(many['config']['samples_per_rank']) == 16 and len(many['config']['samples_per_rank']) == N
    assert many['finite'] and len(many['result_digest']) == 64
    assert many['result_digest'] == out['one']['result_digest'], 'the gathered final state depends on the placement of the samples'
    # the design driver on the listed GPUs: files of every rank + the gathered designs table against the single-process tree
    idx = tmp_path / 'test.idx'
    idx.write_text('6ct7_H_L_S\n6qd7_X_Z_F|E\n')
    ns = max(4, N)
    common = ['--name_idx', str(idx), '--data_dir', os.path.join(GOLDEN, 'npz'), '--num_samples', str(ns), '--num_t', '3', '--mode', 'design']
    gl = ['--gpu_list'] + [str(g) for g in range(N)]
    trees = {}
    for tag, extra in (('one', ['--gpu_list', '0']), ('set', gl + ['--min_block', str(max(1, ns // 2))]), ('shard', gl + ['--shard_samples'])):
        od = str(tmp_path / tag)
        r = subprocess.run([sys.executable, '-m', 'abx_amd.design'] + common + extra + ['--output_dir', od], env=env, cwd=root,
                           capture_output=True, text=True, timeout=1800)
        assert r.returncode == 0, tag + r.stdout[-2000:] + r.stderr[-4000:]
        trees[tag] = {os.path.relpath(os.path.join(dp, f), od): open(os.path.join(dp, f), 'rb').read() for dp, _, fs in os.walk(od) for f in fs}
    for tag in ('set', 'shard'):
        assert sorted(trees[tag]) == sorted(trees['one']), (tag, sorted(set(trees[tag]) ^ set(trees['one'])))
        diff = [k for k in trees['one'] if trees['one'][k] != trees[tag][k]]
        assert not diff, (tag, diff)
