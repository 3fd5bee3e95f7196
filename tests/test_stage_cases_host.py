"""CPU checks of tests/stage_cases.py: the inputs do what tests/test_gpu_stage_kernels.py relies on.  Nothing here is tuned to a kernel:
the conditions are properties of the seeded inputs and of the float64 / float32 host evaluations alone."""
import numpy as np
import pytest
import torch

import stage_cases as SC

PAIR_CASES = SC.PAIR_CASES          # (seed, B, L, Lab): the cases of the GPU tests
PP = dict(num_bins=SC.NUM_BINS, min_bin=SC.MIN_BIN, max_bin=SC.MAX_BIN)


def test_breaks_are_the_model_configuration(cfg):
    pp = cfg.model.embeddings_and_seqformer.prev_pos
    assert (pp.min_bin, pp.max_bin, pp.num_bins) == (SC.MIN_BIN, SC.MAX_BIN, SC.NUM_BINS)
    assert cfg.model.embeddings_and_seqformer.max_relative_feature == 32
    s = SC.sq_breaks()
    assert s.dtype == torch.float32 and s.shape == (14,) and bool((s[1:] > s[:-1]).all())


@pytest.mark.parametrize('seed,B,L,Lab', PAIR_CASES)
def test_pair_case_shapes_and_ranges(sd_shapes, seed, B, L, Lab):
    c = SC.make_pair_case(seed, B, L, Lab)
    pre = 'impl.seqformer.encode_pair_emb.'
    for key, name in (('aa_pair_embed', pre + 'aa_pair_embed.weight'), ('relpos_embed', pre + 'relpos_embed.weight'),
                      ('distcoef', pre + 'aapair_to_distcoef.weight'), ('dgram_embed', pre + 'dgram_embed.weight'),
                      ('proj_rel_pos', 'impl.seqformer.proj_rel_pos.weight')):
        assert tuple(c[key].shape) == sd_shapes[name], key
        assert c[key].dtype == torch.float32
        assert torch.unique(c[key], dim=0).shape[0] == c[key].shape[0], f'{key}: every row distinct'
    assert tuple(c['proj_rel_pos5'].shape) == (13, 128) and torch.unique(c['proj_rel_pos5'], dim=0).shape[0] == 13
    dc = c['distcoef']
    assert 7.0 < float(dc.std()) < 9.0 and int((dc > 20).sum()) > 100 and int((dc < -20).sum()) > 100
    x = c['atom14']
    assert x.dtype == torch.float32 and tuple(x.shape) == (B, L, 14, 3) and float(torch.linalg.norm(x, dim=-1).max()) <= SC.MAX_COORD
    for b in range(B):
        w = c['walk_from'][b]
        step = torch.linalg.norm(x[b, w + 1:, 1] - x[b, w:-1, 1], dim=-1)
        assert step.numel() >= 6 and float((step - 3.8).abs().max()) < 1e-4, 'a 3.8 A C-alpha walk'
    ra = torch.linalg.norm(x - x[:, :, 1:2], dim=-1)
    assert float(ra[:, :, 1].max()) == 0 and 1.1 < float(ra[:, :, [0] + list(range(2, 14))].min()) and float(ra.max()) < 2.6
    assert c['aa'].dtype == torch.int64 and c['chain_id'].dtype == torch.int32 and c['residx'].dtype == torch.int32
    assert c['atom14_exists'].dtype == torch.uint8
    for b in range(B):
        assert sorted(set(c['aa'][b].tolist())) == list(range(23)), 'all 23 residue types'
    aa0 = c['aa'][0]
    assert aa0[0] != aa0[1]                     # pair (0, 1) and its transposed pair (1, 0) are both rows of the output
    ex = c['atom14_exists']
    other = ex[..., [0] + list(range(2, 14))].sum(-1)
    for b in range(B):
        assert int(((ex[b, :, 1] == 0) & (other[b] > 0)).sum()) >= 3, 'C-alpha missing, other atoms present'
        assert int(((ex[b, :, 1] == 1) & (other[b] == 0)).sum()) >= 2, 'C-alpha alone'
        assert int(((ex[b, :, 1] == 1) & (ex[b, :, 0] == 0)).sum()) >= 1, 'atom 0 missing, C-alpha present'
        assert int(((ex[b, :, 1] == 0) & (ex[b, :, 0] == 1)).sum()) >= 1, 'C-alpha missing, atom 0 present'
    assert bool((c['a37to14'][..., :3] == torch.arange(3)).all()), 'the atom37 lift keeps N, CA, C in slots 0..2'


@pytest.mark.parametrize('seed,B,L,Lab', PAIR_CASES)
def test_chains_and_numbering_reach_the_clamps(seed, B, L, Lab):
    c = SC.make_pair_case(seed, B, L, Lab)
    r = SC.pair_reference(seed, B, L, Lab)
    chain, residx = c['chain_id'], c['residx']
    assert len(set(chain[0].tolist())) >= 3
    n0, n1 = set(residx[0][chain[0] == 0].tolist()), set(residx[0][chain[0] == 1].tolist())
    assert len(n0 & n1) >= 5, 'two chains share residue numbers'
    for b in range(B):
        ra = residx[b][chain[b] == 0]
        assert int((ra[1:] - ra[:-1]).max()) > 40, 'a numbering gap of more than 40 inside a chain'
        assert int((ra[1:] == ra[:-1]).sum()) >= 1, 'a repeated residue number'
    raw = residx[:, :, None] - residx[:, None, :]
    assert int(raw[r['same_chain']].max()) > 32 and int(raw[r['same_chain']].min()) < -32
    assert sorted(set(r['rel'][r['same_chain']].tolist())) == list(range(65)), 'every clamped offset among same-chain pairs'
    other = set(r['rel'][~r['same_chain']].tolist())
    assert {0, 32, 64} <= other, 'offsets (the clamped ones included) among different-chain pairs'
    if 0 < Lab < L:
        assert chain[0, Lab - 1] == chain[0, Lab] and abs(int(residx[0, Lab] - residx[0, Lab - 1])) == 1, 'Lab cuts through a chain'
    for max_rel in (32, 5):
        slots = SC.relpos_slots(residx, max_rel)
        i = torch.arange(L)
        on = (i[:, None] < Lab) == (i[None, :] < Lab)
        assert {1, 2 * max_rel + 1} <= set(slots[:, on].reshape(-1).tolist()), 'both clamps of relpos_block fire on-block'
        assert bool(on.any()) and bool((~on).any()) == (0 < Lab < L)
        table = c['proj_rel_pos'] if max_rel == 32 else c['proj_rel_pos5']
        ref = SC.relpos_block_reference(residx, table, Lab, max_rel)
        assert bool((ref[:, ~on] == 0).all()) and bool((ref[:, on].abs().sum(-1) > 0).all())
        assert torch.equal(ref[:, on], table[slots[:, on]])


@pytest.mark.parametrize('seed,B,L,Lab', PAIR_CASES)
def test_distogram_edges(seed, B, L, Lab):
    from oracle import abx_oracle as O
    c = SC.make_pair_case(seed, B, L, Lab)
    r = SC.pair_reference(seed, B, L, Lab)
    near, bins = r['near_edge'], r['bins']
    share = float(near.float().mean())
    print(f'L = {L}: near_edge share {share:.5f}')
    assert share <= 0.01
    s = c['sq_breaks'].double()
    for res, k, side in SC.edge_pairs():
        for i, j in ((0, res), (res, 0)):
            assert not bool(near[0, i, j]), (res, k, side)
            assert int(bins[0, i, j]) == k + side, (res, k, side, float(r['d2'][0, i, j]), float(s[k]))
        rel = float(r['d2'][0, 0, res] / s[k]) - 1.0
        assert abs(abs(rel) - SC.EDGE) < 1e-4 and (rel > 0) == bool(side), 'the pair sits EDGE below / above its break'
    # the tie pairs: every float32 step up to the square is exact, so the float32 d2 IS the float32 squared break and the strict `>` gives k
    pb32 = O.pseudo_beta_v2(c['atom14'])
    ties = SC.tie_pairs(B, L)
    assert len(ties) >= 7 and (len(ties) == 14 or B * L * L < 5000)
    for b, t0, res, k in ties:
        assert pb32[b, t0, 0] == 0 and pb32[b, res, 0] == c['atom14'][b, res, 1, 0] and torch.equal(pb32[b, t0, 1:], pb32[b, res, 1:])
        dv = pb32[b, t0] - pb32[b, res]
        assert float(dv[1]) == 0 and float(dv[2]) == 0 and torch.sum(torch.square(dv)) == c['sq_breaks'][k]
        assert bool(near[b, t0, res]) and bool(near[b, res, t0])
    o32_ = O.dgram_from_positions(pb32, **PP)
    assert all(int(o32_[b, t0, res]) == k and int(o32_[b, res, t0]) == k for b, t0, res, k in ties)
    assert int(bins[0, 0, SC.FAR]) == 14 and float(r['d2'][0, 0, SC.FAR]) > 25.0 ** 2
    assert sorted(set(bins.reshape(-1).tolist())) == list(range(15)), 'all 15 bins occur'
    d = torch.arange(L)
    assert bool((bins[:, d, d] == 0).all()) and not bool(near[:, d, d].any())
    # the margin is wide enough: a correct float32 evaluation (the oracle's) gives the float64 bin wherever the pair is not near an edge
    x = c['atom14']
    o32 = O.dgram_from_positions(O.pseudo_beta_v2(x), **PP)
    assert torch.equal(o32[~near], bins[~near])
    a37 = O.atom14_to_atom37(x, c['a37to14'])
    assert torch.equal(O.dgram_from_positions(O.pseudo_beta_v2(a37), **PP), o32), 'the atom37 lift changes no bin'
    assert torch.equal(torch.square(torch.linspace(SC.MIN_BIN, SC.MAX_BIN, steps=SC.NUM_BINS - 1)), c['sq_breaks'])


def test_dist_gauss_reference_and_fp32_baseline():
    seed, B, L, Lab = PAIR_CASES[0]
    c = SC.make_pair_case(seed, B, L, Lab)
    r = SC.pair_reference(seed, B, L, Lab)
    g = r['d_gauss']
    assert g.dtype == torch.float64 and tuple(g.shape) == (B, L, L, 196)
    assert bool((g[~r['ca_pair']] == 0).all()) and bool((g[r['ca_pair']] > 0).any())
    # one entry by hand: (b, i, j, a, a') -> scalar float64 arithmetic
    b, i, j, a, a2 = 0, 2, 9, 4, 12
    w = float(c['distcoef'][int(c['aa'][b, i]) * 23 + int(c['aa'][b, j]), a * 14 + a2])
    sp = w if w > 20 else np.log1p(np.exp(w))
    d = np.linalg.norm(c['atom14'][b, i, a].double().numpy() - c['atom14'][b, j, a2].double().numpy()) / 10
    assert abs(float(g[b, i, j, a * 14 + a2]) - np.exp(-sp * d * d)) < 1e-14
    base = float((SC.dist_gauss(c, torch.float32).double() - g).abs().max())
    print(f'fp32 host restatement of d_gauss against float64: max abs error {base:.3e}')
    assert 0 < base < 1e-6


def test_residue_case_special_rows():
    for B, L in ((3, 131), (1, 1)):
        c = SC.make_residue_case(60, B, L)
        n = c['n']
        fixed = c['fixed'].view(-1)
        assert len(c['zero_rows']) == 3 and len(set(c['zero_rows'])) == 3
        for r, k in c['zero_rows']:
            assert bool((c['unnorm'][r, k] == 0).all()) and fixed[r] == 0
        ref = c['unnorm'] / torch.sqrt(torch.sum(c['unnorm'] * c['unnorm'], dim=-1, keepdim=True) + 1e-12)
        for r, k in c['zero_rows']:
            assert bool((ref[r, k] == 0).all()), 'l2_normalize with eps 1e-12 gives exact zeros'
        row = c['logits'].view(n, 20)[c['tie_row']]
        assert row[4] == row[13] == row.max() and int((row == row.max()).sum()) == 2 and int(row.argmax()) == 4 and fixed[c['tie_row']] == 0
        pl = c['plddt_logits'][c['plddt_row']]
        assert float(pl.max() - pl.min()) == 80.0
        assert int(c['seq_t'].min()) >= 0 and int(c['seq_t'].max()) <= 20
        if n > 1:
            assert 0 < int(fixed.sum()) < n
            assert max(r for r, _ in c['zero_rows']) >= 384 and c['tie_row'] >= 384, 'special rows in the last block of 128 and of 256'
            assert bool(fixed[384:].any()) and not bool(fixed[384:].all())
