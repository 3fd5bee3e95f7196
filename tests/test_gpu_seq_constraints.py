"""Sequence constraints on the GPU (abx_amd.constraints): the constrained token part of abx_reverse_step against the oracle's rates,
the inverse-cdf restatement and the host twin of the landing rule; the off state; the masked argmax of abx_seq_head_atoms_biased; the
sampler (eager and graph replay) on the tiny workload; the design driver on a shipped complex."""
import os

import numpy as np
import pytest
import torch

from analysis_gpu_cases import (DEV, SHARED, TODAY, assert_same_bytes, gpu_model, names, ops, pdb_args, sample_tiny,       # noqa: F401
                                set_master_port, spy_on_sampler, table_lines, tiny_batch)

pytestmark = pytest.mark.gpu

NINF = float('-inf')
KEEP = (1, 2, 5, 10, 19, 20)


def token_inputs(seed=401, B=4, L=300):
    """The vectors of the kernel-level tests -> (x_t (B,L), logits (B,L,20), u (B,L,20) on the 2^-24 grid, table (L,20), dm (B,L)).
    Row l of the table keeps KEEP[l % 6] letters of a seeded permutation; the kept entries are 0 on alternate cycles of six and
    2 * randn on the others.  The last 12 residues are not diffused (the kernel test reads the table there all the same)."""
    ge = torch.Generator().manual_seed(seed)
    x_t = torch.randint(0, 20, (B, L), generator=ge)
    lg = 3.0 * torch.randn(B, L, 20, generator=ge)
    u = (torch.randint(0, 1 << 24, (B, L, 20), generator=ge).float() + 0.5) / float(1 << 24)
    table = torch.full((L, 20), NINF)
    for l in range(L):
        kept = torch.randperm(20, generator=ge)[:KEEP[l % 6]]
        vals = 2.0 * torch.randn(len(kept), generator=ge)
        table[l, kept] = vals if (l // 6) % 2 else torch.zeros(len(kept))
    dm = torch.ones(B, L, dtype=torch.int32)
    dm[:, L - 12:] = 0
    return x_t, lg, u, table, dm


def _token_diffuser(cfg):
    from abx_amd.diffuser.full_diffuser import FullDiffuser
    D = FullDiffuser(cfg.diffuser)
    D.set_tables(torch.zeros(1000, 1000), torch.zeros(1000, 1000), torch.zeros(1000, 1000), DEV)
    return D


def _token_step(D, x_t, logits, t, dt, dm=None, noise=None, **kw):
    """abx_reverse_step with neutral rigid inputs: returns (seq_out, rates * dt, applied jump counts)."""
    B, L = x_t.shape
    rig = torch.zeros(B, L, 7, dtype=torch.float64, device=DEV)
    rig[..., 0] = 1.0
    z3 = torch.zeros(B, L, 3, device=DEV)
    rates = torch.full((B, L, 20), -1.0, device=DEV)
    jumps = torch.full((B, L, 20), -1.0, device=DEV)
    if dm is None:
        dm = torch.ones(B, L, dtype=torch.int32, device=DEV)
    _, seq = D.reverse(rig, x_t.to(DEV), z3, z3.double(), logits.to(DEV), torch.full((B,), float(t), dtype=torch.float64, device=DEV),
                       dt, dm, noise=noise, rates_out=rates, jumps_out=jumps, **kw)
    return seq.cpu(), rates.cpu(), jumps.cpu()


def test_constrained_token_step_rates_jumps_and_landing(ops, cfg):
    """B = 4, L = 300 (the residue loop of the 256-thread workgroup wraps), two (t, dt).  (a) the rate is exactly 0 at every forbidden
    target and at the current token; (b) on the allowed targets it is the oracle's rate on logits + bias, to the 2e-6 of the
    unconstrained closed form; (c) the jump counts are the inverse cdf of the reported rates, bit for bit; (d) the tokens are
    token_step_host of the reported jumps; (e) a row that starts allowed ends allowed; (f) rows outside diffuse_mask keep their token."""
    from oracle import abx_oracle as O
    from abx_amd.constraints import token_step_host
    x_t, lg, u, table, dm = token_inputs()
    B, L = x_t.shape
    allowed = (table != NINF).numpy()
    al_b = np.broadcast_to(allowed, (B, L, 20))
    D = _token_diffuser(cfg)
    assert abs(D.rate_const - 0.3) < 1e-6
    seq_o = O.OracleSeq({'rate_const': D.rate_const})
    cur = torch.nn.functional.one_hot(x_t, 20).bool().numpy()
    rows = np.broadcast_to(np.arange(L), (B, L))
    mov = dm.bool().numpy()
    for step, (t, dt) in enumerate(((0.02, 0.1), (0.5, 0.01))):
        seq, lam, ja = _token_step(D, x_t, lg, t, dt, dm=dm.to(DEV), noise=dict(u_jumps=u.to(DEV)), seq_bias=table.to(DEV))
        seq, lam_n, ja_n = seq.numpy(), lam.numpy(), ja.numpy()
        closed = ~al_b | cur
        assert (lam_n[closed] == 0).all() and (ja_n[closed] == 0).all()                                    # (a)
        ro, _ = seq_o.reverse_rates(x_t, lg + table[None], torch.tensor(t))
        lo = (ro * dt).numpy()
        assert (lo[~closed] > 0).all() and (lam_n[~closed] > 0).all()
        rel = np.abs(lam_n - lo)[~closed] / lo[~closed]
        print(f'step {step}: max relative rate error {rel.max():.3e}')
        assert float(rel.max()) < 2e-6, float(rel.max())                                                   # (b)
        want_j = O.poisson_icdf(lam_n, u.numpy())
        assert np.array_equal(ja_n, want_j), int((ja_n != want_j).sum())                                   # (c)
        want = token_step_host(x_t.numpy(), ja_n, allowed)
        assert np.array_equal(seq[mov], want[mov])                                                         # (d)
        starts_ok = allowed[rows, x_t.numpy()]
        assert allowed[rows, seq][mov & starts_ok].all()                                                   # (e)
        assert np.array_equal(seq[~mov], x_t.numpy()[~mov])                                                # (f)
        if step == 0:                                   # what keeps the test honest: every rule is exercised many times
            diffs = np.arange(20)[None, None] - x_t.numpy()[..., None]
            land = np.clip(x_t.numpy() + (ja_n * diffs).sum(-1), 0, 19).astype(np.int64)
            rejected = mov & (ja_n.sum(-1) > 0) & (land != x_t.numpy()) & ~allowed[rows, land]
            start_bad = mov & ~starts_ok
            left = start_bad & allowed[rows, seq]
            print(f'rejected {int(rejected.sum())}, start forbidden {int(start_bad.sum())}, left {int(left.sum())}, rates > 3: {int((lam_n > 3).sum())}')
            assert int(rejected.sum()) >= 100 and int(start_bad.sum()) >= 100 and int(left.sum()) >= 50 and int((lam_n > 3).sum()) >= 300
            assert np.array_equal(seq[rejected], x_t.numpy()[rejected])


def test_row_without_a_finite_entry_keeps_its_token(ops, cfg):
    """The host refuses such a table; the kernel must still not produce NaN: all rates 0, no jump, the token stays."""
    x_t, lg, u, table, dm = token_inputs(B=2, L=40)
    table[7] = NINF
    table[39] = NINF
    D = _token_diffuser(cfg)
    for noise in (dict(u_jumps=u.to(DEV)), None):
        seq, lam, ja = _token_step(D, x_t, lg, 0.02, 0.1, noise=noise, seq_bias=table.to(DEV), step=2)
        assert torch.isfinite(lam).all() and torch.isfinite(ja).all()
        for l in (7, 39):
            assert not lam[:, l].any() and not ja[:, l].any() and torch.equal(seq[:, l], x_t[:, l])


def test_table_of_zeros_is_the_unconstrained_step(ops, cfg):
    """seq_bias = zeros and seq_bias = None: identical tokens, rigids, rates and jump counts, with supplied uniforms and with the
    device Philox generator (same seed, sample ids and step)."""
    x_t, lg, u, _, dm = token_inputs(seed=402, B=3, L=300)
    B, L = x_t.shape
    ge = torch.Generator().manual_seed(7)
    q = torch.randn(B, L, 4, generator=ge, dtype=torch.float64)
    rig = torch.cat([q / q.norm(dim=-1, keepdim=True), 10 * torch.randn(B, L, 3, generator=ge, dtype=torch.float64)], -1).to(DEV)
    rs, ts = torch.randn(B, L, 3, generator=ge).to(DEV), torch.randn(B, L, 3, generator=ge, dtype=torch.float64).to(DEV)
    D = _token_diffuser(cfg)
    D.seed = 99
    ids = torch.arange(B, device=DEV) + 40
    tt_ = torch.full((B,), 0.3, dtype=torch.float64, device=DEV)
    zeros = torch.zeros(L, 20, device=DEV)

    def run(noise, bias):
        rates, jumps = torch.full((B, L, 20), -1.0, device=DEV), torch.full((B, L, 20), -1.0, device=DEV)
        r, s = D.reverse(rig, x_t.to(DEV), rs, ts, lg.to(DEV), tt_, 0.05, dm.to(DEV), noise=noise, sample_ids=ids, step=3, rates_out=rates,
                         jumps_out=jumps, seq_bias=bias)
        return s.cpu(), r.cpu(), rates.cpu(), jumps.cpu()

    for noise in (dict(u_jumps=u.to(DEV)), None):
        plain, zero = run(noise, None), run(noise, zeros)
        assert float(plain[3].sum()) > 100                                   # jumps happen
        for name, p, z in zip(('seq_out', 'rigid_out', 'rates_out', 'jumps_out'), plain, zero):
            assert torch.equal(p, z), (name, noise is None)


def test_masked_argmax_equals_the_plain_entry_point_on_biased_logits(ops):
    """L = 37, n = 5 L = 185 (no multiple of the 128-thread block; the table rows repeat across the samples): the biased entry point on
    (logits, bias) and the existing one on logits + bias give the same seq_0, atom14 and atom37, bit for bit; seq_0 is
    masked_argmax_host with constructed ties; fixed residues keep seq_t."""
    from abx_amd import residue_constants as rc
    from abx_amd.constraints import masked_argmax_host
    B, L = 5, 37
    n = B * L
    ge = torch.Generator().manual_seed(403)
    logits = torch.randn(B, L, 20, generator=ge)
    bias = torch.zeros(L, 20)
    for l in range(L):
        kept = torch.randperm(20, generator=ge)[:KEEP[l % 6]]
        row = torch.full((20,), NINF)
        row[kept] = torch.round(2.0 * torch.randn(len(kept), generator=ge) * 4) / 4
        bias[l] = row
    # ties: equal sums at two or three letters that beat everything else in the row (quarter-integer values add exactly in fp32)
    bias[3], bias[10], bias[16] = 0.0, 0.0, 0.0
    logits[:, 3] = torch.round(logits[:, 3] * 4) / 4
    logits[:, 3, 12], logits[:, 3, 5] = 9.0, 9.0                              # plain tie: letter 5
    logits[:, 10, 17], logits[:, 10, 2], logits[:, 10, 8] = 7.0, 5.0, 6.0
    bias[10, 2], bias[10, 8], bias[10, 17] = 3.0, 2.0, 1.0                    # 8 = 8 = 8: letter 2
    logits[:, 16, 0], logits[:, 16, 19], logits[:, 16, 4] = 20.0, 11.0, 11.0
    bias[16, 0] = NINF                                                       # the overall maximum is forbidden; then the tie 4 / 19
    fixed = (torch.rand(B, L, generator=ge) < 0.25).int()
    fixed[:, [3, 10, 16]] = 0
    seq_t = torch.randint(0, 21, (B, L), generator=ge)
    a37 = torch.as_tensor(rc.restype_atom37_to_atom14)[torch.randint(0, 20, (B, L), generator=ge)].long()
    ang = torch.randn(B, L, 7, 2, generator=ge)
    ang = ang / ang.norm(dim=-1, keepdim=True)
    q = torch.randn(B, L, 4, generator=ge)
    rg = torch.cat([q / q.norm(dim=-1, keepdim=True), 10 * torch.randn(B, L, 3, generator=ge)], -1)
    dframes = torch.as_tensor(rc.restype_rigid_group_default_frame).float().to(DEV).contiguous()
    gidx = torch.as_tensor(rc.restype_atom14_to_rigid_group).to(torch.int32).to(DEV).contiguous()
    lit = torch.as_tensor(rc.restype_atom14_rigid_group_positions).float().to(DEV).contiguous()
    d = lambda x: x.to(DEV).contiguous()

    def run(lg, **kw):
        seq0 = torch.full((n,), -1, dtype=torch.int64, device=DEV)
        a14, a37o = torch.full((n, 14, 3), float('nan'), device=DEV), torch.full((n, 37, 3), float('nan'), device=DEV)
        ops.seq_head_atoms(d(lg), d(fixed.view(-1)), d(seq_t), d(rg), d(ang), d(a37), dframes, gidx, lit, seq0, a14, a37o, n, **kw)
        return seq0.cpu().view(B, L), a14.cpu(), a37o.cpu()

    lg_dev = d(logits)
    got = run(logits, seq_bias=d(bias), L=L)
    want = run(logits + bias[None])
    for name, g_, w_ in zip(('seq_0', 'atom14', 'atom37'), got, want):
        assert torch.equal(g_, w_), name
    assert torch.isfinite(got[1]).all() and torch.isfinite(got[2]).all()
    host = torch.from_numpy(masked_argmax_host(logits.numpy(), bias.numpy()))
    assert torch.equal(got[0], torch.where(fixed.bool(), seq_t, host))
    assert got[0][:, 3].tolist() == [5] * B and got[0][:, 10].tolist() == [2] * B and got[0][:, 16].tolist() == [4] * B
    free = ~fixed.bool()
    assert (bias != NINF)[torch.arange(L).expand(B, L), got[0].clamp(max=19)][free].all()     # a free residue never gets a forbidden letter
    assert torch.equal(d(logits), lg_dev)                                                     # the logits are read only
    changed = (got[0] != run(logits)[0]) & free
    assert int(changed.sum()) > 20                                                            # the table matters on these vectors


# -------------------------------------------------------------------------------------------------------------------
# sampler
# -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tiny_runs(gpu_model, cfg, tmp_path_factory):
    """The tiny workload sampled plain and constrained (a forbid set, one residue fixed to one letter, a soft bias) -> dict."""
    from abx_amd.constraints import LETTERS, SequenceConstraints
    batch, sid = tiny_batch(gpu_model)
    dm = ((1 - batch['fixed_mask'][0]) * batch['atom14_gt_exists'][0, :, 0]).bool().cpu().numpy()
    rows = np.nonzero(dm)[0]
    assert len(rows) >= 3
    zero = SequenceConstraints(batch, ['H', 'L', 'A'])
    fix_row, fix_letter = int(rows[1]), 'W'
    f = tmp_path_factory.mktemp('seq') / 'bias.txt'
    f.write_text('* SGY 2.0\n')
    cons = SequenceConstraints(batch, ['H', 'L', 'A'], bias_file=str(f), forbid=['C', 'M', 'AVLI'], fix=[f'{zero.names[fix_row]}={fix_letter}'])
    plain = sample_tiny(gpu_model, cfg, batch, sid)
    return dict(batch=batch, sid=sid, rows=rows, dm=dm, zero=zero, cons=cons, fix=(fix_row, LETTERS.index(fix_letter)), plain=plain,
                eager=sample_tiny(gpu_model, cfg, batch, sid, constraints=cons))


def test_sampler_obeys_the_constraints_in_every_record(tiny_runs):
    R = tiny_runs
    cons, rows, (fix_row, fix_tok) = R['cons'], R['rows'], R['fix']
    assert not cons.allowed[rows].all() and cons.allowed[fix_row].sum() == 1
    assert len(R['eager']) == len(R['plain']) == 5
    other = np.nonzero(~R['dm'])[0]
    Lab = R['eager'][0]['seq'].shape[1]
    assert rows.max() < Lab
    changed = 0
    for k, (p, q) in enumerate(zip(R['plain'], R['eager'])):
        assert set(q) - {'range_fallbacks', 'range_sticky_ops'} == TODAY, (k, sorted(q))
        for key in ('seq_t', 'seq'):
            tok = q[key].cpu().numpy()
            for r in rows:
                assert cons.allowed[r, np.clip(tok[:, r], 0, 19)].all(), (k, key, cons.names[r], tok[:, r])
            assert (tok[:, fix_row] == fix_tok).all(), (k, key, tok[:, fix_row])
            keep = other[other < tok.shape[1]]
            assert np.array_equal(tok[:, keep], p[key].cpu().numpy()[:, keep]), (k, key)
            changed += int((tok[:, rows] != p[key].cpu().numpy()[:, rows]).sum())
        assert torch.isfinite(q['atom14_results']).all() and torch.isfinite(q['rigids_t']).all()
    assert changed > 0                                                   # the plain run did not obey them by chance


def test_sampler_with_a_table_of_zeros_is_the_plain_sampler(gpu_model, cfg, tiny_runs):
    R = tiny_runs
    zero = sample_tiny(gpu_model, cfg, R['batch'], R['sid'], constraints=R['zero'])
    assert 'seq_bias' not in R['batch']                                  # the table went into the sampler's own copy of the batch
    for k, (p, q) in enumerate(zip(R['plain'], zero)):
        assert set(q) - {'range_fallbacks', 'range_sticky_ops'} == TODAY
        for key in SHARED:
            assert torch.equal(p[key], q[key]), (k, key)


def test_sampler_graph_replay_equals_the_eager_constrained_run(gpu_model, cfg, tiny_runs):
    R = tiny_runs
    graph = sample_tiny(gpu_model, cfg, R['batch'], R['sid'], constraints=R['cons'], use_graph=True)
    assert len(graph) == 5
    for k, (p, q) in enumerate(zip(R['eager'], graph)):
        for key in SHARED:
            assert torch.equal(p[key], q[key]), (k, key)


# -------------------------------------------------------------------------------------------------------------------
# driver
# -------------------------------------------------------------------------------------------------------------------
def test_design_driver_forbid_fix_and_the_sequence_table(tmp_path, monkeypatch):
    """`abx_amd.design` on the shipped 6ct7 complex, 4 samples, 4 grid points: --seq_forbid C M and --seq_fix on the first H3 residue
    hold in <complex>_designs.tsv, <complex>_sequence.tsv has one line per designed residue and no violation; a --seq_bias file of zeros
    leaves every file of the plain run byte-identical and adds the one table."""
    from abx_amd import design
    from abx_amd.constraints import LETTERS
    code, N = '6ct7_H_L_S', 4
    seen = spy_on_sampler(monkeypatch, lambda batch, kw, traj: (batch, kw.get('constraints')))
    set_master_port(monkeypatch)
    common = pdb_args([code]) + ['--num_samples', str(N), '--num_t', '4']
    plain_files = design.main(common + ['--output_dir', str(tmp_path / 'plain')])
    batch, none = seen[-1]
    assert none is None
    dm = ((1 - batch['fixed_mask'][0]) * batch['atom14_gt_exists'][0, :, 0]).bool().cpu().numpy()
    rows = np.nonzero(dm)[0]
    r0 = int(rows[0])
    assert int(batch['chain_id'][0, r0]) == 0                            # the first H3 residue, named from the featurised batch
    res = f'H:{int(batch["residx"][0, r0])}'
    wild = ''.join(LETTERS[int(a)] for a in batch['seq'][0].tolist()[:batch['anchor_flag'].shape[1]])
    # ---- forbid + fix
    out = tmp_path / 'cons'
    files = design.main(common + ['--seq_forbid', 'C', 'M', '--seq_fix', f'{res}=Y', '--output_dir', str(out)])
    assert names(files) == sorted(names(plain_files) + [f'{code}_sequence.tsv'])
    assert seen[-1][1] is not None and seen[-1][1].names[r0] == res
    designs = table_lines(out, code, 'designs')[1:]
    assert len(designs) == N
    for ln in designs:
        s = ln[2]
        assert len(s) == len(wild) and s[r0] == 'Y' and not set(s[r] for r in rows) & set('CM'), s
        assert all(s[r] == wild[r] for r in range(len(wild)) if r not in rows)
    tab = table_lines(out, code, 'sequence')
    assert tab[0] == ['residue', 'wild', 'allowed'] + list(LETTERS) + ['violations'] and len(tab) == 1 + len(rows)
    for ln, r in zip(tab[1:], rows):
        assert ln[0] == seen[-1][1].names[r] and ln[1] == wild[r] and ln[-1] == '0'
        assert ln[2] == ('Y' if r == r0 else ''.join(c for c in LETTERS if c not in 'CM'))
        counts = [int(v) for v in ln[3:23]]
        assert sum(counts) == N and counts == [sum(d[2][r] == c for d in designs) for c in LETTERS]
    # ---- a file of zeros: the plain run's bytes, plus the one table
    zf = tmp_path / 'zeros.txt'
    zf.write_text('# no opinion\n* ARNDCQEGHILKMFPSTWYV 0\n')
    zout = tmp_path / 'zeros'
    zfiles = design.main(common + ['--seq_bias', str(zf), '--output_dir', str(zout)])
    assert names(zfiles) == sorted(names(plain_files) + [f'{code}_sequence.tsv'])
    assert sorted(os.listdir(zout)) == names(zfiles)
    assert_same_bytes(plain_files, zout)
    assert all(ln[-1] == '0' and ln[2] == LETTERS for ln in table_lines(zout, code, 'sequence')[1:])


def test_design_driver_set_level_schedule_writes_one_table_per_complex(tmp_path, monkeypatch):
    """Both shipped complexes through the 1-rank RCCL path (whole work units, one gather of rows at the end): --seq_forbid holds in the
    designs of each, and each gets its <complex>_sequence.tsv from the gathered rows."""
    from abx_amd import design
    from abx_amd.constraints import LETTERS
    from analysis_gpu_cases import CODES
    seen = spy_on_sampler(monkeypatch, lambda batch, kw, traj: (batch['seq'].shape[1], kw.get('constraints')))
    set_master_port(monkeypatch)
    out = tmp_path / 'set'
    files = design.main(pdb_args(CODES) + ['--num_samples', '2', '--num_t', '4', '--force_collective', '--min_block', '1', '--seq_forbid', 'CM',
                                           '--output_dir', str(out)])
    assert [f for f in names(files) if f.endswith('_sequence.tsv')] == sorted(f'{c}_sequence.tsv' for c in CODES)
    assert len(seen) == 4 and all(c is not None for _, c in seen)
    for code in CODES:
        cons = next(c for L, c in seen if L == (231 if code.startswith('6ct7') else 259))
        rows = np.nonzero(cons.diffuse_mask)[0]
        designs = table_lines(out, code, 'designs')[1:]
        assert len(designs) == 2 and not any(set(d[2][r] for r in rows) & set('CM') for d in designs)
        tab = table_lines(out, code, 'sequence')
        assert [ln[0] for ln in tab[1:]] == [cons.names[r] for r in rows]
        for ln, r in zip(tab[1:], rows):
            assert ln[2] == ''.join(c for c in LETTERS if c not in 'CM') and ln[-1] == '0'
            assert [int(v) for v in ln[3:23]] == [sum(d[2][r] == c for d in designs) for c in LETTERS]
