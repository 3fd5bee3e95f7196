"""Kernel-level parity of the embedding stage (csrc/embed.hip) and the per-residue geometry stage (csrc/geometry.hip) against float64
restatements of the same operations on the seeded inputs of tests/stage_cases.py (their properties are asserted on the CPU in
tests/test_stage_cases_host.py).  Gathers, clamps, masks and distogram bins are compared exactly; every output buffer is NaN (or -1)
before the launch, so a row that a kernel skips or a column that it must leave alone shows.  Needs an MI355X: `pytest -m gpu`."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stage_cases as SC

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN = float('nan')


@pytest.fixture(scope='module')
def ops():
    from abx_amd import ops as _ops, _lib
    lib = _lib.load()
    assert lib.abx_init(0) == 0, lib.abx_last_error_string()
    return _ops


def dev(x):
    return x.contiguous().to(DEV)


def nans(*shape):
    return torch.full(shape, NAN, device=DEV)


def guarded(x, extra):
    """x on the device as the head of a longer buffer whose tail holds `extra` zeros: a kernel that is off by one row reads zeros (a valid
    index, a finite value) there, and what it writes shows in the NaN tail of the output."""
    buf = torch.zeros(x.numel() + extra, dtype=x.dtype, device=DEV)
    buf[:x.numel()] = x.reshape(-1).to(DEV)
    return buf[:x.numel()].view(x.shape)


def g(seed):
    return torch.Generator().manual_seed(seed)


def rel_err(a, b):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def check(a, b, tol, name):
    assert a.shape == b.shape, (name, a.shape, b.shape)
    e = rel_err(a, b)
    assert np.isfinite(e) and e <= tol, f'{name}: rel err {e:.3e} > {tol}'


def check_blocks(a, b, tol, name, n, blk=128):
    """check() on the whole tensor, then on every block of `blk` residues with the block's own normalisation: rows that only a later
    thread block writes cannot hide behind the largest reference value of the whole tensor."""
    check(a, b, tol, name)
    a2, b2 = a.detach().cpu().double().reshape(n, -1), b.detach().cpu().double().reshape(n, -1)
    for s in range(0, n, blk):
        check(a2[s:s + blk], b2[s:s + blk], tol, f'{name}, residues {s}..{min(s + blk, n) - 1}')


# ------------------------------------------------------------------------------------------------------------------
# embed.hip: pair_embed_features, relpos_block, gather_rows
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed,B,L,Lab', SC.PAIR_CASES)
def test_pair_embed_features(ops, seed, B, L, Lab):
    """Gathered groups bit for bit, the distance-MLP columns untouched, dist196 exactly 0 without both C-alpha and within
    atol = 8 x (max abs error of the float32 host restatement against float64) elsewhere.  The factor 8: device expf / log1pf are a
    couple of ulp looser than libm, the kernel takes sqrtf(..) / 10 then d * d where the model has dist ** 2, and an argument error is
    amplified by at most x exp(-x) <= 0.37.
    Measured on the MI355X (float32 host baseline / kernel max abs error): L = 37: 1.482e-07 / 1.482e-07; L = 70: 1.570e-07 / 1.593e-07;
    L = 131: 1.581e-07 / 1.504e-07, against atol = 1.19e-06, 1.26e-06, 1.26e-06.
    """
    c, r = SC.make_pair_case(seed, B, L, Lab), SC.pair_reference(seed, B, L, Lab)
    M2 = B * L * L
    feat, dist = nans(M2, 512), nans(M2, 196)
    ops.pair_embed_features(dev(c['aa']), dev(c['chain_id']), dev(c['residx']), dev(c['atom14']), dev(c['atom14_exists']),
                            dev(c['aa_pair_embed']), dev(c['relpos_embed']), dev(c['distcoef']), dev(c['dgram_embed']), dev(c['sq_breaks']),
                            feat, dist, B, L)
    torch.cuda.synchronize()
    f = feat.cpu().view(B, L, L, 512)
    assert torch.equal(f[..., 0:128], r['f_aapair']), 'aa_pair_embed[aa_i * 23 + aa_j]'
    assert torch.equal(f[..., 128:256], r['f_relpos']), 'relpos_embed[clamp(residx_i - residx_j) + 32] * same_chain'
    assert bool((f[..., 128:256][~r['same_chain']] == 0).all()), 'different chains: exact zeros'
    assert bool(torch.isnan(f[..., 256:384]).all()), 'columns 256..383 belong to the distance MLP'
    near = r['near_edge']
    fd = f[..., 384:512]
    for res, k, side in SC.edge_pairs():
        for i, j in ((0, res), (res, 0)):
            assert torch.equal(fd[0, i, j], c['dgram_embed'][k + side]), f'pair ({i}, {j}) sits {"above" if side else "below"} break {k}'
    assert torch.equal(fd[0, 0, SC.FAR], c['dgram_embed'][14])
    for b, t0, res, k in SC.tie_pairs(B, L):
        for i, j in ((t0, res), (res, t0)):
            assert torch.equal(fd[b, i, j], c['dgram_embed'][k]), f'pair ({i}, {j}) of sample {b} sits ON break {k}: d2 > break is false'
    assert torch.equal(fd[~near], r['f_dgram'][~near]), 'dgram_embed[bin] away from the breaks'
    d = dist.cpu().view(B, L, L, 196)
    assert bool(torch.isfinite(d).all())
    assert bool((d[~r['ca_pair']] == 0).all()), 'a missing C-alpha on either side: exact zeros'
    ref = r['d_gauss']
    base = float((SC.dist_gauss(c, torch.float32).double() - ref).abs().max())
    err = float((d.double() - ref)[r['ca_pair']].abs().max())
    print(f'dist196 (B, L) = ({B}, {L}): float32 host baseline {base:.3e}, atol {8 * base:.3e}, kernel max abs error {err:.3e}')
    assert 0 < base < 1e-6
    assert err <= 8 * base, f'dist196: kernel max abs error {err:.3e} > 8 x baseline {base:.3e}'


@pytest.mark.parametrize('max_rel', [32, 5])
@pytest.mark.parametrize('seed,B,L,Lab', SC.PAIR_CASES)
def test_relpos_block(ops, seed, B, L, Lab, max_rel):
    c = SC.make_pair_case(seed, B, L, Lab)
    table = c['proj_rel_pos'] if max_rel == 32 else c['proj_rel_pos5']
    assert table.shape[0] >= 2 * max_rel + 2                 # slot 0 (padding) and slots 1..2 max_rel + 1
    out = nans(B * L * L, 128)
    ops.relpos_block(dev(c['residx']), dev(table), out, B, L, Lab, max_rel)
    ref = SC.relpos_block_reference(c['residx'], table, Lab, max_rel)
    o = out.cpu().view(B, L, L, 128)
    assert torch.equal(o, ref)
    i = torch.arange(L)
    off = (i[:, None] < Lab) != (i[None, :] < Lab)
    assert bool((o[:, off] == 0).all()), 'antibody x antigen pairs: exact zeros'


@pytest.mark.parametrize('n,C,width,col', [(1, 512, 1538, 0), (37, 512, 1538, 514), (257, 7, 19, 3)])
def test_gather_rows(ops, n, C, width, col):
    ge = g(70 + n)
    table = torch.randn(23, C, generator=ge)
    idx = torch.randint(0, 23, (n,), generator=ge)
    idx[0], idx[-1] = 22, 0
    scales = {'none': None, '0/1': (torch.rand(n, generator=ge) > 0.4).float(), 'fractional': torch.rand(n, generator=ge) + 0.25}
    for name, rs in scales.items():
        h = nans(n, width)
        ops.gather_rows(dev(table), dev(idx), h[:, col:col + C], rowscale=None if rs is None else dev(rs))
        ref = table[idx] if rs is None else table[idx] * rs[:, None]
        o = h.cpu()
        assert torch.equal(o[:, col:col + C], ref), f'rowscale {name}'
        assert bool(torch.isnan(o[:, :col]).all()) and bool(torch.isnan(o[:, col + C:]).all()), 'columns outside the window'


# ------------------------------------------------------------------------------------------------------------------
# embed.hip: assemble_seq, assemble_pair, pair_mask
# ------------------------------------------------------------------------------------------------------------------
def _ln64(x, gamma, beta):
    return F.layer_norm(x.double(), (x.shape[-1],), gamma.double(), beta.double(), 1e-5)


@pytest.mark.parametrize('Lab', [0, 29, 37])
def test_assemble_seq(ops, Lab):
    B, L, C, E = 3, 37, 512, 32                    # 111 rows: the last block of 4 rows holds 3
    ge = g(80)
    seq_static = torch.randn(B, L, C, generator=ge)
    aa_table = torch.randn(22, C, generator=ge)
    seq_t = torch.randint(0, 21, (B, L), generator=ge)
    temb = torch.randn(B, E, generator=ge)
    prev = torch.randn(B, L, C + E, generator=ge) * 2 + 0.5
    gamma, beta = torch.randn(C + E, generator=ge), torch.randn(C + E, generator=ge)
    for bcast, has_prev in itertools.product((False, True), (False, True)):
        ss = seq_static[:1] if bcast else seq_static
        out = nans(B, L, C + E)
        ops.assemble_seq(dev(ss), dev(aa_table), dev(seq_t), Lab, dev(temb), dev(prev) if has_prev else None,
                         dev(gamma) if has_prev else None, dev(beta) if has_prev else None, out, B, L, C, E)
        ref = ss.double().expand(B, L, C).clone()
        ref[:, :Lab] += aa_table.double()[seq_t[:, :Lab]]
        ref = torch.cat([ref, temb.double()[:, None].expand(B, L, E)], -1)
        if has_prev:
            ref = ref + _ln64(prev, gamma, beta)
        check(out, ref, 2e-6, f'assemble_seq Lab={Lab} broadcast={bcast} prev={has_prev}')
        if not has_prev:
            assert torch.equal(out.cpu()[:, Lab:, :C], ss.expand(B, L, C)[:, Lab:]), 'antigen rows: the static part unchanged'


def test_assemble_pair(ops):
    B, L, C, E = 3, 37, 128, 32                    # 4107 rows: the last block of 16 rows holds 11, the last block of 4 holds 3
    W, rows = C + 2 * E, B * L * L
    ge = g(81)
    pair_static = torch.randn(B, L, L, C, generator=ge)
    temb = torch.randn(B, E, generator=ge)
    prev = torch.randn(B, L, L, W, generator=ge) * 2 + 0.5
    gamma, beta = torch.randn(W, generator=ge), torch.randn(W, generator=ge)
    pos = torch.randint(0, 15, (B, L, L), generator=ge)
    pos[0, 0, 0], pos[-1, -1, -1] = 14, 0
    pos_table = torch.randn(15, W, generator=ge)
    ln = _ln64(prev, gamma, beta)
    d = dict(temb=guarded(temb, E), prev=guarded(prev, 4 * W), gamma=dev(gamma), beta=dev(beta), pos=guarded(pos, 16), pos_table=dev(pos_table),
             ps={False: guarded(pair_static, 4 * C), True: guarded(pair_static[:1], 4 * C)})
    for bcast, has_prev, has_pos in itertools.product((False, True), (False, True), (False, True)):
        ps = pair_static[:1] if bcast else pair_static
        te = temb.double()[:, None, None].expand(B, L, L, E)
        ref = torch.cat([ps.double().expand(B, L, L, C), te, te], -1)
        if has_prev:
            ref = ref + ln
        if has_pos:
            ref = ref + pos_table.double()[pos]
        args = (d['ps'][bcast], d['temb'], d['prev'] if has_prev else None, d['gamma'] if has_prev else None, d['beta'] if has_prev else None,
                d['pos'] if has_pos else None, d['pos_table'] if has_pos else None)
        tag = f'broadcast={bcast} prev_pair={has_prev} prev_pos={has_pos}'
        # the 192-wide 16-byte-vector kernel
        vbuf = nans(rows * W + 4 * W)
        o_vec = vbuf[:rows * W].view(B, L, L, W)
        assert o_vec.data_ptr() % 16 == 0
        ops.assemble_pair(*args, o_vec, B, L, C, E)
        check(o_vec, ref, 2e-6, f'assemble_pair vector kernel, {tag}')
        assert bool(torch.isnan(vbuf[rows * W:]).all()), 'vector kernel: nothing past the last row'
        # the generic kernel, taken because the fused statistics are asked for
        sbuf, st = nans(rows * W + 4 * W), nans(rows, 2)
        o_st = sbuf[:rows * W].view(B, L, L, W)
        ops.assemble_pair(*args, o_st, B, L, C, E, stats_out=st)
        assert bool(torch.isnan(sbuf[rows * W:]).all()), 'generic kernel: nothing past the last row'
        check(o_st, ref, 2e-6, f'assemble_pair generic kernel (stats), {tag}')
        r2 = ref.view(rows, W)
        check(st[:, 0], r2.mean(-1), 2e-6, f'fused stats mean, {tag}')
        check(st[:, 1], 1 / torch.sqrt(r2.var(-1, unbiased=False) + 1e-5), 2e-6, f'fused stats rstd, {tag}')
        # the generic kernel, taken because the output starts 4 bytes off a 16-byte boundary
        buf = nans(rows * W + 4 * W)
        o_off = buf[1:1 + rows * W].view(B, L, L, W)
        assert o_off.data_ptr() % 16 == 4 and o_off.is_contiguous()
        ops.assemble_pair(*args, o_off, B, L, C, E)
        check(o_off, ref, 2e-6, f'assemble_pair generic kernel (unaligned out), {tag}')
        assert bool(torch.isnan(buf[:1]).all()) and bool(torch.isnan(buf[1 + rows * W:]).all()), 'nothing outside the view'
        check(o_vec, o_st.cpu(), 1e-6, f'vector against generic (stats), {tag}')
        check(o_vec, o_off.cpu(), 1e-6, f'vector against generic (unaligned out), {tag}')
        assert torch.equal(o_st, o_off), 'one kernel, one answer'


@pytest.mark.parametrize('Lp', [37, 40, 64])
def test_pair_mask_padded(ops, Lp):
    B, L = 3, 37
    ge = g(82)
    masks = {'0/1': (torch.rand(B, L, generator=ge) > 0.3).float(), 'fractional': torch.rand(B, L, generator=ge)}
    for name, m in masks.items():
        total = B * L * Lp
        buf = nans(total + 300)
        ops.pair_mask(dev(m), buf[:total], B, L, Lp)
        o = buf.cpu()
        pm = o[:total].view(B, L, Lp)
        assert torch.equal(pm[..., :L], m[:, :, None] * m[:, None, :]), name
        assert bool((pm[..., L:] == 0).all()), 'pad columns'
        assert bool(torch.isnan(o[total:]).all()), 'nothing past B * L * Lp'


# ------------------------------------------------------------------------------------------------------------------
# geometry.hip
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,L', [(3, 131), (1, 1)])
def test_per_residue_geometry(ops, params, cfg, oracle_diffuser, B, L):
    """The checks and tolerances of tests/test_gpu_kernels.py::test_frames_scores_heads at n = 393 residues (blocks 0..3 of the 128-thread
    kernel, blocks 0..1 of the 256-thread ones, both with a partly filled last block) and at n = 1, each also per block of 128 residues.
    rot_score: the reference test bounds the share of rows whose discretised IGSO(3) bucket differs by 0.03; per block the same share
    applies, but a block always may hold one such row (0.03 m < 1 for the 9-row last block, where one bucket mismatch is as legitimate
    as anywhere else)."""
    from oracle import abx_oracle as O
    from abx_amd.model.forward import Packed
    c = SC.make_residue_case(60, B, L)
    n = c['n']
    rig, fixed = c['rigids'], c['fixed']
    fx = dev(fixed.view(-1))
    bufs = [nans(n, k) for k in (4, 3, 4, 3, 9, 4)]
    init_q, init_t, cur_q, cur_t, cur_R, delta_q = bufs
    one = torch.zeros(n, 4)
    one[:, 0] = 1
    for dt_ in (torch.float32, torch.float64):
        for b_ in bufs:
            b_.fill_(NAN)
        ops.frames_init(dev(rig.to(dt_).view(n, 7)), *bufs, n, 10.0)
        check_blocks(cur_R, O.quat_to_rot(rig[..., :4]).reshape(n, 9), 2e-6, 'frames_init R', n)
        check_blocks(cur_t, rig[..., 4:].reshape(n, 3) / 10, 1e-7, 'frames_init t', n)
        assert torch.equal(init_q.cpu(), rig[..., :4].reshape(n, 4)) and torch.equal(cur_q.cpu(), rig[..., :4].reshape(n, 4))
        assert torch.equal(init_t.cpu(), rig[..., 4:].reshape(n, 3)) and torch.equal(delta_q.cpu(), one)
    q, t, R, dq = rig[..., :4].clone(), rig[..., 4:] / 10, O.quat_to_rot(rig[..., :4]), torch.zeros(B, L, 4)
    dq[..., 0] = 1
    dm = (1 - fixed[..., None]).float()
    for upd in c['updates']:
        ops.rigid_update(dev(upd.view(n, 6)), fx, init_q, init_t, cur_q, cur_t, cur_R, delta_q, n, 10.0)
        dq = O.quat_precompose_vec(dq, upd[..., :3])
        q = O.quat_precompose_vec(q, upd[..., :3])
        t = t + torch.einsum('...rd,...d->...r', R, upd[..., 3:])
        q = dm * q + (1 - dm) * rig[..., :4]
        t = dm * t + (1 - dm) * (rig[..., 4:] / 10)
        R = O.quat_to_rot(q)
    check_blocks(cur_q, q.reshape(n, 4), 3e-6, 'rigid_update q', n)
    check_blocks(cur_t, t.reshape(n, 3), 3e-6, 'rigid_update t', n)
    check_blocks(delta_q, dq.reshape(n, 4), 3e-6, 'rigid_update delta', n)
    # scores: fp64 t (loop) and fp32 t (warm-up)
    D = oracle_diffuser
    so3 = D.so3
    q_fin = dm * O.quat_multiply(rig[..., :4], dq) + (1 - dm) * rig[..., :4]
    for tvals in (torch.tensor([0.5050505050505051, 0.02, 0.77], dtype=torch.float64)[:B], torch.tensor([1.0, 0.37, 0.6], dtype=torch.float32)[:B]):
        is32 = tvals.dtype == torch.float32
        rot = nans(n, 3)
        ts = torch.full((n, 3), NAN, device=DEV, dtype=torch.float32 if is32 else torch.float64)
        rigids = nans(n, 7)
        ops.scores(init_q=init_q, init_t=init_t, delta_q=delta_q, cur_t=cur_t, fixed_mask=fx, t=dev(tvals.double()),
                   t_is_f32=int(is32), score_norms=dev(so3._score_norms), num_sigma=1000, num_omega=1000,
                   discrete_sigma=dev(so3.discrete_sigma), discrete_omega=dev(so3.discrete_omega),
                   exp_max_sigma=float(torch.exp(torch.tensor(1.5))), exp_min_sigma=float(torch.exp(torch.tensor(0.1))),
                   min_b=float(torch.tensor(0.1)), bdiff=float(torch.tensor(19.9)), coord_scale=float(torch.tensor(0.1)),
                   position_scale=10.0, rot_score=rot, trans_score=ts, rigids=rigids, B=B, L=L)
        ref_ts = D.calc_trans_score(rig[..., 4:], t * 10, tvals)
        ref_rs = D.calc_quat_score(rig[..., :4], q_fin, tvals)
        assert ref_ts.dtype == ts.dtype
        check_blocks(ts, ref_ts.reshape(n, 3), 3e-6, f'trans_score f32={is32}', n)
        check_blocks(rigids, torch.cat([q_fin, t * 10], -1).reshape(n, 7), 3e-6, 'rigids', n)
        assert bool(torch.isfinite(rot).all())
        # fixed residues have q0^-1 q_t == identity: their rot_score is rounding noise / 2e-6 in the reference too -> diffused residues only
        dif = fixed.view(-1).bool().logical_not()
        ref_rs = ref_rs.reshape(n, 3)
        bad = ((rot.cpu() - ref_rs).abs() > 1e-4 + 1e-4 * ref_rs.abs()).any(-1) & dif
        share = float(bad.sum()) / float(dif.sum())
        assert share <= 0.03, f'rot_score bucket mismatches {share}'
        for s in range(0, n, 128):
            m, k = int(dif[s:s + 128].sum()), int(bad[s:s + 128].sum())
            assert k <= max(1, int(0.03 * m)), f'rot_score: {k} of {m} diffused residues of {s}..{min(s + 128, n) - 1} off'
    # torsions
    un, gt = c['unnorm'], c['gt']
    ang = nans(n, 7, 2)
    ops.torsion_finalize(dev(un), dev(gt), fx, ang, n)
    ref = torch.where(fixed.view(n, 1, 1).bool(), gt, O.l2_normalize(un))
    check_blocks(ang, ref, 2e-6, 'torsion_finalize', n)
    for r_, k_ in c['zero_rows']:
        assert bool((ang[r_, k_].cpu() == 0).all()), f'zero-norm torsion ({r_}, {k_})'
    # sequence head tail: argmax + frames + atoms
    P = Packed(dict(params), DEV)
    logits, seq_t, a37, angles = c['logits'], c['seq_t'], c['a37to14'], c['angles']
    rg = torch.cat([q_fin, t * 10], -1)
    seq0 = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    a14, a37o = nans(n, 14, 3), nans(n, 37, 3)
    ops.seq_head_atoms(dev(logits), fx, dev(seq_t), dev(rg), dev(angles), dev(a37), P.default_frames, P.group_idx, P.lit_pos, seq0, a14, a37o, n)
    s0 = logits.argmax(-1) * (1 - fixed) + seq_t * fixed
    assert torch.equal(seq0.cpu().view(B, L), s0)
    assert int(seq0[c['tie_row']]) == 4, 'a tied maximum: the first index wins'
    fR, ft = O.torsion_angles_to_frames(s0, O.quat_to_rot(rg[..., :4]), rg[..., 4:], angles)
    ref14 = O.frames_to_atom14(s0, fR, ft)
    check_blocks(a14, ref14.reshape(n, 14, 3), 3e-6, 'atom14', n)
    check_blocks(a37o, O.atom14_to_atom37(ref14, a37).reshape(n, 37, 3), 3e-6, 'atom37', n)
    # pLDDT
    lg = c['plddt_logits']
    pl = nans(n)
    ops.plddt(dev(lg), pl, n, 50)
    centers = torch.arange(start=0.01, end=1.0, step=0.02, dtype=torch.float64)
    ref = (torch.softmax(lg.double(), -1) * centers).sum(-1) * 100
    check_blocks(pl, ref, 2e-6, 'plddt', n)
    p_ = c['plddt_row']
    got = float(pl[p_])
    assert np.isfinite(got) and abs(got - float(ref[p_])) <= 2e-6 * float(ref[p_]), f'pLDDT of logits spread over 80: {got} vs {float(ref[p_])}'


@pytest.mark.parametrize('seed,B,L,Lab', SC.PAIR_CASES)
def test_prev_pos_bins(ops, seed, B, L, Lab):
    from oracle import abx_oracle as O
    c, r = SC.make_pair_case(seed, B, L, Lab), SC.pair_reference(seed, B, L, Lab)
    atom37 = O.atom14_to_atom37(c['atom14'], c['a37to14'])
    out = torch.full((B, L, L), -1, dtype=torch.int64, device=DEV)
    res = ops.prev_pos(dev(atom37), dev(c['sq_breaks']), out, B, L)
    assert res.dtype == torch.int64
    o = out.cpu()
    bins, near = r['bins'], r['near_edge']
    for rr, k, side in SC.edge_pairs():
        assert int(o[0, 0, rr]) == k + side and int(o[0, rr, 0]) == k + side, f'pair (0, {rr}) sits {"above" if side else "below"} break {k}'
    assert int(o[0, 0, SC.FAR]) == 14
    for b, t0, rr, k in SC.tie_pairs(B, L):
        assert int(o[b, t0, rr]) == k and int(o[b, rr, t0]) == k, f'pair ({t0}, {rr}) of sample {b} sits ON break {k}: d2 > break is false'
    i = torch.arange(L)
    assert bool((o[:, i, i] == 0).all()), 'the diagonal is bin 0'
    assert torch.equal(o[~near], bins[~near])
    assert int(o.min()) >= 0 and int(o.max()) <= 14
