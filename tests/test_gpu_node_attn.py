"""Kernel-level fp64 parity of the node track at every length edge: abx_seq_attn_fwd (csrc/attention.hip, seq_attn2_kernel) and the IPA core
abx_ipa_pack -> abx_ipa_weights -> abx_ipa_pair (csrc/ipa.hip) against the float64 evaluation of the same operation
(tests/node_attn_cases.py, whose inputs and references are checked on the CPU in tests/test_node_attn_cases_host.py).

The lengths.  seq_attn: below one 4-query wave pass (1, 3, 4, 5); around the 64 keys of a lane slot (63, 64, 65); both sides of every
instantiation threshold (128 | 129, 256 | 257, 384 | 385, 512 | 513 - the last one is the query split as well), the workload's own 352, and
the largest admitted 716; 717, 768 and 800 are refused in front of the launch.  IPA: below, at and above the 12 queries of a workgroup, the
8 / 16 keys of a pair-kernel step, the 64 keys of a wave task (1 .. 65), 96 / 128 / 192, the two sides of the LDS region crossover
(224: sized by the phase-B1 fold, 225: by the logits), the largest admitted 800 and the refused 801; the B split (no full round of 8 samples,
exactly one, one and a rest, two, two and a rest); a sample with every residue masked, one with a single unmasked residue; translations of
10 units with peaked logits.  The projections of the IPA inputs come from ops.gemm (exact fp32), as in test_ipa_core.

The bound.  The yardstick is the reference's own float32 evaluation (NA.baseline), never a kernel: with e = NA.err(GPU output) and
e32 = NA.err(baseline) - both (max, mean) of |out - float64| PER OUTPUT GROUP (seq: the one output; IPA: scalar, points, norms and pair
separately) - every case asserts e.max <= K_MAX * e32.max and e.mean <= K_MEAN * e32.mean for every group.  K_MAX / K_MEAN are the smallest
powers of two at or above the largest measured ratio, capped at 4 / 2: these kernels are plain fp32 FMA arithmetic that differs from the
reference in summation order and in the hardware exponential only; two bits over the reference's own fp32 is the most that justifies.  A
case above the cap is a finding: a kernel fault is fixed, anything else gets its own CASE_FACTORS entry with the derivation next to it.
Where e32 is 0 (the pair group at L = 1: every weight is exactly 1) the bound asks for the exact value.

Measured ratios e / e32 on an MI355X, (max, mean) per group - the table the constants were read from (case ids as `pytest` shows them):

    sequence attention                 max    mean     instantiation, query rows per workgroup
    seq-L1-B2-random20+two             1.060  1.132    seq_attn2_kernel<2, 1024>, 4
    seq-L3-B2-random20+two             1.379  1.024    <2, 1024>, 4
    seq-L4-B2-random20+zero            0.889  1.019    <2, 1024>, 4
    seq-L5-B2-random20+two             0.529  1.057    <2, 1024>, 8
    seq-L63-B2-random20+two            0.855  0.995    <2, 1024>, 64
    seq-L64-B2-random20+zero           0.934  0.824    <2, 1024>, 64
    seq-L65-B2-random20+two            1.167  0.982    <2, 1024>, 68
    seq-L128-B2-random20+zero          1.264  0.780    <2, 1024>, 128
    seq-L129-B2-random20+two           0.953  0.955    <4, 1024>, 132
    seq-L256-B2-random20+zero          1.014  0.861    <4, 1024>, 256
    seq-L257-B2-random20+two           1.228  0.988    <6, 1024>, 260
    seq-sharp-L257-B2-random20+two     1.313  0.980    <6, 1024>, 260
    seq-L352-B2-random20+zero          0.768  0.834    <6, 1024>, 352
    seq-L384-B2-random20+zero          0.513  0.834    <6, 1024>, 384
    seq-L385-B2-random20+two           1.314  0.983    <8, 512>, 388
    seq-L512-B2-random20+zero          0.699  0.925    <8, 512>, 512
    seq-L513-B2-random20+two           0.803  1.018    <12, 256>, 260 (two workgroups per head)
    seq-L716-B1                        1.001  0.991    <12, 256>, 360 (two workgroups per head)

    IPA core                           scalar         points         norms          pair
    ipa-L1-B2                          2.273  1.664   1.575  1.278   1.305  1.305   exact (e32 = e = 0)
    ipa-L11-B2                         1.586  1.341   1.184  1.091   1.071  1.141   1.025  1.139
    ipa-L12-B2                         1.781  1.205   0.965  1.113   0.850  1.153   1.350  1.115
    ipa-L13-B2                         1.518  1.287   1.146  1.129   1.136  1.184   1.361  1.119
    ipa-L16-B2                         1.662  1.288   1.262  1.144   1.272  1.164   1.309  1.213
    ipa-L17-B2                         1.527  1.280   1.290  1.146   1.374  1.154   1.286  1.176
    ipa-L24-B2                         1.430  1.282   1.606  1.122   1.562  1.138   1.006  1.212
    ipa-L25-B2                         1.611  1.257   0.995  1.069   1.054  1.131   1.473  1.146
    ipa-L31-B2                         1.293  1.258   1.595  1.044   1.447  1.050   1.399  1.158
    ipa-L63-B2                         1.723  1.224   1.161  1.003   1.149  1.022   1.334  1.179
    ipa-L64-B2                         1.245  1.238   0.906  1.000   0.931  1.006   1.301  1.170
    ipa-L65-B2                         0.996  1.214   1.237  0.959   0.731  0.992   1.198  1.158
    ipa-L96-B2                         1.472  1.176   0.841  0.911   0.877  0.927   1.778  1.171
    ipa-L128-B2                        1.387  1.186   0.862  0.872   1.145  0.898   1.261  1.169
    ipa-L192-B2                        1.275  1.138   0.780  0.788   0.976  0.810   1.219  1.154
    ipa-L224-B2                        1.224  1.189   0.841  0.947   0.854  0.944   1.213  1.248
    ipa-L225-B2                        1.628  1.183   1.071  0.929   0.967  0.931   1.502  1.247
    ipa-L800-B1                        1.317  1.159   0.815  0.904   0.845  0.892   1.399  1.412
    ipa-L13-B1                         1.853  1.240   1.321  1.089   0.951  1.131   0.927  0.980
    ipa-L13-B7                         1.860  1.284   0.975  1.131   1.329  1.160   1.164  1.152
    ipa-L13-B8                         2.005  1.280   1.488  1.116   2.124  1.159   1.000  1.106
    ipa-L13-B9                         1.645  1.253   0.933  1.111   0.839  1.135   1.166  1.100
    ipa-L13-B16                        1.795  1.281   0.903  1.128   0.888  1.162   1.230  1.139
    ipa-L13-B17                        1.269  1.270   1.138  1.101   1.335  1.121   1.235  1.096
    ipa-L65-B13                        1.142  1.226   0.976  0.986   1.037  1.006   1.241  1.172
    ipa-L65-B2-random15+zero           0.927  1.193   1.246  0.984   0.933  0.989   1.107  1.164
    ipa-L65-B2-random15+single         0.927  1.195   1.246  0.986   0.933  0.992   1.107  1.164
    ipa-sharp-L65-B2                   1.405  1.279   1.416  1.122   1.094  1.148   1.211  1.187
    ipa-sharp-L225-B2                  1.025  1.282   0.826  1.136   1.130  1.150   1.381  1.247

The largest max-ratio is 2.273 and the largest mean-ratio 1.664, both in the scalar group at L = 1: K_MAX = 4, K_MEAN = 2, no case above the
cap, CASE_FACTORS is empty.  The sequence attention alone stays within 1.379 / 1.132, and every IPA group but the scalar one within
2.124 / 1.412.  At L = 1 each softmax weight is exactly 1, so the scalar output there is the v columns of the projection GEMM and nothing
else: its 1.66 x is the exact fp32 MFMA GEMM of ops.gemm (K = 256) against torch's float32 linear, not the attention kernels; the scalar
group's mean falls from there to 1.16 at L = 800 as the key average takes over.  The far-and-sharp inputs raise the float32 error itself four-
to sevenfold (e32 up to 2.4e-5 in the point group) and the kernels' with it: the ratios do not move.

The contracts, as equal bits of an entry point with itself: the IPA scratch (attn_ws, qpack, kpack, vpack, feat) needs no initialisation;
a sample does not depend on its batch (IPA: B = 13 and 17 against B = 1, across the XCD rounds and the rest; seq_attn: B = 2 against 1);
masked keys carry no weight (large finite values in K / V / z / bias at masked keys change no bit of an unmasked query row); abx_ipa_attn is
abx_ipa_weights followed by abx_ipa_pair.
Needs an MI355X: `pytest -m gpu`."""
import math

import pytest
import torch

import node_attn_cases as NA

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 8                   # rows behind the last feat / out row: they keep the NaN they were filled with
K_MAX, K_MEAN = 4.0, 2.0
BIG = 1.0e4                 # what the masked keys hold in test_masked_keys_carry_no_weight
# a case above the cap keeps its own factors here, with the derivation next to it: {(case_id, group): (k_max, k_mean)}
CASE_FACTORS = {}


@pytest.fixture(scope='module')
def ops():
    from abx_amd import ops as _ops, _lib
    lib = _lib.load()
    assert lib.abx_init(0) == 0, lib.abx_last_error_string()
    return _ops


def bits(t):
    return t.contiguous().view(torch.int32)


def scratch(shape, fill=0xFF):
    """A device buffer of float32 whose every BYTE is `fill`: 0xFF reads as NaN, 0 as 0."""
    t = torch.empty(shape, device=DEV, dtype=torch.float32)
    t.view(-1).view(torch.uint8).fill_(fill)
    return t


def assert_bound(c, e, e32):
    """Print one line per group, then assert the bound for every group."""
    bad = []
    for name, _ in NA.groups(c):
        (m, a), (m32, a32) = e[name], e32[name]
        ratio = lambda x, y: (x / y) if y > 0 else (0.0 if x == 0 else math.inf)
        r_max, r_mean = ratio(m, m32), ratio(a, a32)
        print(f'NODE-ATTN {NA.case_id(c)} {name}: e32 max {m32:.3e} mean {a32:.3e}; e max {m:.3e} mean {a:.3e}; ratio max {r_max:.3f} mean {r_mean:.3f}')
        k_max, k_mean = CASE_FACTORS.get((NA.case_id(c), name), (K_MAX, K_MEAN))
        if not (m <= k_max * m32 and a <= k_mean * a32):
            bad.append((name, round(r_max, 3), round(r_mean, 3)))
    assert not bad, bad


# ---- sequence attention ----------------------------------------------------------------------------------------------------------------
def seq_run(ops, c, samples=None, big_at_masked=False):
    """abx_seq_attn_fwd on the samples of case c: (out rows (B L, 544) on the device, guard rows)."""
    x = NA.inputs(c)
    idx = list(range(c.B)) if samples is None else list(samples)
    B, L = len(idx), c.L
    qkv, bias, gate, mask = (x[k][idx].contiguous().to(DEV) for k in ('qkv', 'bias', 'gate', 'mask'))
    if big_at_masked:
        dead = mask == 0                                                        # (B, L)
        qkv[..., NA.D_SEQ:].masked_fill_(dead[:, :, None, None], BIG)           # k | v of the masked keys
        bias.masked_fill_(dead[:, None, None, :], -BIG)
    buf = scratch((B * L + GUARD, NA.H_SEQ * NA.D_SEQ))
    ops.seq_attn(qkv.view(B * L, -1), bias, mask, gate.view(B * L, -1), buf[:B * L], B, L)
    torch.cuda.synchronize()
    return buf[:B * L], buf[B * L:]


@pytest.mark.parametrize('c', NA.SEQ_CASES, ids=NA.case_id)
def test_seq_attn_parity(ops, c):
    """abx_seq_attn_fwd against float64 in units of the reference's own float32 error; the instantiation and the query rows per workgroup
    the length is meant to reach; finite output; the rows behind the last one untouched."""
    assert ops.seq_attn_kernel_name(c.L, with_qblk=True) == NA.SEQ_PLAN[c.L]
    e32 = NA.baseline_err(c)
    out, guard = seq_run(ops, c)
    assert bool(torch.isfinite(out).all()), int((~torch.isfinite(out)).sum())
    assert bool(torch.isnan(guard).all()), 'rows behind the last sample were written'
    assert_bound(c, NA.err(out, c), e32)


@pytest.mark.parametrize('L', NA.SEQ_REFUSED)
def test_seq_attn_refuses_a_length_beyond_the_limit(ops, L):
    """One past the largest admitted length, the end of the 12-keys-per-lane range and a length beyond it: the library's error, the message
    names the limit, and nothing ran - the requirements stand in front of the launch."""
    from abx_amd import _lib
    H, D = NA.H_SEQ, NA.D_SEQ
    qkv, bias, gate = torch.zeros(L, H * 3 * D, device=DEV), torch.zeros(1, H, L, L, device=DEV), torch.zeros(L, H * D, device=DEV)
    mask, out = torch.ones(1, L, device=DEV), scratch((L + GUARD, H * D))
    with pytest.raises(_lib.AbxHipError, match='L <= %d' % NA.SEQ_LMAX):
        ops.seq_attn(qkv, bias, mask, gate, out[:L], 1, L)
    assert (b'L <= %d' % NA.SEQ_LMAX) in _lib.load().abx_last_error_string()
    with pytest.raises(_lib.AbxHipError, match='L <= %d' % NA.SEQ_LMAX):
        ops.seq_attn_kernel_name(L)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def test_seq_attn_sample_does_not_depend_on_its_batch(ops):
    c = NA.Case('seq', 129, 2, ('random20', 'two'), False)
    both, guard = seq_run(ops, c)
    assert bool(torch.isfinite(both).all()) and bool(torch.isnan(guard).all())
    for b in range(c.B):
        one, _ = seq_run(ops, c, samples=[b])
        assert torch.equal(bits(one), bits(both[b * c.L:(b + 1) * c.L])), b


@pytest.mark.parametrize('L', [65, 257])
def test_seq_attn_masked_keys_carry_no_weight(ops, L):
    """k, v and the bias column of every masked key replaced by +-1e4: the bits of the samples that keep a key stay."""
    c = NA.Case('seq', L, 2, ('random20', 'two'), False)
    assert float((1 - NA.inputs(c)['mask'][0]).sum()) > 0
    a, _ = seq_run(ops, c)
    b, guard = seq_run(ops, c, big_at_masked=True)
    assert bool(torch.isfinite(b).all()) and bool(torch.isnan(guard).all())
    diff = bits(a) != bits(b)
    assert not bool(diff.any()), (int(diff.sum()), 'elements moved; first row', int(diff.any(1).nonzero()[0]))


# ---- IPA core --------------------------------------------------------------------------------------------------------------------------
_IPA_DEV = {}


def ipa_dev(sharp):
    """The module's parameters as the kernels take them, built here from the state-dict tensors: the fused projection
    [q_scalar | kv_scalar | q_point_local | kv_point_local] and proj_pair transposed to [K][N], the point weights
    -0.5 sqrt(1 / (3 * 4 * 9 / 2)) softplus(w) (folding.py:59-66, 96)."""
    if sharp not in _IPA_DEV:
        p = NA.ipa_params(sharp)
        names = ('proj_q_scalar', 'proj_kv_scalar', 'proj_q_point_local', 'proj_kv_point_local')
        w_p = math.sqrt(1.0 / (3 * NA.PQK * 9. / 2))
        _IPA_DEV[sharp] = {
            'wt': torch.cat([p[NA.PRE + n + '.weight'] for n in names], 0).t().contiguous().to(DEV),
            'b': torch.cat([p[NA.PRE + n + '.bias'] for n in names]).contiguous().to(DEV),
            'wt_pair': p[NA.PRE + 'proj_pair.weight'].t().contiguous().to(DEV),
            'b_pair': p[NA.PRE + 'proj_pair.bias'].contiguous().to(DEV),
            'pw': (-0.5 * w_p * torch.nn.functional.softplus(p[NA.PRE + 'trainable_point_weights'])).contiguous().to(DEV),
            'w_s': math.sqrt(1.0 / (3 * NA.SQK)), 'w_2d': math.sqrt(1.0 / 3)}
    return _IPA_DEV[sharp]


def ipa_buffers(ops, B, L, fill=0xFF):
    M1 = B * L
    return {'qp': scratch(ops.ipa_qpack_numel(B, L), fill), 'kp': scratch(M1 * NA.H_IPA * 28, fill), 'vp': scratch(M1 * NA.H_IPA * 40, fill),
            'attn_ws': scratch(B * L * L * NA.H_IPA, fill), 'feat': scratch((M1 + GUARD, NA.NFEAT), fill)}


def ipa_run(ops, c, samples=None, fill=0xFF, fused=False, big_at_masked=False):
    """abx_ipa_pack, abx_ipa_weights, abx_ipa_pair (fused: abx_ipa_attn for the last two) on the samples of case c, every scratch and output
    buffer filled with `fill` bytes first.  Returns the buffers; 'out' is feat[:B L], 'guard' the rows behind it."""
    x = NA.inputs(c)
    idx = list(range(c.B)) if samples is None else list(samples)
    B, L = len(idx), c.L
    M1, W = B * L, ipa_dev(c.sharp)
    s, z, mask, Rd, td = (x[k][idx].contiguous().to(DEV) for k in ('s', 'z', 'mask', 'rots', 'trans'))
    s, z, Rd, td = s.view(M1, NA.CS), z.view(M1 * L, NA.CZ), Rd.view(M1, 9), td.view(M1, 3)
    proj = scratch((M1, 1152))
    ops.gemm(s, W['wt'], proj, bias=W['b'])
    bias2d = scratch((M1 * L, NA.H_IPA))
    ops.gemm(z, W['wt_pair'], bias2d, bias=W['b_pair'], alpha=W['w_2d'])
    if big_at_masked:
        dead = mask == 0                                                        # (B, L)
        proj.masked_fill_(dead.view(M1, 1), BIG)                                # the whole projected row: q of a masked residue too
        z.view(B, L, L, NA.CZ).masked_fill_(dead[:, None, :, None], -BIG)
        bias2d.view(B, L, L, NA.H_IPA).masked_fill_(dead[:, None, :, None], BIG)
    u = ipa_buffers(ops, B, L, fill)
    feat = u['feat'][:M1]
    ops.ipa_pack(proj, Rd, td, u['qp'], u['kp'], u['vp'], B, L, W['w_s'])
    if fused:
        ops.ipa_attn(u['qp'], u['kp'], u['vp'], bias2d, z, mask, Rd, td, W['pw'], feat, B, L, attn_ws=u['attn_ws'])
    else:
        ops.ipa_weights(u['qp'], u['kp'], u['vp'], bias2d, mask, Rd, td, W['pw'], u['attn_ws'], feat, B, L)
        ops.ipa_pair(u['attn_ws'], z, feat, B, L)
    torch.cuda.synchronize()
    u.update(out=feat, guard=u['feat'][M1:], mask=mask, B=B, L=L)
    return u


def qpack_pad_rows(u):
    """The pad query rows of the last block of 12 of every sample: Q[b][i / 12][h][(i % 12) / 2][28][i % 2], rows L .. 12 ceil(L / 12) - 1."""
    B, L = u['B'], u['L']
    nib = (L + 11) // 12
    last = u['qp'].view(B, nib, NA.H_IPA, 6, 28, 2)[:, -1]
    rows = [last[:, :, r // 2, :, r % 2] for r in range(L - (nib - 1) * 12, 12)]
    return torch.stack(rows) if rows else None


@pytest.mark.parametrize('c', NA.IPA_CASES, ids=NA.case_id)
def test_ipa_core_parity(ops, c):
    """pack + weights + pair against float64, each of the four output groups in units of the reference's own float32 error; finite output;
    the rows behind the last feature row untouched; the pad query rows of the last Q block zero."""
    e32 = NA.baseline_err(c)
    u = ipa_run(ops, c)
    assert bool(torch.isfinite(u['out']).all()), int((~torch.isfinite(u['out'])).sum())
    assert bool(torch.isnan(u['guard']).all()), 'rows behind the last feature row were written'
    pad = qpack_pad_rows(u)
    assert (pad is None) == (c.L % 12 == 0) and (pad is None or bool((pad == 0).all())), 'pad query rows of the last block'
    assert bool(torch.isfinite(u['attn_ws']).all()) and bool(torch.isfinite(u['qp']).all())
    assert_bound(c, NA.err(u['out'], c), e32)


@pytest.mark.parametrize('L', NA.IPA_REFUSED)
def test_ipa_refuses_a_length_beyond_the_limit(ops, L):
    """One past the largest admitted length, on buffers of the proper size: the library's error in front of any launch, by abx_ipa_weights
    and by abx_ipa_attn; nothing was written."""
    from abx_amd import _lib
    W = ipa_dev(False)
    u = ipa_buffers(ops, 1, L)
    u['qp'].zero_(); u['kp'].zero_(); u['vp'].zero_()
    bias2d, z, mask = torch.zeros(L * L, NA.H_IPA, device=DEV), torch.zeros(L * L, NA.CZ, device=DEV), torch.ones(1, L, device=DEV)
    Rd, td = torch.eye(3, device=DEV).reshape(1, 9).repeat(L, 1), torch.zeros(L, 3, device=DEV)
    with pytest.raises(_lib.AbxHipError, match='L too large'):
        ops.ipa_weights(u['qp'], u['kp'], u['vp'], bias2d, mask, Rd, td, W['pw'], u['attn_ws'], u['feat'][:L], 1, L)
    assert b'abx_ipa_weights: L too large' in _lib.load().abx_last_error_string()
    with pytest.raises(_lib.AbxHipError, match='L too large'):
        ops.ipa_attn(u['qp'], u['kp'], u['vp'], bias2d, z, mask, Rd, td, W['pw'], u['feat'][:L], 1, L, attn_ws=u['attn_ws'])
    torch.cuda.synchronize()
    assert bool(torch.isnan(u['feat']).all()) and bool(torch.isnan(u['attn_ws']).all())


@pytest.mark.parametrize('L', [13, 65])
def test_ipa_scratch_needs_no_initialisation(ops, L):
    """attn_ws, qpack, kpack, vpack and feat full of 0xFF bytes (NaN) give the bits of zero-filled ones, at B = 9: one XCD round and a rest."""
    c = NA.Case('ipa', L, 9, ('random15',) * 9, False)
    res = [ipa_run(ops, c, fill=fill) for fill in (0, 0xFF)]
    assert bool(torch.isfinite(res[1]['out']).all()) and bool(torch.isnan(res[1]['guard']).all()) and bool((res[0]['guard'] == 0).all())
    for name in ('out', 'attn_ws', 'kp', 'vp', 'qp'):
        diff = bits(res[0][name]) != bits(res[1][name])
        assert not bool(diff.any()), (name, int(diff.sum()), 'elements depend on what the buffers held')


def test_ipa_sample_does_not_depend_on_its_batch(ops):
    """L = 65: the samples of a B = 17 call (two XCD rounds and one sample dealt workgroup by workgroup) and of a B = 13 call (one round,
    five dealt) equal the same samples run alone."""
    L = 65
    c = NA.Case('ipa', L, 17, ('random15',) * 17, False)
    b17, b13 = ipa_run(ops, c)['out'], ipa_run(ops, c, samples=range(13))['out']
    assert bool(torch.isfinite(b17).all())
    for b in range(17):
        one = bits(ipa_run(ops, c, samples=[b])['out'])
        assert torch.equal(one, bits(b17[b * L:(b + 1) * L])), ('B = 17', b)
        if b < 13:
            assert torch.equal(one, bits(b13[b * L:(b + 1) * L])), ('B = 13', b)


@pytest.mark.parametrize('L,masks', [(13, ('random15', 'random15')), (65, ('random15', 'single')), (225, ('random15', 'random15'))])
def test_ipa_masked_keys_carry_no_weight(ops, L, masks):
    """The projected row of every masked residue (its k, v and points), z[b, :, j] and the pair bias of every masked key j replaced by +-1e4:
    the bits of every unmasked query row stay (a masked query row attends uniformly to ALL keys, as in the reference: it may move)."""
    c = NA.Case('ipa', L, 2, masks, False)
    a, b = ipa_run(ops, c), ipa_run(ops, c, big_at_masked=True)
    live = (a['mask'].view(-1) != 0)
    assert 0 < int(live.sum()) < live.numel()
    assert bool(torch.isnan(b['guard']).all()) and bool(torch.isfinite(b['out'][live]).all())
    diff = bits(a['out'])[live] != bits(b['out'])[live]
    assert not bool(diff.any()), (int(diff.sum()), 'elements of unmasked query rows moved')


@pytest.mark.parametrize('L,B', [(13, 2), (65, 9)])
def test_ipa_attn_is_weights_then_pair(ops, L, B):
    c = NA.Case('ipa', L, B, ('random15',) * B, False)
    two, one = ipa_run(ops, c), ipa_run(ops, c, fused=True)
    assert bool(torch.isfinite(one['out']).all()) and bool(torch.isnan(one['guard']).all())
    assert torch.equal(bits(one['out']), bits(two['out'])) and torch.equal(bits(one['attn_ws']), bits(two['attn_ws']))
