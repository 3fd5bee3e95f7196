"""Inputs and references shared by the kernel-level tests of the node track (tests/test_node_attn_cases_host.py,
tests/test_gpu_node_attn.py): the sequence attention with pair bias (abx_seq_attn_fwd) and the IPA core (abx_ipa_pack, abx_ipa_weights,
abx_ipa_pair) on seeded inputs at every length edge of their kernels.  The float64 `reference` and the float32 `baseline` of a case are the
same plain torch text evaluated in two dtypes: oracle._attention times the sigmoid gate for the sequence attention, the body of
oracle.ipa_attention up to (without) final_proj for the IPA core.  CPU only.  A case is built once, shared between the tests and never
modified."""
import collections
import functools
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from abx_amd import synthetic
from oracle import abx_oracle as O

PRE = O.P_IPA + 'attention_module.'
H_SEQ, D_SEQ = 32, 17
H_IPA, SQK, SV, PQK, PV, CZ, CS = 12, 16, 16, 4, 8, 128, 256
NFEAT = 2112
# the feature row of the IPA core: [scalar 192 | points '(r n)' 288 | norms 96 | pair 1536]
IPA_GROUPS = (('scalar', slice(0, 192)), ('points', slice(192, 480)), ('norms', slice(480, 576)), ('pair', slice(576, 2112)))
SEQ_GROUPS = (('out', slice(0, H_SEQ * D_SEQ)),)

# ---- case lists ---------------------------------------------------------------------------------------------------------------------
# family 'seq' | 'ipa'; masks: one pattern name per sample (mask_row); sharp: the "far and sharp" inputs of the family (below)
Case = collections.namedtuple('Case', 'family L B masks sharp')


def _seq(L, second, B=2, sharp=False):
    return Case('seq', L, B, ('random20', second)[:B], sharp)


def _ipa(L, B=2, masks=None, sharp=False):
    return Case('ipa', L, B, tuple(masks) if masks else ('random15',) * B, sharp)


# Sequence attention, H = 32, D = 17.  Sample 0 has a random 20 % of its keys masked; sample 1 has every key masked but two ('two', the
# pattern of test_seq_attn) - or every key ('zero') in one case of each edge group.  The edge groups, by the unit whose multiple they sit on:
# below one 4-query wave pass; the 64 keys of a lane slot; the 2 | 4, 4 | 6, 6 | 8 and 8 | 12 instantiation thresholds (128, 256, 384, 512:
# 512 is the query split as well); the workload's own L = 352; the largest admitted length (one sample: its group's 'zero' sample is L = 512's).
SEQ_CASES = [_seq(1, 'two'), _seq(3, 'two'), _seq(4, 'zero'), _seq(5, 'two'),
             _seq(63, 'two'), _seq(64, 'zero'), _seq(65, 'two'),
             _seq(128, 'zero'), _seq(129, 'two'),
             _seq(256, 'zero'), _seq(257, 'two'), _seq(257, 'two', sharp=True),
             _seq(352, 'zero'),
             _seq(384, 'zero'), _seq(385, 'two'),
             _seq(512, 'zero'), _seq(513, 'two'),
             _seq(716, None, B=1)]
# what each length is meant to reach: (instantiation - keys per lane, threads -, query rows per workgroup: below L where the queries are split).
# Written down by hand from the lengths' purpose; the tests compare it with the library's own plan (ops.seq_attn_kernel_name).
_K = 'seq_attn2_kernel<%d, %d>'
SEQ_PLAN = {1: (_K % (2, 1024), 4), 3: (_K % (2, 1024), 4), 4: (_K % (2, 1024), 4), 5: (_K % (2, 1024), 8),
            63: (_K % (2, 1024), 64), 64: (_K % (2, 1024), 64), 65: (_K % (2, 1024), 68),
            128: (_K % (2, 1024), 128), 129: (_K % (4, 1024), 132),
            256: (_K % (4, 1024), 256), 257: (_K % (6, 1024), 260),
            352: (_K % (6, 1024), 352),
            384: (_K % (6, 1024), 384), 385: (_K % (8, 512), 388),
            512: (_K % (8, 512), 512), 513: (_K % (12, 256), 260),
            716: (_K % (12, 256), 360)}
SEQ_REFUSED = (717, 768, 800)         # 717, 768: the LDS-resident K / V no longer fit; 800: more than 12 keys per lane
SEQ_LMAX = 716

# IPA core.  ipa_weights_kernel: 12 queries per workgroup, 64-key wave tasks, 12 key groups x 4 keys per round in phase B1; ipa_pair_kernel:
# 8 keys per step, two steps in flight; 224 | 225: the LDS region is sized by the B1 fold | by the logits; 800: the largest admitted length.
IPA_CASES = [_ipa(L) for L in (1, 11, 12, 13, 16, 17, 24, 25, 31, 63, 64, 65, 96, 128, 192, 224, 225)]
IPA_CASES += [_ipa(800, B=1)]
# the B split of ipa_weights_kernel: full rounds of 8 samples pinned to the XCDs, the rest dealt workgroup by workgroup
IPA_CASES += [_ipa(13, B=B) for B in (1, 7, 8, 9, 16, 17)] + [_ipa(65, B=13)]
IPA_CASES += [_ipa(65, masks=('random15', 'zero')),                      # a sample with every residue masked
              _ipa(65, masks=('random15', 'single')),                    # a sample with one unmasked residue
              _ipa(65, sharp=True), _ipa(225, sharp=True)]
IPA_REFUSED = (801,)
IPA_LMAX = 800

SHARP_SEQ = 4.0         # seq: q and the pair bias x 4 - a peaked softmax
SHARP_IPA_TRANS = 10.0  # ipa: translations of about 10 position units (3 otherwise) ...
SHARP_IPA_Q = 4.0       # ... the scalar queries x 4 and both point projections x 2: (q.k) and |q_pt - k_pt|^2 both x 4 in the frames' own scale
SHARP_IPA_PT = 2.0


def case_id(c):
    m = '' if all(x.startswith('random') for x in c.masks) else '-' + '+'.join(c.masks)
    return f'{c.family}{"-sharp" if c.sharp else ""}-L{c.L}-B{c.B}{m}'


def case_seed(c):
    return 9001 + 100000 * (c.family == 'ipa') + 16 * c.L + c.B


def mask_row(pattern, L, gen):
    """float 0/1 (L,): 'random20' / 'random15' about that share of zeros, 'two' every residue masked but the first two (test_seq_attn),
    'zero' every residue masked (the reference REPLACES masked logits by finfo.min: uniform weights over all L keys), 'single' one
    unmasked residue in the middle."""
    if pattern.startswith('random'):
        return (torch.rand(L, generator=gen) > int(pattern[6:]) / 100.0).float()
    m = torch.zeros(L)
    if pattern == 'two':
        m[:2] = 1.0
    elif pattern == 'single':
        m[L // 2] = 1.0
    else:
        assert pattern == 'zero', pattern
    return m


@functools.lru_cache(maxsize=None)
def ipa_params(sharp=False):
    """The float32 tensors of the IPA attention module from synthetic.random_state_dict(sd_shapes, seed=7) - the `params` fixture of
    conftest.py - without final_proj.  sharp: see SHARP_IPA_*."""
    keys = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sd_keys.json')))
    shapes = collections.OrderedDict((k, tuple(s)) for k, s in keys)
    p = {k: v for k, v in synthetic.random_state_dict(shapes, seed=7).items() if k.startswith(PRE) and 'final_proj' not in k}
    if sharp:
        for name, f in (('proj_q_scalar', SHARP_IPA_Q), ('proj_q_point_local', SHARP_IPA_PT), ('proj_kv_point_local', SHARP_IPA_PT)):
            for leaf in ('.weight', '.bias'):
                p[PRE + name + leaf] = p[PRE + name + leaf] * f
    return p


@functools.lru_cache(maxsize=3)
def inputs(c):
    """The float32 inputs of a case.  seq: qkv (B, L, 32, 51) with the per-head layout [q | k | v], bias (B, 32, L, L), gate (B, L, 544),
    mask (B, L).  ipa: s (B, L, 256), z (B, L, L, 128), rots (B, L, 3, 3), trans (B, L, 3), mask (B, L), p (module parameters)."""
    gen = torch.Generator().manual_seed(case_seed(c))
    B, L = c.B, c.L
    if c.family == 'seq':
        qkv = torch.randn(B, L, H_SEQ, 3 * D_SEQ, generator=gen)
        bias = torch.randn(B, H_SEQ, L, L, generator=gen)
        gate = torch.randn(B, L, H_SEQ * D_SEQ, generator=gen)
        if c.sharp:
            qkv[..., :D_SEQ] *= SHARP_SEQ
            bias *= SHARP_SEQ
        mask = torch.stack([mask_row(m, L, gen) for m in c.masks])
        return {'qkv': qkv, 'bias': bias, 'gate': gate, 'mask': mask}
    s = torch.randn(B, L, CS, generator=gen)
    z = torch.randn(B, L, L, CZ, generator=gen)
    rots = O.quat_to_rot(F.normalize(torch.randn(B, L, 4, generator=gen), dim=-1))
    trans = torch.randn(B, L, 3, generator=gen) * (SHARP_IPA_TRANS if c.sharp else 3.0)
    mask = torch.stack([mask_row(m, L, gen) for m in c.masks])
    return {'s': s, 'z': z, 'rots': rots, 'trans': trans, 'mask': mask, 'p': ipa_params(c.sharp)}


# ---- the references: one text, two dtypes ----------------------------------------------------------------------------------------------
def seq_attn_core(qkv, bias, gate, mask):
    """oracle._attention times the sigmoid gate, as tests/test_gpu_kernels.py test_seq_attn builds it: (B, L, 544)."""
    t = qkv.permute(0, 2, 1, 3)[:, None]
    q, k, v = torch.chunk(t, 3, dim=-1)
    return O._attention(q, k, v, bias, mask[:, None, :], D_SEQ)[:, 0] * torch.sigmoid(gate)


def ipa_core(p, s, z, mask, rots, trans, rows=128):
    """The body of oracle.ipa_attention (InvariantPointAttention.forward, folding.py:47-132) up to, but without, final_proj: the concat
    [scalar 192 | points 288 | norms 96 | pair 1536] (B, L, 2112).  Query rows are taken `rows` at a time - every row is its own softmax, so
    the chunking changes no operation on any element - which bounds the (B, i, j, 12, 4, 3) distance tensor at L = 800."""
    H, sqk, sv, pqk, pv = H_IPA, SQK, SV, PQK, PV
    B, L, _ = s.shape
    w_s = np.sqrt(1.0 / (3 * max(sqk, 1) * 1.))
    w_p = np.sqrt(1.0 / (3 * max(pqk, 1) * 9. / 2))
    w_2d = np.sqrt(1.0 / 3)
    q_s = O.lin(p, PRE + 'proj_q_scalar', s).reshape(B, L, H, sqk).permute(0, 2, 1, 3)
    kv_s = O.lin(p, PRE + 'proj_kv_scalar', s).reshape(B, L, H, sqk + sv).permute(0, 2, 1, 3)
    k_s, v_s = kv_s[..., :sqk], kv_s[..., sqk:]
    q_p = O.lin(p, PRE + 'proj_q_point_local', s).reshape(B, L, 3, H * pqk).transpose(-1, -2)
    kv_p = O.lin(p, PRE + 'proj_kv_point_local', s).reshape(B, L, 3, H * (pqk + pv)).transpose(-1, -2)
    q_g = O.rigid_apply(rots, trans, q_p).reshape(B, L, H, pqk, 3)
    kv_g = O.rigid_apply(rots, trans, kv_p).reshape(B, L, H, pqk + pv, 3)
    k_g, v_g = kv_g[:, :, :, :pqk], kv_g[:, :, :, pqk:]
    pw = -0.5 * w_p * F.softplus(p[PRE + 'trainable_point_weights'])
    out = []
    for i0 in range(0, L, rows):
        r = slice(i0, min(L, i0 + rows))
        n = r.stop - r.start
        logits = torch.einsum('bhic,bhjc->bhij', q_s[:, :, r] * w_s, k_s)
        d2 = torch.sum(torch.square(q_g[:, r, None] - k_g[:, None]), dim=[-1, -2])                     # (B,i,j,H)
        logits = logits + (pw * d2).permute(0, 3, 1, 2)
        logits = logits + w_2d * O.lin(p, PRE + 'proj_pair', z[:, r]).permute(0, 3, 1, 2)
        m2 = (mask[:, r, None] * mask[:, None, :])[:, None]
        logits = logits.masked_fill(~m2.bool(), torch.finfo(logits.dtype).min)
        a = F.softmax(logits, dim=-1)
        o_s = torch.matmul(a, v_s).permute(0, 2, 1, 3).reshape(B, n, H * sv)
        o_pg = torch.einsum('bhij,bjhnr->bhinr', a, v_g).permute(0, 2, 1, 3, 4).reshape(B, n, H * pv, 3)
        o_pl = O.rigid_invert_apply(rots[:, r], trans[:, r], o_pg)
        o_pts = o_pl.transpose(-1, -2).reshape(B, n, 3 * H * pv)                                       # '(r n)'
        o_norm = torch.sqrt(torch.sum(torch.square(o_pl), dim=-1) + 1e-8)
        o_2d = torch.einsum('bhij,bijc->bhic', a, z[:, r]).permute(0, 2, 1, 3).reshape(B, n, -1)
        out.append(torch.cat([o_s, o_pts, o_norm, o_2d], dim=-1))
    return torch.cat(out, dim=1)


def _evaluate(c, dtype):
    x = inputs(c)
    with torch.no_grad():
        if c.family == 'seq':
            return seq_attn_core(x['qkv'].to(dtype), x['bias'].to(dtype), x['gate'].to(dtype), x['mask'].to(dtype))
        p = {k: v.to(dtype) for k, v in x['p'].items()}
        return ipa_core(p, x['s'].to(dtype), x['z'].to(dtype), x['mask'].to(dtype), x['rots'].to(dtype), x['trans'].to(dtype))


@functools.lru_cache(maxsize=None)
def reference(c):
    """The case in float64: (B, L, 544) | (B, L, 2112).  Kept for every case that asked (the largest is 13 MB)."""
    return _evaluate(c, torch.float64)


def baseline(c):
    """The same text in float32: the reference's own arithmetic."""
    return _evaluate(c, torch.float32)


def groups(c):
    return SEQ_GROUPS if c.family == 'seq' else IPA_GROUPS


def err(out, c, samples=None):
    """{group: (max, mean) of |out - float64|} per OUTPUT GROUP - for the IPA core the four groups separately, never the concat as one: the
    pair group's magnitude would hide the others.  samples: the samples of the case that `out` holds (default: all)."""
    ref = reference(c)
    if samples is not None:
        ref = ref[samples]
    d = (out.detach().cpu().reshape(ref.shape).double() - ref).abs()
    return {name: (float(d[..., sl].max()), float(d[..., sl].mean())) for name, sl in groups(c)}


@functools.lru_cache(maxsize=None)
def baseline_err(c):
    """err(baseline(c), c), kept for every case that asked."""
    return err(baseline(c), c)


def uniform_average(c, b):
    """What a fully masked sample b must give, in float64, for the groups that are a plain mean over the keys: seq 'out' = mean_k v times the
    gate; ipa 'scalar' = mean_j v_scalar, 'pair' = mean_j z[b, i, j] for every head."""
    x = inputs(c)
    if c.family == 'seq':
        v = x['qkv'][b, :, :, 2 * D_SEQ:].double().mean(0)                                            # (H, D)
        return {'out': v.reshape(1, -1) * torch.sigmoid(x['gate'][b].double())}
    p = {k: v.double() for k, v in x['p'].items()}
    kv = O.lin(p, PRE + 'proj_kv_scalar', x['s'][b].double()).reshape(c.L, H_IPA, SQK + SV)
    return {'scalar': kv[..., SQK:].mean(0).reshape(1, -1).expand(c.L, -1),
            'pair': x['z'][b].double().mean(1)[:, None, :].expand(-1, H_IPA, -1).reshape(c.L, -1)}
