"""Inputs shared by the kernel-level tests of the embedding and geometry stages (tests/test_stage_cases_host.py,
tests/test_gpu_stage_kernels.py): seeded cases that reach the clamps, the distogram breaks, the masks and the block tails of the
kernels in csrc/embed.hip and csrc/geometry.hip, and float64 restatements of the same operations (abx/model/encoder.py:231-262,
seqformer.py:181-206, common_modules.py:62-83,107-120) on the float32 inputs.  CPU only; every case is built once per argument tuple,
shared between the tests and never modified."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from abx_amd import residue_constants as rc

MIN_BIN, MAX_BIN, NUM_BINS = 3.375, 21.375, 15          # config: embeddings_and_seqformer.prev_pos
EDGE = 1e-3                 # the constructed pairs sit at d2 = s_k (1 -+ EDGE)
NEAR = 2e-4                 # |d2 - s_k| <= NEAR s_k: a pair whose bin a correct fp32 evaluation may put on either side (derivation: pair_reference)
MAX_COORD = 64.0
RULER = [0, 1, 2, 3, 4, 5, 6, 7, 8, 16, 24, 32]         # residue numbers whose differences cover 0..32
N_EDGE = 2 * (NUM_BINS - 1)                               # residues 1..28 of sample 0
FAR = N_EDGE + 1                                          # residue 29 of sample 0: more than 25 A from residue 0
# (seed, B, L, Lab) of the GPU tests: L = 37 and 131 leave partly filled blocks; Lab inside a chain, Lab == L, Lab == 0
PAIR_CASES = [(11, 2, 37, 29), (12, 3, 70, 70), (13, 1, 131, 0)]
TIE_V = (0.0, 1.25, 0.75)     # tie residues: N = CA - TIE_V, C = CA + TIE_V, all three in the plane x = 0 (template) or x = break_k


def tie_layout(B, L):
    """(sample, first residue, breaks) of the tie block: the residue after the template of the block is the template moved by break_k
    along x, for every k of `breaks`.  Each tie pair is near an edge by construction, so the 37-residue case takes every other break
    only: its 2738 pairs leave room for 27 near-edge pairs under the 1 % cap."""
    return B - 1, 0 if B > 1 else FAR + 1, list(range(0, NUM_BINS - 1, 2)) if B * L * L < 5000 else list(range(NUM_BINS - 1))


def tie_pairs(B, L):
    """[(sample, template residue, residue, k)]: the float32 squared pseudo-beta distance of the pair EQUALS the float32 squared break k,
    so the strict `>` of the binning gives bin k and a `>=` gives k + 1."""
    b, t0, ks = tie_layout(B, L)
    return [(b, t0, t0 + 1 + m, k) for m, k in enumerate(ks)]


def sq_breaks():
    """The float32 squared breaks exactly as the model hands them to the kernels (common_modules.py:108-109)."""
    return torch.square(torch.linspace(MIN_BIN, MAX_BIN, steps=NUM_BINS - 1))


def _unit(rng, shape):
    d = rng.normal(size=tuple(shape) + (3,))
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _confined_walk(rng, start, n, step=3.8, radius=58.0):
    """n C-alpha positions after `start`: steps of `step` Angstrom in random directions, redrawn while they would leave the ball of
    `radius` (a step towards the origin always stays inside, so the loop ends)."""
    out, p = [], np.asarray(start, np.float64)
    for _ in range(n):
        for _ in range(64):
            q = p + step * _unit(rng, ())
            if np.linalg.norm(q) <= radius:
                break
        else:
            q = p - step * p / np.linalg.norm(p)
        out.append(q)
        p = q
    return np.array(out).reshape(n, 3)


def _chains(rng, b, L, Lab):
    """chain_id, residx (L,) int32.  Chain 0 (14 residues): the RULER numbers, then 77 (a gap of 45: differences beyond +-32) twice (a
    repeated number).  Chain 1 (12 residues): -3..8, which shares 0..8 with chain 0 and has negative numbers.  Chain 2 (the rest): from
    200, consecutive in sample 0 and with random steps 1..3 in the others."""
    nA, nB = len(RULER) + 2, 12
    nC = L - nA - nB
    assert nC >= 4
    chain = np.concatenate([np.zeros(nA), np.ones(nB), np.full(nC, 2)]).astype(np.int32)
    stepsC = np.ones(nC, np.int64) if b == 0 else rng.integers(1, 4, nC)
    residx = np.concatenate([RULER, [77, 77], np.arange(-3, nB - 3), 200 + np.cumsum(stepsC)]).astype(np.int32)
    return chain, residx


@functools.lru_cache(maxsize=None)
def make_pair_case(seed, B, L, Lab):
    """Inputs of ops.pair_embed_features / ops.relpos_block / ops.prev_pos as CPU tensors (dict, read-only).

    atom14 (B, L, 14, 3) float32: a 3.8 A C-alpha walk inside a ball of 58 A, atom 1 is the C-alpha, the other 13 atoms lie 1.2..2.5 A
    from it, so every coordinate is within MAX_COORD of the origin.  In sample 0, residue 0 is a template; residue 1 + 2k is the
    template translated by sqrt(s_k (1 - EDGE)) and residue 2 + 2k by sqrt(s_k (1 + EDGE)) along random directions (s_k: the float32
    squared break as float64), so pair (0, r) sits just below / above break k; residue FAR is the template translated by 30 A.
    Tie block (tie_layout, tie_pairs): a template whose N, CA, C lie on one line in the plane x = 0 with C - CA == CA - N exactly (the
    cross-product term of its pseudo-beta vanishes, x of the pseudo-beta is x of the C-alpha, y and z are those of the template) and copies moved by the float32 break_k along x: the float32 evaluation
    of d2 is fl(break_k^2), which is the float32 squared break itself.
    chain_id / residx: _chains.  aa (B, L) int64: every sample holds all 23 types.  atom14_exists (B, L, 14) uint8: residues 3, 11, L-1
    lack the C-alpha alone, residues 5 and 17 have the C-alpha alone, residue 7 lacks atom 0, random side-chain atoms are missing.
    Tables: seeded normal float32 of the model's shapes (not its parameters); distcoef has a standard deviation of 8."""
    assert L >= FAR + 8 and 0 <= Lab <= L and (B > 1 or L >= FAR + 20)
    rng = np.random.default_rng(seed)
    sq = sq_breaks()
    s64 = sq.double().numpy()
    x = np.zeros((B, L, 14, 3))
    tb, t0, tks = tie_layout(B, L)
    bk = torch.linspace(MIN_BIN, MAX_BIN, steps=NUM_BINS - 1).double().numpy()
    walk_from = []
    for b in range(B):
        cur = rng.normal(scale=3.0, size=3)
        off = _unit(rng, (L, 14)) * rng.uniform(1.2, 2.5, (L, 14, 1))
        off[:, 1] = 0.0
        p = 0
        if b == 0:
            tmpl = cur[None] + off[0]
            x[0, 0] = tmpl
            for k in range(NUM_BINS - 1):
                x[0, 1 + 2 * k] = tmpl + np.sqrt(s64[k] * (1 - EDGE)) * _unit(rng, ())
                x[0, 2 + 2 * k] = tmpl + np.sqrt(s64[k] * (1 + EDGE)) * _unit(rng, ())
            cur = cur + 30.0 * _unit(rng, ())
            x[0, FAR] = cur[None] + off[0]
            p = FAR + 1
        if b == tb:
            assert p == t0
            cur = np.array([0.0, np.round(cur[1] * 64) / 64, np.round(cur[2] * 64) / 64])
            tmpl = cur[None] + off[p]
            tmpl[0], tmpl[2] = cur - np.array(TIE_V), cur + np.array(TIE_V)
            x[b, p] = tmpl
            for m, k in enumerate(tks):
                x[b, p + 1 + m] = tmpl + np.array([bk[k], 0.0, 0.0])
            cur = cur + np.array([bk[tks[-1]], 0.0, 0.0])
            p += 1 + len(tks)
        walk_from.append(p)
        ca = _confined_walk(rng, cur, L - p)
        x[b, p:] = ca[:, None] + off[p:]
    x = torch.from_numpy(x.astype(np.float32))
    assert float(x.abs().max()) <= MAX_COORD and float(torch.linalg.norm(x, dim=-1).max()) <= MAX_COORD
    chain, residx = zip(*[_chains(rng, b, L, Lab) for b in range(B)])
    aa = np.stack([np.concatenate([rng.permutation(23), rng.integers(0, 23, L - 23)]) for _ in range(B)]).astype(np.int64)
    ex = (rng.random((B, L, 14)) > 0.15).astype(np.uint8)
    ex[:, :, :5] = 1
    for b in range(B):
        sh = 0 if b == 0 else int(rng.integers(1, 6))
        no_ca = [(3 + sh) % L, (11 + sh) % L, L - 1 - sh]
        only_ca = [(5 + sh) % L, (17 + sh) % L]
        ex[b, no_ca, 1] = 0
        ex[b, only_ca] = 0
        ex[b, only_ca, 1] = 1
        ex[b, (7 + sh) % L, 0] = 0
    a37 = torch.as_tensor(rc.restype_atom37_to_atom14)[torch.from_numpy(rng.integers(0, 20, (B, L)))].long()
    tbl = lambda r, c, s=1.0: torch.from_numpy((s * rng.normal(size=(r, c))).astype(np.float32))
    case = dict(B=B, L=L, Lab=Lab, atom14=x, chain_id=torch.from_numpy(np.stack(chain)), residx=torch.from_numpy(np.stack(residx)),
                walk_from=walk_from, aa=torch.from_numpy(aa), atom14_exists=torch.from_numpy(ex), a37to14=a37, sq_breaks=sq,
                aa_pair_embed=tbl(529, 128), relpos_embed=tbl(65, 128), distcoef=tbl(529, 196, 8.0), dgram_embed=tbl(15, 128),
                proj_rel_pos=tbl(66, 128), proj_rel_pos5=tbl(2 * 5 + 1 + 2, 128))
    return case


def pseudo_beta(pos):
    """common_modules.py:62-83 in the dtype of pos (N, CA, C are atoms 0, 1, 2)."""
    N, CA, C = pos[..., 0, :], pos[..., 1, :], pos[..., 2, :]
    b = CA - N
    c = C - CA
    a = torch.cross(b, c, dim=-1)
    return -0.58273431 * a + 0.56802827 * b - 0.54067466 * c + CA


def dist_gauss(case, dtype):
    """encoder.py:248-257 in `dtype`: exp(-softplus(coef[aa_i * 23 + aa_j]) (|x_ia - x_ja'| / 10)^2) * CA_i exists * CA_j exists,
    (B, L, L, 196) with a * 14 + a' fastest."""
    B, L = case['B'], case['L']
    x = case['atom14'].to(dtype)
    aa = case['aa']
    aap = aa[:, :, None] * 23 + aa[:, None, :]
    dist = (torch.linalg.norm(x[:, :, None, :, None] - x[:, None, :, None, :], dim=-1, ord=2) / 10).reshape(B, L, L, -1)
    coef = F.softplus(case['distcoef'].to(dtype)[aap])
    ca = case['atom14_exists'][..., 1].to(dtype)
    return torch.exp(-1 * coef * dist ** 2) * (ca[:, :, None, None] * ca[:, None, :, None])


@functools.lru_cache(maxsize=None)
def pair_reference(seed, B, L, Lab):
    """float64 reference of pair_embed_features on make_pair_case(seed, B, L, Lab) (dict, read-only):
    f_aapair, f_relpos, f_dgram (float32: gathers of float32 rows, f_relpos times the 0/1 same-chain flag, all exact), d_gauss (float64,
    masked), d2 (float64 squared pseudo-beta distances), bins (int64), ca_pair (bool: both C-alpha exist) and near_edge (bool).

    near_edge: |d2 - s_k| <= NEAR * s_k for some break s_k (the float32 value handed to the kernel, as float64).  Coordinates are within
    64 A, so one float32 rounding is at most 2^-18 = 3.8e-6 A; the pseudo-beta takes about 8 operations per component and the difference
    of two doubles that, so a distance d is off by at most about 1e-4 A, which at the smallest break (3.375 A) is 6e-5 relative in
    d2.  NEAR = 2e-4 is about three times that and below EDGE."""
    case = make_pair_case(seed, B, L, Lab)
    aa, chain, residx = case['aa'], case['chain_id'], case['residx']
    aap = aa[:, :, None] * 23 + aa[:, None, :]
    f_aapair = case['aa_pair_embed'][aap]
    same = chain[:, :, None] == chain[:, None, :]
    rel = torch.clamp(residx[:, :, None] - residx[:, None, :], min=-32, max=32) + 32
    f_relpos = case['relpos_embed'][rel.long()] * same[..., None]
    pb = pseudo_beta(case['atom14'].double())
    d2 = torch.sum(torch.square(pb[:, :, None, :] - pb[:, None, :, :]), dim=-1)
    s = case['sq_breaks'].double()
    bins = torch.sum(d2[..., None] > s, dim=-1).long()
    near_edge = ((d2[..., None] - s).abs() <= NEAR * s).any(-1)
    ca = case['atom14_exists'][..., 1].bool()
    return dict(f_aapair=f_aapair, f_relpos=f_relpos, f_dgram=case['dgram_embed'][bins], d_gauss=dist_gauss(case, torch.float64), d2=d2,
                bins=bins, near_edge=near_edge, same_chain=same, rel=rel, ca_pair=ca[:, :, None] & ca[:, None, :])


def relpos_slots(residx, max_rel):
    """seqformer.py:181-190: slot[b, i, j] = clip(residx_j - residx_i + max_rel, 0, 2 max_rel) + 1 (slot 0 is the padding row)."""
    off = residx[:, None, :] - residx[:, :, None]
    return (torch.clip(off + max_rel, min=0, max=2 * max_rel) + 1).long()


def relpos_block_reference(residx, table, Lab, max_rel):
    """The two-block construction of seqformer.py:181-206: antibody x antibody and antigen x antigen blocks, exact zeros elsewhere."""
    B, L = residx.shape
    out = torch.zeros(B, L, L, table.shape[1])
    if Lab > 0:
        out[:, :Lab, :Lab] = table[relpos_slots(residx[:, :Lab], max_rel)]
    if Lab < L:
        out[:, Lab:, Lab:] = table[relpos_slots(residx[:, Lab:], max_rel)]
    return out


def edge_pairs():
    """[(r, k, side)]: residue r of sample 0 sits at d2 = s_k (1 - EDGE) (side 0, bin k) or s_k (1 + EDGE) (side 1, bin k + 1) from
    residue 0."""
    return [(1 + 2 * k + side, k, side) for k in range(NUM_BINS - 1) for side in (0, 1)]


@functools.lru_cache(maxsize=None)
def make_residue_case(seed, B, L):
    """Inputs of the per-residue geometry kernels, drawn as in tests/test_gpu_kernels.py::test_frames_scores_heads (dict of CPU tensors,
    read-only): rigids (B, L, 7), fixed (B, L) int32, three updates (B, L, 6), unnorm / gt (n, 7, 2), logits (B, L, 20), seq_t in 0..20,
    a37to14, angles (B, L, 7, 2), plddt_logits (n, 50); n = B L.  Special rows (flat residue index, clipped to n - 1; all of them
    diffused, i.e. fixed = 0): zero_rows [(residue, torsion)] x 3 have unnorm == (0, 0); tie_row has its maximum logit at indices 4 and
    13; plddt_row has logits spread over 80."""
    ge = torch.Generator().manual_seed(seed)
    n = B * L
    rig = torch.cat([F.normalize(torch.randn(B, L, 4, generator=ge), dim=-1), torch.randn(B, L, 3, generator=ge) * 10], -1)
    fixed = (torch.rand(B, L, generator=ge) > 0.4).int()
    upd = [torch.randn(B, L, 6, generator=ge) * 0.3 for _ in range(3)]
    un, gt = torch.randn(n, 7, 2, generator=ge), torch.randn(n, 7, 2, generator=ge)
    logits = torch.randn(B, L, 20, generator=ge)
    seq_t = torch.randint(0, 21, (B, L), generator=ge)
    a37 = torch.as_tensor(rc.restype_atom37_to_atom14)[torch.randint(0, 20, (B, L), generator=ge)].long()
    ang = torch.randn(B, L, 7, 2, generator=ge)
    ang = ang / torch.sqrt(torch.sum(ang * ang, dim=-1, keepdim=True) + 1e-12)
    lg = torch.randn(n, 50, generator=ge)
    clip = lambda r: min(r, n - 1)
    zero_rows = [(clip(5), 0), (clip(200), 3), (clip(n - 2), 6)]
    tie_row, plddt_row = clip(389), clip(300)
    for r, k in zero_rows:
        un[r, k] = 0.0
    lf = logits.view(n, 20)
    top = float(lf[tie_row].max()) + 1.0
    lf[tie_row, 4] = top
    lf[tie_row, 13] = top
    lg[plddt_row] = torch.linspace(-40.0, 40.0, 50)[torch.randperm(50, generator=ge)]
    for r in [r for r, _ in zero_rows] + [tie_row]:
        fixed.view(-1)[r] = 0
    return dict(B=B, L=L, n=n, rigids=rig, fixed=fixed, updates=upd, unnorm=un, gt=gt, logits=logits, seq_t=seq_t, a37to14=a37, angles=ang,
                plddt_logits=lg, zero_rows=zero_rows, tie_row=tie_row, plddt_row=plddt_row)
