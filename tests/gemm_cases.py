"""The case table of abx_gemm's tile kernels (csrc/gemm.hip: the exact fp32 kernels; csrc/gemm3.hip: the split-f16 tile kernels), shared by
tests/test_gemm_cases_host.py and tests/test_gpu_gemm_cases.py: one case per dispatch, tile, K and alignment edge, each with the kernel
instantiation it is meant to reach (written by hand; the tests compare it with the library's own plan), seeded float32 inputs, and the
operation in plain torch - `reference` in float64 and `baseline` in float32 are the same text (`_evaluate`): layer_norm, matmul and the
epilogue in the order documented at the head of gemm.hip,

    epi(v) = ((ln(v) + bias[n]) * alpha) -> act -> [out_ln] -> * rowscale[m] -> * (sigmoid?)(gate[m][n]) -> + resid[m][n]

The LayerNorm fold takes the weights already scaled by gamma and beta folded into the bias (gemm.hip, head), so the text normalises the
rows without an affine part and multiplies with the weights as given.  CPU only.  Inputs and references are cached per problem (layout
variants of one problem share them) and never modified.

Memory layout of a case (`layout`): every operand is a strided view (offset, strides in floats) of a flat buffer.  Aligned operands have
their leading dimension rounded up to 4 floats - 16-byte loads and stores with a ragged end; an operand named in `misalign` starts one
float off the boundary and is dense - scalar loads and stores.  The output is a view inside a larger buffer: GUARD_ROWS rows behind the
last one and GUARD_COLS columns beside it (in its own orientation for the transposed store)."""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

# family: the edge family of the case (every family has at least one case of 1024 or more outputs)
Case = collections.namedtuple('Case', 'name M N K batch a_layout b_layout store exact epi misalign offset kernel family')

ALPHA = 0.5
EPS = 1e-5
GUARD_ROWS, GUARD_COLS = 8, 4
P = 1 << 40                       # placeholder "device addresses" of `descriptor`: 16-byte aligned, 1 TiB apart, never followed

# ---- kernel names, as the library's plan spells them --------------------------------------------------------------------------------
X32 = 'gemm_kernel<128, 32, 32, 32, 16, %s, 3>'          # N <= 32
X64S = 'gemm_kernel<128, 64, 32, 64, 16, %s, 3>'         # N <= 64
X64 = 'gemm_kernel<64, 64, 32, 32, 16, %s, 3>'           # fewer than 512 tiles of 128 x 128
X128 = 'gemm_kernel<128, 128, 64, 64, 16, %s, 3>'
X192 = 'gemm_kernel<128, 192, 64, 96, 16, %s, 2>'        # pad192(N) <= pad128(N)
# (A k-contiguous, B n-contiguous, transposed store) of the exact kernels
FLAGS = {('k', 'n'): 'true, true, false', ('k', 'k'): 'true, false, false', ('m', 'n'): 'false, true, false', ('m', 'k'): 'false, false, false'}
TS = 'true, true, true'
S64 = 'gemm3_kernel<64, 128, 32, 64, %d, %s, 4>'         # fewer than 384 tiles and M > 64
S128 = 'gemm3_kernel<128, 128, 32, 128, %d, %s, 4>'
S192 = 'gemm3_kernel<128, 192, 32, 192, %d, %s, 3>'      # N % 128 != 0 and pad192(N) <= pad128(N)
SNARROW = 'gemm3_kernel<128, 32, 32, 32, 0, %s, 6>'      # N <= 32
SOLN = 'gemm3_oln_kernel<128, 128, 32, 128, 4>'

# every instantiation gemm_run and abx_gemm3_dispatch launch without tune bits or environment switches, for the plain, narrow, plane and
# out_ln forms (the single-tile fused forms mlp / dual and the A-stationary kernels have their own tests)
REQUIRED = sorted([x % f for x in (X32, X64S, X64, X128, X192) for f in list(FLAGS.values()) + [TS]] +
                  [s % (amode, 'false') for s in (S64, S128, S192) for amode in (0, 1, 2)] +
                  [s % (0, 'true') for s in (S64, S128, S192)] +
                  [SNARROW % 'false', SNARROW % 'true', SOLN])

CASES = []


def _add(family, M, N, K, kernel, batch=1, a='k', b='n', store='plain', exact=1, epi=(), mis=(), offset=0, tag=''):
    epi, mis = frozenset(epi), frozenset(mis)
    name = f'{family}-{M}x{N}x{K}' + (f'-b{batch}' if batch > 1 else '') + f'-A{a}-B{b}' + ('-T' if store == 'transposed' else '') + f'-e{exact}'
    name += ''.join('+' + e for e in sorted(epi)) + ''.join('-mis' + m for m in sorted(mis)) + (f'-off{offset}' if offset else '') + tag
    CASES.append(Case(name, M, N, K, batch, a, b, store, exact, epi, mis, offset, kernel, family))


FULL = ('bias', 'alpha', 'relu', 'rowscale', 'gate', 'resid')
FULL_SIG = ('bias', 'alpha', 'sigmoid', 'rowscale', 'gate_raw', 'resid')

# ---- exact fp32 kernels (exact = 1) ---------------------------------------------------------------------------------------------------
# skinny and small tiles: the N <= 32 | N <= 64 | launch-size rules, every layout of each
_add('x-small', 1, 1, 1, X32 % FLAGS['k', 'n'])
_add('x-small', 37, 20, 256, X32 % FLAGS['k', 'n'])
_add('x-small', 513, 192, 192, X64 % FLAGS['k', 'n'])
for N_, X_ in ((32, X32), (33, X64S), (64, X64S), (65, X64)):
    for (a_, b_), f_ in FLAGS.items():
        _add('x-small', 130, N_, 52, X_ % f_, a=a_, b=b_)
# K below, at and above one and two k-tiles of 16; aligned rows (16-byte loads with a ragged end) and dense ones (scalar loads)
for K_ in (1, 15, 16, 17, 31, 32, 33):
    _add('x-k', 130, 65, K_, X64 % FLAGS['k', 'n'])
    _add('x-k', 130, 65, K_, X64 % FLAGS['k', 'n'], mis=('A', 'B'))
    _add('x-k', 130, 65, K_, X64 % FLAGS['m', 'k'], a='m', b='k')
# the launch-size rule (512 tiles of 128 x 128) and the wide rule
_add('x-launch', 32640, 256, 16, X64 % FLAGS['k', 'n'])
_add('x-launch', 32641, 256, 16, X128 % FLAGS['k', 'n'])
_add('x-launch', 32641, 192, 16, X192 % FLAGS['k', 'n'])
_add('x-launch', 16385, 448, 16, X128 % FLAGS['k', 'n'])
_add('x-launch', 21889, 384, 17, X192 % FLAGS['k', 'n'])
_add('x-launch', 257, 130, 24, X192 % FLAGS['k', 'n'], batch=128)
# both large tiles in all four layouts, without and with a K tail, and with scalar loads
for N_, X_ in ((256, X128), (192, X192)):
    for (a_, b_), f_ in FLAGS.items():
        for K_ in (16, 17):
            _add('x-layout', 32641, N_, K_, X_ % f_, a=a_, b=b_)
        _add('x-misalign', 32641, N_, 16, X_ % f_, a=a_, b=b_, mis=('A', 'B'))
# transposed store: M = 32641 is no multiple of 4 (a ragged float4 along m)
for M_, N_, K_, X_ in ((130, 45, 52, X64S), (130, 20, 52, X32), (130, 65, 52, X64), (32641, 256, 16, X128), (32641, 192, 16, X192)):
    for mis_ in ((), ('C',)):
        _add('x-ts', M_, N_, K_, X_ % TS, store='transposed', mis=mis_)
        _add('x-ts', M_, N_, K_, X_ % TS, store='transposed', mis=mis_ + (('gate', 'resid') if mis_ else ()), epi=('rowscale', 'gate', 'resid'))
# epilogue order, on one small and one large tile; operands off the boundary
for M_, N_, K_, X_ in ((130, 65, 52, X64), (32641, 192, 16, X192)):
    for epi_ in (FULL, FULL_SIG, ('a_relu',)):
        _add('x-epi', M_, N_, K_, X_ % FLAGS['k', 'n'], epi=epi_)
    _add('x-epi', M_, N_, K_, X_ % FLAGS['k', 'n'], epi=FULL, mis=('C', 'gate', 'resid'))
_add('x-epi', 130, 67, 52, X64 % FLAGS['k', 'n'], epi=FULL, mis=('A', 'B', 'C', 'gate', 'resid'))
# LayerNorm fold: statistics given | inline, both A layouts, rows of mean 0 | 3 | 30 sigma; K = 128 with m-contiguous rows is the tri-mul tail
for M_, N_, K_, X_ in ((300, 192, 192, X64), (32641, 192, 128, X192)):
    for ln_ in ('ln_stats', 'ln_inline'):
        for a_ in ('k', 'm'):
            for off_ in (0, 3, 30):
                _add('x-ln', M_, N_, K_, X_ % FLAGS[a_, 'n'], a=a_, epi=('bias', ln_), offset=off_)

# ---- split-f16 tile kernels (exact = 2, weight planes) -------------------------------------------------------------------------------
W = dict(b='weights', exact=2)
# tile choice
_add('s-tile', 64, 128, 16, S128 % (0, 'false'), **W)
_add('s-tile', 65, 128, 16, S64 % (0, 'false'), **W)
_add('s-tile', 129, 128, 32, S64 % (0, 'false'), **W)
_add('s-tile', 49024, 128, 16, S64 % (0, 'false'), **W)
_add('s-tile', 49025, 128, 16, S128 % (0, 'false'), **W)
_add('s-tile', 130, 192, 16, S192 % (0, 'false'), **W)
_add('s-tile', 130, 190, 16, S192 % (0, 'false'), **W)
for N_ in (448, 768, 65):
    _add('s-tile', 130, N_, 16, S64 % (0, 'false'), **W)
# ring depth: one, two, three, four and twelve k-tiles on each of the three tiles
for K_ in (16, 32, 48, 64, 192):
    _add('s-ring', 64, 128, K_, S128 % (0, 'false'), **W)
    _add('s-ring', 130, 128, K_, S64 % (0, 'false'), **W)
    _add('s-ring', 130, 192, K_, S192 % (0, 'false'), **W)
# rows
for M_ in (1, 63, 64, 65, 127, 128, 129):
    _add('s-rows', M_, 128, 32, (S128 if M_ <= 64 else S64) % (0, 'false'), epi=('bias',), **W)
    _add('s-rows', M_, 192, 32, S192 % (0, 'false'), epi=('bias',), **W)
# narrow tile
for K_ in (16, 192):
    for N_ in (1, 4, 12, 31, 32):
        _add('s-narrow', 130, N_, K_, SNARROW % 'false', epi=('bias', 'alpha'), **W)
        _add('s-narrow', 130, N_, K_, SNARROW % 'true', store='transposed', epi=('bias', 'alpha'), **W)
# row-contiguous A (M % 4 == 0)
_add('s-rowA', 132, 192, 16, S192 % (1, 'false'), a='m', **W)
_add('s-rowA', 132, 128, 16, S64 % (1, 'false'), a='m', **W)
_add('s-rowA', 4, 128, 16, S128 % (1, 'false'), a='m', **W)
_add('s-rowA', 132, 192, 48, S192 % (1, 'false'), a='m', epi=FULL, **W)
# transposed store
_add('s-ts', 130, 128, 16, S64 % (0, 'true'), store='transposed', **W)
_add('s-ts', 130, 192, 16, S192 % (0, 'true'), store='transposed', **W)
_add('s-ts', 64, 128, 16, S128 % (0, 'true'), store='transposed', **W)
_add('s-ts', 130, 128, 48, S64 % (0, 'true'), store='transposed', epi=('rowscale', 'gate', 'resid'), **W)
_add('s-ts', 130, 192, 48, S192 % (0, 'true'), store='transposed', epi=('rowscale', 'gate', 'resid'), mis=('C', 'gate', 'resid'), **W)
# epilogue order on the split tiles
_add('s-epi', 130, 128, 48, S64 % (0, 'false'), epi=FULL, **W)
_add('s-epi', 130, 192, 48, S192 % (0, 'false'), epi=FULL_SIG, mis=('C', 'gate', 'resid'), **W)
_add('s-epi', 64, 128, 48, S128 % (0, 'false'), epi=('a_relu', 'bias', 'relu'), **W)
# plane x plane (the tri-mul contraction): K is the length padded to 16, the pad columns of the images are zero
PL = dict(a='planes', b='planes', exact=2)
_add('s-planes', 64, 64, 64, S128 % (2, 'false'), batch=3, **PL)
_add('s-planes', 65, 65, 80, S64 % (2, 'false'), batch=3, **PL)
_add('s-planes', 97, 97, 112, S64 % (2, 'false'), batch=2, **PL)
_add('s-planes', 352, 352, 352, S192 % (2, 'false'), batch=2, **PL)
# output LayerNorm
_add('s-oln', 130, 128, 192, SOLN, epi=('bias', 'out_ln'), **W)
_add('s-oln', 130, 100, 192, SOLN, epi=('bias', 'out_ln'), **W)
for M_ in (1, 127, 128, 129):
    _add('s-oln', M_, 128, 32, SOLN, epi=('bias', 'out_ln'), **W)
# LayerNorm fold with inline statistics: the shift exists here, the cases prove it
for a_, amode_ in (('k', 0), ('m', 1)):
    for off_ in (0, 30):
        _add('s-ln', 132, 192, 128, S192 % (amode_, 'false'), a=a_, epi=('bias', 'ln_inline'), offset=off_, **W)
        _add('s-ln', 132, 128, 128, S64 % (amode_, 'false'), a=a_, epi=('bias', 'ln_inline'), offset=off_, **W)
# problems the split dispatch turns away: the exact kernel that serves them, the bound of any exact case
_add('s-away', 130, 64, 16, X64S % FLAGS['k', 'n'], **W)
_add('s-away', 130, 33, 16, X64S % FLAGS['k', 'n'], **W)
_add('s-away', 130, 192, 24, X64 % FLAGS['k', 'n'], **W)
_add('s-away', 130, 192, 16, X64 % FLAGS['m', 'n'], a='m', **W)
_add('s-away', 2, 192, 16, X64 % FLAGS['m', 'n'], a='m', **W)
_add('s-away', 130, 192, 16, X64 % FLAGS['k', 'n'], mis=('A',), **W)
# exact = 0: ABX_SPLIT_MIN_TILES = 256 tiles of 128 x 128
_add('s-size', 32640, 128, 16, X64 % FLAGS['k', 'n'], b='weights', exact=0)
_add('s-size', 32641, 128, 16, S64 % (0, 'false'), b='weights', exact=0)

BY_NAME = {c.name: c for c in CASES}


def case_id(c):
    return c.name


def outputs(c):
    return c.batch * c.M * c.N


def _data_key(c):
    """What the inputs and the reference depend on: the problem, not where its operands lie."""
    return (c.M, c.N, c.K, c.batch, tuple(sorted(c.epi)), c.offset, c.a_layout == 'planes')


def case_seed(c):
    return zlib.crc32(repr(_data_key(c)).encode()) & 0x7fffffff


# ---- operand images of the plane x plane contraction ---------------------------------------------------------------------------------
def _host_planes(x, a_side):
    """fp32 tensor (..., rows, K) -> int16 k-tiled f16 operand image (..., K/16, 2, rows, 16) of the plane x plane contraction
    (include/abx_hip.h): A side x' = x / 16, (a0, (x' - a0) 2^11); B side x' = 16 x, (p0, x' - p0); RNE pieces."""
    xs = x / 16 if a_side else x * 16
    p0 = xs.half()
    r = xs - p0.float()
    p1 = (r * 2048).half() if a_side else r.half()
    pl = torch.stack([p0.view(torch.int16), p1.view(torch.int16)], dim=-3)                            # (..., 2, rows, K)
    rows, K = x.shape[-2:]
    assert K % 16 == 0
    pl = pl.reshape(*x.shape[:-2], 2, rows, K // 16, 16)
    return pl.movedim(-2, -4).contiguous()                                                           # (..., K/16, 2, rows, 16)


def _planes_to_f64(pl, a_side):
    """value of an operand image: (..., K/16, 2, rows, 16) int16 -> float64 (..., rows, K)."""
    h = pl.view(torch.float16).double()
    f = (h.select(-3, 0) + h.select(-3, 1) / 2048) * 16 if a_side else (h.select(-3, 0) + h.select(-3, 1)) / 16   # (..., K/16, rows, 16)
    return f.movedim(-3, -2).reshape(*f.shape[:-3], f.shape[-2], -1)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _inputs(key, seed):
    M, N, K, batch, epi, offset, planes = key
    gen = torch.Generator().manual_seed(seed)
    x = {}
    if planes:
        A, Bt = torch.randn(batch, M, K, generator=gen) * 2, torch.randn(batch, N, K, generator=gen)
        A[..., M:], Bt[..., N:] = 0.0, 0.0                     # the pad columns of a length that is no multiple of 16 (K >= M = N)
        x['A_planes'], x['B_planes'] = _host_planes(A, True), _host_planes(Bt, False)
        # the float32 operands of the text: the values the images stand for (22 | 23 significant bits: exact in float32)
        x['A'], x['B'] = _planes_to_f64(x['A_planes'], True).float(), _planes_to_f64(x['B_planes'], False).float().transpose(1, 2)
        assert torch.equal(x['A'].double(), _planes_to_f64(x['A_planes'], True))
    else:
        x['A'] = torch.randn(batch, M, K, generator=gen) + float(offset)
        x['B'] = torch.randn(batch, K, N, generator=gen) / K ** 0.5          # batch > 1: one B per problem (a contraction); else the weights
    if 'bias' in epi:
        x['bias'] = torch.randn(N, generator=gen)
    if 'rowscale' in epi:
        x['rowscale'] = torch.rand(batch, M, generator=gen) * 1.5 + 0.25
    if 'gate' in epi or 'gate_raw' in epi:
        x['gate'] = torch.randn(batch, M, N, generator=gen)
    if 'resid' in epi:
        x['resid'] = torch.randn(batch, M, N, generator=gen)
    if 'ln_stats' in epi or 'ln_inline' in epi:
        x['csum'] = x['B'][0].double().sum(0).float()
    if 'ln_stats' in epi:              # (mean, rstd) per row as the caller passes them: float64 values rounded once
        a = x['A'].double()
        x['stats'] = torch.stack([a.mean(-1), 1.0 / torch.sqrt(a.var(-1, unbiased=False) + EPS)], -1).float().reshape(batch * M, 2)
    if 'out_ln' in epi:
        x['oln_w'], x['oln_b'] = 1 + 0.2 * torch.randn(N, generator=gen), 0.1 * torch.randn(N, generator=gen)
    return x


def inputs(c):
    """The seeded float32 tensors of a case as LOGICAL dense tensors: A (batch, M, K), B (batch, K, N), and by `epi`: bias (N), rowscale
    (batch, M), gate / resid (batch, M, N), csum (N), stats (batch M, 2), oln_w / oln_b (N); plane cases: A_planes / B_planes, the int16
    operand images (batch, K/16, 2, rows, 16), A and B the values they stand for.  Where they lie in memory is `layout`."""
    return _inputs(_data_key(c), case_seed(c))


# ---- the operation: one text, two dtypes -----------------------------------------------------------------------------------------------
def evaluate(epi, x, dtype):
    """epi(A' B) on the logical tensors of `inputs` in `dtype`: (batch, M, N)."""
    t = lambda k: x[k].to(dtype)
    with torch.no_grad():
        A, B = t('A'), t('B')
        if 'a_relu' in epi:
            A = torch.relu(A)
        if 'ln_stats' in epi or 'ln_inline' in epi:
            A = F.layer_norm(A, (A.shape[-1],), None, None, EPS)
        v = torch.matmul(A, B)
        if 'bias' in epi:
            v = v + t('bias')
        if 'alpha' in epi:
            v = v * ALPHA
        if 'relu' in epi:
            v = torch.relu(v)
        if 'sigmoid' in epi:
            v = torch.sigmoid(v)
        if 'out_ln' in epi:
            v = F.layer_norm(v, (v.shape[-1],), t('oln_w'), t('oln_b'), EPS)
        if 'rowscale' in epi:
            v = v * t('rowscale')[..., None]
        if 'gate' in epi:
            v = v * torch.sigmoid(t('gate'))
        if 'gate_raw' in epi:
            v = v * t('gate')
        if 'resid' in epi:
            v = v + t('resid')
    return v


@functools.lru_cache(maxsize=4)
def _reference(key, seed):
    return evaluate(frozenset(key[4]), _inputs(key, seed), torch.float64)


def reference(c):
    """The case in float64, (batch, M, N)."""
    return _reference(_data_key(c), case_seed(c))


def baseline(c):
    """The same text in float32: the reference's own arithmetic."""
    return evaluate(c.epi, inputs(c), torch.float32)


def err(out, c):
    """(max, mean) of |out - float64| over the (batch, M, N) outputs of the case."""
    ref = reference(c)
    d = (out.detach().cpu().reshape(ref.shape).double() - ref).abs()
    return float(d.max()), float(d.mean())


@functools.lru_cache(maxsize=None)
def _baseline_err(key, seed):
    x = _inputs(key, seed)
    d = (evaluate(frozenset(key[4]), x, torch.float32).double() - _reference(key, seed)).abs()
    return float(d.max()), float(d.mean())


def baseline_err(c):
    """err(baseline(c), c), kept for every problem that asked."""
    return _baseline_err(_data_key(c), case_seed(c))


# ---- the bound (derived in tests/test_gpu_gemm_cases.py) --------------------------------------------------------------------------------
K_MAX, K_MEAN = 4.0, 2.0
MEAN_FROM = 1024                  # outputs from which the mean error is asserted as well


def within_bound(c, e, e32, factors=None):
    """e.max <= k_max e32.max, and from MEAN_FROM outputs on e.mean <= k_mean e32.mean; where e32 is 0 the exact value is required."""
    k_max, k_mean = factors or (K_MAX, K_MEAN)
    return e[0] <= k_max * e32[0] and (outputs(c) < MEAN_FROM or e[1] <= k_mean * e32[1])


# ---- memory layout ----------------------------------------------------------------------------------------------------------------------
View = collections.namedtuple('View', 'offset shape strides numel')      # of a flat float32 buffer of `numel` elements


def _c4(n):
    return (n + 3) // 4 * 4


def _view(offset, shape, strides):
    return View(offset, tuple(shape), tuple(strides), offset + 1 + sum((n - 1) * s for n, s in zip(shape, strides)))


def layout(c):
    """{operand: View} of the fp32 operands A, B, C, gate, resid as (batch, rows, cols) LOGICAL views; 'Cbuf': the (batch, rows + guard,
    ld) shape of the buffer C lies in, in its own orientation."""
    b, M, N, K, mis = c.batch, c.M, c.N, c.K, c.misalign
    L = {}
    if c.a_layout != 'planes':
        off = int('A' in mis)
        if c.a_layout == 'k':
            ld = K if off else _c4(K)
            L['A'] = _view(off, (b, M, K), (M * ld, ld, 1))
        else:
            ld = M if off else _c4(M)
            L['A'] = _view(off, (b, M, K), (K * ld, 1, ld))
    if c.b_layout != 'planes':
        off = int('B' in mis)
        if c.b_layout == 'k':
            ld = K if off else _c4(K)
            L['B'] = _view(off, (b, K, N), (N * ld, 1, ld))
        else:
            ld = N if (off or c.b_layout == 'weights') else _c4(N)
            L['B'] = _view(off, (b, K, N), (K * ld, ld, 1))
    rows, cols = (N, M) if c.store == 'transposed' else (M, N)            # in the orientation of the store: cols are contiguous
    t = (lambda s: (s[0], s[2], s[1])) if c.store == 'transposed' else (lambda s: s)
    off = int('C' in mis)
    ld = _c4(cols) + GUARD_COLS + off
    L['C'] = _view(off, (b, M, N), t(((rows + GUARD_ROWS) * ld, ld, 1)))
    L['Cbuf'] = (b, rows + GUARD_ROWS, ld)
    for name in ('gate', 'resid'):
        off = int(name in mis)
        ld = cols + 1 if off else _c4(cols)
        L[name] = _view(off, (b, M, N), t((rows * ld, ld, 1)))
    return L


def descriptor(c):
    """The AbxGemm of the case on placeholder addresses that honour its layout and misalignment (ops.gemm fills the same fields from the
    device tensors), so that abx_gemm_plan can be asked without a GPU."""
    from abx_amd._lib import AbxGemm
    L = layout(c)
    addr = iter(range(P, 64 * P, P))
    at = lambda v: next(addr) + 4 * v.offset
    bs = lambda v: v.strides[0] if c.batch > 1 else 0
    g = AbxGemm()
    g.M, g.N, g.K, g.batch, g.exact, g.alpha = c.M, c.N, c.K, c.batch, c.exact, (ALPHA if 'alpha' in c.epi else 1.0)
    KT = c.K // 16
    if c.a_layout == 'planes':
        g.A_split, g.sA3m, g.sA3p, g.sA3k, g.sA3b = next(addr), 16, 16 * c.M, 32 * c.M, (KT * 32 * c.M if c.batch > 1 else 0)
        g.B_split, g.sB3n, g.sB3p, g.sB3k, g.sB3b = next(addr), 16, 16 * c.N, 32 * c.N, (KT * 32 * c.N if c.batch > 1 else 0)
    else:
        g.A, g.sAb, g.sAm, g.sAk = at(L['A']), bs(L['A']), L['A'].strides[1], L['A'].strides[2]
        g.B, g.sBb, g.sBk, g.sBn = at(L['B']), bs(L['B']), L['B'].strides[1], L['B'].strides[2]
        if c.b_layout == 'weights':
            g.B_split, g.sB3n, g.sB3p, g.sB3k, g.b_f16 = next(addr), 16, 16 * c.N, 32 * c.N, 1
    ts = c.store == 'transposed'
    sm = lambda v: v.strides[2] if ts else v.strides[1]
    g.C, g.sCb, g.c_transposed, g.sCm = at(L['C']), bs(L['C']), int(ts), sm(L['C'])
    if 'ln_stats' in c.epi or 'ln_inline' in c.epi:
        g.ln_csum, g.ln_eps = next(addr), EPS
    if 'ln_stats' in c.epi:
        g.ln_stats, g.sSb = next(addr), c.M
    g.a_relu = int('a_relu' in c.epi)
    g.act = 1 if 'relu' in c.epi else 2 if 'sigmoid' in c.epi else 0
    if 'bias' in c.epi:
        g.bias = next(addr)
    if 'rowscale' in c.epi:
        g.rowscale, g.sRSb = next(addr), c.M
    if 'gate' in c.epi or 'gate_raw' in c.epi:
        g.gate, g.sGb, g.sGm, g.gate_sigmoid = at(L['gate']), bs(L['gate']), sm(L['gate']), int('gate' in c.epi)
    if 'resid' in c.epi:
        g.resid, g.sRb, g.sRm = at(L['resid']), bs(L['resid']), sm(L['resid'])
    if 'out_ln' in c.epi:
        g.out_ln_w, g.out_ln_b, g.out_ln_eps = next(addr), next(addr), EPS
    return g


def plan(g):
    """(return code, kernel name) of abx_gemm_plan for a descriptor."""
    import ctypes
    from abx_amd import _lib
    buf = ctypes.create_string_buffer(128)
    rc = _lib.load().abx_gemm_plan(ctypes.byref(g), None, buf, len(buf))
    return rc, buf.value.decode()
