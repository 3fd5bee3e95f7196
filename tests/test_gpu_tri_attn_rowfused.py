"""Row-fused triangle attention (csrc/attention.hip tri_attn8_rowfused_kernel, abx_tri_attn_rowfused_fwd): q | k | v of a pair row are
projected inside the attention workgroup of that row.  The yardstick is the route it replaces - the LayerNorm-folded split-f16 projection
(ops.gemm, exact=2) followed by ops.tri_attn on the projected rows - and the demand is equal bits.  Needs an MI355X: `pytest -m gpu`."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
H, D, C = 4, 48, 192


@pytest.fixture(scope='module')
def ops():
    from abx_amd import ops as _ops, _lib
    lib = _lib.load()
    assert lib.abx_init(0) == 0, lib.abx_last_error_string()
    return _ops


def g(seed):
    return torch.Generator().manual_seed(seed)


def _packs(ops, seed, k_bias_shift=None):
    """qkv / gate / pair / out LinearPacks of a TriangleAttention block from seeded weights (LayerNorm folded as model/forward.py does)."""
    ge = g(seed)
    W = lambda n, k=C: (torch.randn(n, k, generator=ge) / k ** 0.5).to(DEV)
    b = lambda n: (torch.randn(n, generator=ge) * 0.3).to(DEV)
    ln = ((1.0 + 0.2 * torch.randn(C, generator=ge)).to(DEV), (0.1 * torch.randn(C, generator=ge)).to(DEV))
    bk = b(C)
    if k_bias_shift is not None:
        bk[k_bias_shift[0]] = k_bias_shift[1]
    qkv = ops.LinearPack([(W(C), b(C), 0), (W(C), bk, 0), (W(C), b(C), 0)], C, ln=ln)
    gate = ops.LinearPack([(W(C), b(C), 0)], C, ln=ln)
    pair = ops.LinearPack([(W(4), None, 0)], C, ln=ln)
    out = ops.LinearPack([(W(C), b(C), 0)], C, permute_k16=True)
    return qkv, gate, pair, out


def _inputs(L, B, seed, masked=True):
    ge = g(seed)
    Lp = (L + 3) // 4 * 4
    z = (torch.randn(B, L * L, C, generator=ge) * 1.3 + 0.2).to(DEV)
    bias = torch.zeros(B, H, L, Lp)
    bias[..., :L] = torch.randn(B, H, L, L, generator=ge) * 150.0          # (accumulator units: ABX_TRI_BIAS_LOG2 x an O(1) pair bias)
    mask = torch.ones(B, L)
    if masked:
        mask = (torch.rand(B, L, generator=ge) > 0.15).float()
        mask[:, 0] = 1
        mask[0, L - 5:] = 0
    return z, bias.to(DEV), mask.to(DEV)


def _two_launches(ops, qkv, z, bias, mask, B, L, per_row):
    """Today's route: q | k | v rows through the split-f16 GEMM with the folded LayerNorm, then the attention on them."""
    M = B * L * L
    rows = torch.full((M, 3 * C), float('nan'), device=DEV)
    ops.gemm(z.view(M, C), qkv.Wt, rows, bias=qkv.bias, ln=(None, qkv.csum), B3=qkv.planes, exact=2, range_class='tri_attn')
    o = torch.full((M, C), float('nan'), device=DEV)
    ops.tri_attn(rows, bias, mask, o, B, L, per_row, bias_is_qk=True, bias_log2=True)
    return o, rows


def _fused(ops, rowp, z, bias, mask, B, L, per_row, **kw):
    o = torch.full((B * L * L, C), float('nan'), device=DEV)
    ops.tri_attn(z.view(B * L * L, C), bias, mask, o, B, L, per_row, bias_is_qk=True, bias_log2=True, rowpack=rowp, **kw)
    return o


@pytest.mark.parametrize('per_row', [True, False])
@pytest.mark.parametrize('L,B', [(97, 4), (120, 3), (230, 2), (261, 1), (352, 2)])
def test_fused_equals_projection_plus_attention(ops, L, B, per_row):
    """Both orientations, masked keys, rows not divisible by 32 (97, 120, 230, 261) and by 4 (97, 230, 261), both slot orders: the output of
    the fused entry equals, bit for bit, gemm + tri_attn on the same z, packs and bias."""
    qkv = _packs(ops, 5000 + L)[0]
    rowp = ops.TriRowPack(qkv)
    z, bias, mask = _inputs(L, B, 5100 + L)
    assert ops.tri_attn_kernel_name(L, exact=False, rowfused=True) == 'tri_attn8_rowfused_kernel'
    ref, _ = _two_launches(ops, qkv, z, bias, mask, B, L, per_row)
    assert torch.isfinite(ref).all()
    for order in (0, 1):
        o = _fused(ops, rowp, z, bias, mask, B, L, per_row, slot_order=order)
        d = (o - ref).abs()
        print(f'L={L} B={B} per_row={per_row} order={order}: max |fused - two launches| = {float(d.max()):.3e}, '
              f'differing elements = {int((o != ref).sum())} of {o.numel()}')
        assert torch.equal(o, ref), (L, B, per_row, order, float(d.max()))


@pytest.mark.parametrize('L,B', [(120, 3), (352, 1)])
def test_fused_without_keymask(ops, L, B):
    """keymask = None (AbxTriAttn.keymask == NULL, as abx_tri_attn_fwd admits it): the workgroup's issuing wave then has no key-mask loads in
    its queue - its counted waits for the weight groups must not depend on that.  Equal bits with the two launches, both orientations, both
    slot orders, and equal to an all-ones mask."""
    qkv = _packs(ops, 5500 + L)[0]
    rowp = ops.TriRowPack(qkv)
    z, bias, _ = _inputs(L, B, 5501 + L, masked=False)
    ones = torch.ones(B, L, device=DEV)
    for per_row in (True, False):
        ref, _ = _two_launches(ops, qkv, z, bias, None, B, L, per_row)
        assert torch.isfinite(ref).all()
        for order in (0, 1):
            o = _fused(ops, rowp, z, bias, None, B, L, per_row, slot_order=order)
            print(f'L={L} B={B} per_row={per_row} order={order} no keymask: differing elements = {int((o != ref).sum())} of {o.numel()}')
            assert torch.equal(o, ref), (L, per_row, order, float((o - ref).abs().max()))
        assert torch.equal(_fused(ops, rowp, z, bias, ones, B, L, per_row), ref)


def test_range_contract(ops):
    """A z element beyond the split range of the projection's A operand (2^20) turns q, k and v of its pair position into NaN: every query of
    that row is NaN in every head (the key is shared), nothing else, and the tri_attn range bit is set - by the two launches and by the fused
    kernel alike.  A k channel beyond the range of the attention's key planes (4095: here through the projection's bias) is NaN in its head
    only, in every row."""
    L, B = 128, 2
    word = ops.range_word(DEV)
    T = ops.RANGE_TAGS
    z, bias, mask = _inputs(L, B, 5200, masked=False)
    qkv = _packs(ops, 5201)[0]
    rowp = ops.TriRowPack(qkv)
    word.zero_()
    clean = _fused(ops, rowp, z, bias, mask, B, L, True)
    assert int(word.item()) == 0 and torch.isfinite(clean).all()
    z2 = z.clone()
    z2.view(B, L, L, C)[1, 5, 9, 17] = 3.0e6
    word.zero_()
    ref, _ = _two_launches(ops, qkv, z2, bias, mask, B, L, True)
    assert int(word.item()) == T['tri_attn']
    word.zero_()
    o = _fused(ops, rowp, z2, bias, mask, B, L, True)
    assert int(word.item()) == T['tri_attn']
    nan = ~torch.isfinite(o)
    expect = torch.zeros_like(nan)
    expect.view(B, L, L, C)[1, 5] = True
    assert torch.equal(nan, expect) and torch.equal(nan, ~torch.isfinite(ref))
    assert torch.equal(o[~nan], clean[~nan]) and torch.equal(o[~nan], ref[~nan])
    # a key channel of head 1 beyond 4095
    qkv2 = _packs(ops, 5201, k_bias_shift=(1 * D + 7, 5000.0))[0]
    rowp2 = ops.TriRowPack(qkv2)
    word.zero_()
    ref, rows = _two_launches(ops, qkv2, z, bias, mask, B, L, True)
    assert int(word.item()) == T['tri_attn'] and torch.isfinite(rows).all()
    word.zero_()
    o = _fused(ops, rowp2, z, bias, mask, B, L, True)
    assert int(word.item()) == T['tri_attn']
    nan = ~torch.isfinite(o)
    expect = torch.zeros_like(nan)
    expect[:, D:2 * D] = True
    assert torch.equal(nan, expect) and torch.equal(nan, ~torch.isfinite(ref))
    assert torch.equal(o[~nan], ref[~nan])
    word.zero_()


def test_batch_independence(ops):
    """Samples {0, 7, 12} of a B = 13 launch equal the same samples run at B = 1, bit for bit, at L = 352 (the route is chosen by L alone)."""
    L, B = 352, 13
    qkv = _packs(ops, 5300)[0]
    rowp = ops.TriRowPack(qkv)
    z, bias, mask = _inputs(L, B, 5301)
    for per_row in (True, False):
        o = _fused(ops, rowp, z, bias, mask, B, L, per_row).view(B, L * L, C)
        assert torch.isfinite(o).all()
        for s in (0, 7, 12):
            o1 = _fused(ops, rowp, z[s:s + 1].contiguous(), bias[s:s + 1].contiguous(), mask[s:s + 1].contiguous(), 1, L, per_row)
            assert torch.equal(o1.view(L * L, C), o[s]), (per_row, s)
        del o


@pytest.mark.parametrize('L,B,exact', [(402, 1, False), (97, 4, True), (120, 3, False)])
def test_block_route_and_ineligible_shapes(ops, L, B, exact):
    """abx_tri_attn_block_fwd with and without the row pack: L = 402 and the exact route take the old kernels either way (equal bits, and
    ops.tri_attn_kernel_name says so); an eligible L takes the fused kernel with the row pack and gives the bits of the two launches.
    Which route ran is read off the q | k | v region of the workspace (the first B L L 576 floats), poisoned with NaN before every call: the
    two launches write it, the fused route leaves it untouched."""
    from abx_amd import _lib
    from abx_amd._lib import AbxTriRowPack, AbxHipError
    lib = _lib.load()
    qkv, gate, pair, out = _packs(ops, 5400 + L)
    z, _, mask = _inputs(L, B, 5401 + L)
    name = ops.tri_attn_kernel_name(L, exact=exact, rowfused=None if exact else bool(lib.abx_tri_attn_rowfused_ok(L)))
    fused_route = not exact and L <= 352
    assert int(lib.abx_tri_attn_rowfused_ok(L)) == (1 if L <= 352 else 0), 'ABX_NO_TRI_ROWFUSED must not be set for this test'
    if L > 352:
        assert name.startswith('tri_attn8_kernel<')
        with pytest.raises(AbxHipError, match='ABX_TRI_ROWFUSED_LMAX'):
            _fused(ops, ops.TriRowPack(qkv), z, torch.zeros(B, H, L, (L + 3) // 4 * 4, device=DEV), mask, B, L, True)
    elif exact:
        assert name == 'tri_attn_kernel'
    else:
        assert name == 'tri_attn8_rowfused_kernel'
        assert ops.tri_attn_kernel_name(L, exact=False, rowfused=False).startswith('tri_attn8_kernel<')
    ws = ops.tri_attn_block_workspace(B, L, DEV)
    rows = ws[:4 * B * L * L * 576].view(torch.float32)
    res = {}
    for with_row in (True, False):
        p = ops.tri_attn_pack(qkv, gate, pair, out)
        assert p._row is not None
        if not with_row:
            p.row = AbxTriRowPack()
        for per_row in (True, False):
            zz = z.clone().view(B * L * L, C)
            rows.fill_(float('nan'))
            ops.tri_attn_block_fwd(p, zz, mask, B, L, per_row, ws, exact=exact, attn_exact=exact)
            res[(with_row, per_row)] = zz
            untouched = bool(torch.isnan(rows).all())
            assert untouched == (with_row and fused_route), (L, exact, with_row, per_row, 'q | k | v region untouched' if untouched else 'q | k | v region written')
    for per_row in (True, False):
        assert torch.isfinite(res[(True, per_row)]).all()
        assert torch.equal(res[(True, per_row)], res[(False, per_row)]), (L, exact, per_row)
