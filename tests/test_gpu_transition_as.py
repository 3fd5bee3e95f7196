"""The pair Transition as an A-stationary fused MLP (csrc/gemm_as.hip gemm_as_mlp_kernel: one block per 64 pair rows, z split once, the hidden
sum of the second GEMM split over two waves).  The yardsticks are fp64 and the tile kernel it replaces for the shape class K = 192, hidden
768, 192 outputs (gemm3_mlp_kernel<2>, kept per descriptor by AbxGemm.tune bit 11).  The two differ in the ORDER of the hidden sum, so the
demand between them is agreement at fp32 rounding, and the new kernel is chosen by the shape class alone: a sample's bits must not depend
on the launch.  Needs an MI355X: `pytest -m gpu`."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TILE = 2048
K, NH, N2 = 192, 768, 192
# one block; whole blocks; ragged last blocks of 1 and of 63 rows; 43 blocks with a ragged last one (two samples of L = 37)
SHAPES = [64, 64 * 3, 64 * 5 + 1, 64 * 4 + 63, 37 * 37 * 2]


@pytest.fixture(scope='module')
def ops():
    from abx_amd import ops as _ops, _lib
    lib = _lib.load()
    assert lib.abx_init(0) == 0, lib.abx_last_error_string()
    return _ops


def g(seed):
    return torch.Generator().manual_seed(seed)


def fold_ln(W, b, gamma, beta):
    """LayerNorm folded into the Linear: Wt' = gamma * Wt, its column sums, bias' = beta @ Wt + b."""
    wt = W.double().t()
    wts = gamma.double()[:, None] * wt
    bias = beta.double() @ wt + b.double()
    return wts.float().contiguous().to(DEV), wts.sum(0).float().contiguous().to(DEV), bias.float().contiguous().to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


class Transition:
    """Weights and rows of test_gemm_fused_transition (tests/test_gpu_kernels.py): z = randn * 2 + 0.7 with row 3 at |mean| >> sigma,
    W1 / sqrt(K), W2 / sqrt(NH), both biases, the LayerNorm folded.  The host copies stay as they were drawn."""

    def __init__(self, ops, seed, rows=max(SHAPES), spike=None):
        self.ops = ops
        ge = g(seed)
        self.z = torch.randn(rows, K, generator=ge) * 2 + 0.7
        self.z[3] = 1e3 + torch.randn(K, generator=ge)
        self.W1, self.b1 = torch.randn(NH, K, generator=ge) / K ** 0.5, 0.1 * torch.randn(NH, generator=ge)
        self.W2, self.b2 = torch.randn(N2, NH, generator=ge) / NH ** 0.5, 0.1 * torch.randn(N2, generator=ge)
        self.ga, self.be = 1 + 0.1 * torch.randn(K, generator=ge), 0.1 * torch.randn(K, generator=ge)
        if spike is not None:
            self.W1[spike] = 400.0
        self.w1, self.cs1, self.bi1 = fold_ln(self.W1, self.b1, self.ga, self.be)
        self.w13 = ops.split_weights(self.w1)
        self.w23 = ops.split_weights(ops.permute_k16(self.W2.t().contiguous().to(DEV)))
        self.b2d = self.b2.to(DEV)

    def run(self, M, tune, inplace, z=None):
        """One launch on the first M rows, which sit in a buffer with eight guard rows behind them (NaN out of place; in place the guard rows
        hold a value no output takes).  Returns (output rows, guard rows)."""
        zd = (self.z if z is None else z)[:M].to(DEV)
        if inplace:
            buf = torch.full((M + 8, K), 7.0e7, device=DEV)
            buf[:M] = zd
            src = buf[:M]
        else:
            buf = torch.full((M + 8, N2), float('nan'), device=DEV)
            src = zd
        self.ops.gemm(src, self.w1, buf[:M], bias=self.bi1, ln=(None, self.cs1), B3=self.w13, act=1, resid=src, exact=2, mlp=(self.w23, self.b2d),
                      tune=tune)
        torch.cuda.synchronize()
        return buf[:M], buf[M:]

    def fp64(self, M):
        x = self.z[:M].double()
        ln = (x - x.mean(-1, keepdim=True)) / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + 1e-5) * self.ga.double() + self.be.double()
        return torch.relu(ln @ self.W1.double().t() + self.b1.double()) @ self.W2.double().t() + self.b2.double() + x


@pytest.fixture(scope='module')
def tr(ops):
    return Transition(ops, 9700)


def plan_name(ops, M, tune=0, with_resid=True):
    """The kernel the library names for the transition descriptor of M rows (abx_gemm_plan: its own dispatch, nothing launched)."""
    from abx_amd import _lib
    from abx_amd._lib import AbxGemm
    P = 1 << 40
    d = AbxGemm()
    d.M, d.N, d.K, d.batch, d.alpha, d.exact = M, NH, K, 1, 1.0, 2
    d.A, d.sAm, d.sAk = 1 * P, K, 1
    d.B, d.sBk, d.sBn = 2 * P, NH, 1
    d.B_split, d.sB3n, d.sB3p, d.sB3k, d.b_f16 = 3 * P, 16, 16 * NH, 32 * NH, 1
    d.C, d.sCm = 1 * P, N2
    d.ln_csum, d.bias, d.ln_eps = 5 * P, 6 * P, 1e-5
    d.mlp, d.act, d.N2 = 1, 1, N2
    d.B2_split, d.sB23n, d.sB23p, d.sB23k, d.bias2 = 12 * P, 16, 16 * N2, 32 * N2, 13 * P
    if with_resid:
        d.resid, d.sRm = 1 * P, N2
    d.tune = tune
    buf = ctypes.create_string_buffer(128)
    rc = _lib.load().abx_gemm_plan(ctypes.byref(d), None, buf, len(buf))
    assert rc == 0, _lib.load().abx_last_error_string()
    return buf.value.decode()


def test_the_shape_class_decides_the_kernel_not_the_launch(ops):
    for M in SHAPES + [1, 352 * 352 * 100]:
        assert plan_name(ops, M) == 'gemm_as_mlp_kernel', M
        assert plan_name(ops, M, tune=TILE) == 'gemm3_mlp_kernel<2>', M


@pytest.mark.parametrize('inplace', [True, False])
@pytest.mark.parametrize('M', SHAPES)
def test_against_fp64_and_the_tile_kernel(ops, tr, M, inplace):
    """fp64 at the bound of test_gemm_fused_transition (3e-6); the tile kernel at the bound that test sets between the fused kernel and the two
    launches of the same arithmetic class (2e-6: fp32 rounding of the hidden sums); nothing but the M rows is written."""
    out, guard = tr.run(M, 0, inplace)
    old, guard_old = tr.run(M, TILE, inplace)
    ref = tr.fp64(M)
    e64, e_old, e64_old = rel_err(out, ref), rel_err(out, old), rel_err(old, ref)
    print(f'M = {M} inplace = {inplace}: new vs fp64 {e64:.3e}, tile kernel vs fp64 {e64_old:.3e}, new vs tile kernel {e_old:.3e}')
    assert torch.isfinite(out).all()
    assert e64 == e64 and e64 <= 3e-6, f'A-stationary transition vs fp64: rel err {e64:.3e}'
    assert e_old == e_old and e_old <= 2e-6, f'A-stationary transition vs tile kernel: rel err {e_old:.3e}'
    if inplace:
        assert bool((guard == 7.0e7).all()) and bool((guard_old == 7.0e7).all())
    else:
        assert torch.isnan(guard).all() and torch.isnan(guard_old).all()


@pytest.mark.parametrize('inplace', [True, False])
def test_a_sample_does_not_depend_on_the_launch(ops, tr, inplace):
    """The first three blocks give the same bits launched alone and as the head of a launch of five blocks and one row."""
    alone, _ = tr.run(64 * 3, 0, inplace)
    head, _ = tr.run(64 * 5 + 1, 0, inplace)
    assert torch.isfinite(alone).all()
    assert torch.equal(bits(alone), bits(head[:64 * 3])), float((alone - head[:64 * 3]).abs().max())


def test_range_contract(ops):
    """One hidden activation beyond the 2^4 lift of the hidden pieces (|h| >= 4094): hidden channel 100 weighs input channel 17 with 400, and
    one row is a spike on that channel (LayerNorm value ~ sqrt(191), hidden ~ 5 500; every other row stays below 400 x 5).  NaN in exactly
    that row, the bit of the pair transition in the range word as the tile kernel sets it, every other row as without the spike."""
    M, row = 64 * 4 + 63, 64 * 2 + 37
    t = Transition(ops, 9800, rows=M, spike=(100, 17))
    assert float(t.ga[17]) > 0.5
    word = ops.range_word(DEV)
    word.zero_()
    clean, _ = t.run(M, 0, False)
    assert int(word.item()) == 0 and torch.isfinite(clean).all()
    z = t.z.clone()
    z[row] = 0.0
    z[row, 17] = 50.0
    got = []
    for tune in (TILE, 0):
        word.zero_()
        out, guard = t.run(M, tune, False, z)
        got.append((out, int(word.item())))
        assert torch.isnan(guard).all()
    word.zero_()
    (old, w_old), (out, w_new) = got
    assert w_old & ops.RANGE_TAGS['pair_transition'] and w_new == w_old, (w_old, w_new)
    bad = torch.isnan(out).any(-1)
    assert torch.equal(bad, torch.isnan(old).any(-1))
    assert bool(bad[row]) and int(bad.sum()) == 1, int(bad.sum())
    assert torch.isnan(out[row]).all()
    assert torch.equal(bits(out[~bad]), bits(clean[~bad]))


def test_block_entry_equals_the_descriptor_path(ops):
    """ops.transition_fwd (abx_transition_fwd, weights packed by abx_pack_linear) against the descriptor-level launch on the same pack, two
    samples of L = 33: both go through abx_gemm and take the same kernel."""
    L, B = 33, 2
    M = B * L * L
    ge = g(9900)
    W1, b1 = (torch.randn(NH, K, generator=ge) / K ** 0.5).to(DEV), (0.1 * torch.randn(NH, generator=ge)).to(DEV)
    W2, b2 = (torch.randn(N2, NH, generator=ge) / NH ** 0.5).to(DEV), (0.1 * torch.randn(N2, generator=ge)).to(DEV)
    ln = ((1 + 0.1 * torch.randn(K, generator=ge)).to(DEV), (0.1 * torch.randn(K, generator=ge)).to(DEV))
    l1 = ops.LinearPack([(W1, b1, 0)], K, ln=ln)
    l2 = ops.LinearPack([(W2, b2, 0)], NH, permute_k16=True)
    z = (torch.randn(M, K, generator=ge) * 2 + 0.7).to(DEV)
    got = ops.transition_fwd(l1, l2, z.clone())
    ref = z.clone()
    ops.gemm(ref, l1.Wt, ref, bias=l1.bias, ln=(None, l1.csum), B3=l1.planes, act=1, resid=ref, exact=2, mlp=(l2.planes, l2.bias))
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    assert torch.equal(bits(got), bits(ref)), float((got - ref).abs().max())
