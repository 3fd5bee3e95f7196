"""Tensor-level wrappers over the C ABI (abx_amd/_lib.py).  torch is used for device memory and the current
stream only; every function launches HIP kernels from libabx_hip.so and raises if the library is unavailable."""
import ctypes as C
import math
import os

import torch

from abx_amd import _lib
from abx_amd._lib import (AbxGemm, AbxTriAttn, AbxIpaTail, AbxHeadsTail, AbxScoreArgs, AbxReverseArgs, AbxGuidanceArgs, AbxContactArgs, AbxDesignScoreArgs, AbxRelaxArgs, AbxInterfaceArgs, AbxPolarArgs, AbxDevelopabilityArgs, AbxShapeArgs, AbxPatchArgs, AbxTorsionArgs, AbxSecondaryArgs, AbxDistogramArgs, AbxAccuracyArgs, AbxEnsemblePairsArgs, AbxEnsembleClusterArgs, AbxLinearPack, AbxLinearSrc,
                           AbxTriMulPack, AbxTriAttnPack, AbxTriRowPack, check)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    assert t.is_cuda, 'libabx_hip works on device memory only'
    return t.data_ptr()


def _f32(t):
    assert t.dtype == torch.float32, t.dtype
    return t


def env_on(name):
    """The one rule for the on / off environment switches, the library's abx_env_on (csrc/capi.hip): ON when the variable is set, not empty
    and not "0"."""
    return os.environ.get(name, '') not in ('', '0')


# kernel-variant selector (benchmarking only: AbxGemm.tune of every descriptor-level launch).  The live bits are listed at AbxGemm.tune in
# include/abx_hip.h (ABX_TUNE_LIVE_MASK: 1, 64, 128, 2048, 16384); any other bit - a retired variant's, DESIGN.md - is refused by the library at the first GEMM
GEMM_TUNE = int(os.environ.get('ABX_GEMM_TUNE', '0'))

# ---- range safety of the split-f16 kernels (include/abx_hip.h, AbxGemm.range_flag) ----------------------------------------------
# Every split-f16 launch made through this module carries the address of one device word per GPU and a bit that names its call-site
# class; a kernel whose accumulators are not finite - what an operand beyond the split ranges turns into - ORs its bit into the word.
# abx_amd.model.abx.ScoreNetwork clears the word before a network call, reads it after, and repeats the call on the exact fp32-MFMA
# kernels when it is set, so the range contract of the fast path never reaches a caller as a wrong or non-finite result.
RANGE_TAGS = {'gemm': 1, 'contraction': 2, 'plane_projection': 4, 'tri_mul_tail': 8, 'pair_transition': 16, 'ipa_pair_init': 32,
              'tri_attn': 64, 'ipa_tail': 128, 'heads_tail': 256, 'gemm_late': 512}     # gemm / gemm_late: the plain GEMMs in front of / behind the pair stack
RANGE_CHECK = not env_on('ABX_NO_RANGE_CHECK')     # (A / B measurements of the probe's cost)
_range_words = {}


RANGE_SLOTS = 4
RANGE_SLOT = 0       # which of the device's range words the launches issued now report to (ScoreNetwork: one word per network pass, so that
                     # the pass - and with ops.RANGE_ORDER the op class - that left the range FIRST is known from one read-back per call)


def range_words(device):
    """The int32 [RANGE_SLOTS] range words of a device (created on first use, zero)."""
    idx = torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    w = _range_words.get(idx)
    if w is None:
        w = torch.zeros(RANGE_SLOTS, dtype=torch.int32, device=torch.device('cuda', idx))
        _range_words[idx] = w
    return w


def range_word(device):
    """The first range word (int32 [1] view): what every launch reports to unless ops.RANGE_SLOT says otherwise."""
    return range_words(device)[0:1]


def range_ptr(device):
    """Device address of the range word in use (ops.RANGE_SLOT)."""
    return range_words(device).data_ptr() + 4 * RANGE_SLOT


def range_names(bits):
    return [n for n, b in RANGE_TAGS.items() if bits & b]


# order in which the op classes appear in a network pass: a class that left its range hands NaN rows to every class after it, so of the
# bits a call sets only the FIRST one names an op that needs the exact kernels (abx_amd.model.abx.ScoreNetwork.forward)
RANGE_ORDER = ('gemm', 'plane_projection', 'contraction', 'tri_mul_tail', 'tri_attn', 'pair_transition', 'ipa_pair_init', 'gemm_late', 'ipa_tail', 'heads_tail')


def first_range_tag(bits, skip=0):
    """The bit of the earliest op class of a pass among `bits` that is not in `skip`, or 0."""
    for n in RANGE_ORDER:
        if bits & RANGE_TAGS[n] & ~skip:
            return RANGE_TAGS[n]
    return 0


GEMM_EXACT = False   # True: every GEMM on the exact fp32 MFMA kernel (v_mfma_f32_32x32x2_f32); default: large problems on the
                     # split-f16 kernels of csrc/gemm3.hip (fp32-accurate)


def _plan_name(fn, *args):
    """(return code, kernel name) of abx_gemm_plan / abx_tri_attn_plan / abx_seq_attn_plan: the library's own dispatch run up to the launch.  Needs no GPU."""
    buf = C.create_string_buffer(128)
    rc = fn(*args, buf, len(buf))
    return rc, buf.value.decode()


def _placeholders():
    """Stand-in device addresses for a descriptor that is only planned: non-null, 16-byte aligned, 1 TiB apart (disjoint for any tensor).
    The library looks at their alignment and overlap and never follows them."""
    return iter(range(1 << 40, 1 << 62, 1 << 40))


def gemm_kernel_name(M, N, K, batch, a_kcontig=True, b_ncontig=True, transposed=False, split=False, exact=None, a_split=False, dual=False, out_ln=False):
    """Name of the kernel instantiation abx_gemm launches for a problem, as `rocprofv3 --stats` spells it; used by bench.py to aggregate per
    KERNEL.  The answer is the library's (abx_gemm_plan: the dispatch of csrc/gemm.hip, gemm3.hip and gemm_as.hip itself, environment
    switches and GEMM_TUNE included) for a descriptor of dense tensors of this shape at placeholder addresses: fp32 A (k- or m-contiguous) and
    B, weight planes with `split`, operand images on both sides with `a_split`, no epilogue operands; `dual`: the tri-mul tail (K2 = 192 gate
    rows, both LayerNorms folded, residual); `out_ln`: the output LayerNorm."""
    P = _placeholders()
    g = AbxGemm()
    g.M, g.N, g.K, g.batch = M, N, K, batch
    g.exact, g.tune, g.alpha = (1 if GEMM_EXACT else int(exact or 0)), GEMM_TUNE, 1.0
    KT = (K + 15) // 16
    if a_split:
        g.A_split, g.sA3m, g.sA3p, g.sA3k, g.sA3b = next(P), 16, 16 * M, 32 * M, (KT * 32 * M if batch > 1 else 0)
        g.B_split, g.sB3n, g.sB3p, g.sB3k, g.sB3b = next(P), 16, 16 * N, 32 * N, (KT * 32 * N if batch > 1 else 0)
    else:
        g.A, g.sAb = next(P), (M * K if batch > 1 else 0)
        g.sAm, g.sAk = (K, 1) if a_kcontig else (1, M)
        g.B, g.sBb = next(P), (K * N if batch > 1 else 0)
        g.sBk, g.sBn = (N, 1) if b_ncontig else (1, K)
        if split:
            g.B_split, g.sB3n, g.sB3p, g.sB3k, g.b_f16 = next(P), 16, 16 * N, 32 * N, 1
    g.C, g.sCb, g.c_transposed, g.sCm = next(P), (M * N if batch > 1 else 0), int(bool(transposed)), (M if transposed else N)
    if dual:
        g.A2, g.K2, g.sA2m, g.sA2b = next(P), 192, 192, (M * 192 if batch > 1 else 0)
        g.B2_split, g.sB23n, g.sB23p, g.sB23k = next(P), 16, 16 * N, 32 * N
        g.ln_csum, g.bias, g.ln2_csum, g.bias2, g.ln_eps = next(P), next(P), next(P), next(P), 1e-5
        g.resid, g.sRb, g.sRm = next(P), g.sCb, g.sCm
    if out_ln:
        g.out_ln_w, g.out_ln_b = next(P), next(P)
    rc, name = _plan_name(_lib.load().abx_gemm_plan, C.byref(g), None)
    if rc and dual:       # no launch to name (the exact fp32 kernels have no dual form; M % 4 with a channel-major product): the tile kernel's
        return 'gemm3_dual_kernel<128, 96, 32, 96, 3>'
    check(rc, 'abx_gemm_plan')
    return name


def gemm_as_kernel_name(g, side=None):
    """Name of the A-stationary kernel instantiation (csrc/gemm_as.hip) that abx_gemm / abx_gemm_side launch for a filled descriptor, or
    None when the problem goes to the tile kernels - or is the dual GEMM, which gemm_kernel_name names (abx_gemm_plan on the descriptors
    themselves: alignment, switches and tune bits count as they do for the launch)."""
    rc, name = _plan_name(_lib.load().abx_gemm_plan, C.byref(g), None if side is None else C.byref(side))
    return name if rc == 0 and name.startswith('gemm_as_kernel') else None


SPLIT_MIN_L = 64


def gemm_mode(L):
    """Arithmetic class of the GEMMs of a network pass, fixed by the complex (residue count L) and NOT by how many samples share a
    launch: 2 (split-f16 kernels) from L = 64, 1 (exact fp32 MFMA) below.  Chunking a batch, sharding it over GPUs or running
    one sample alone therefore gives bit-identical results."""
    return 1 if (GEMM_EXACT or L < SPLIT_MIN_L) else 2


def gemm_split_eligible(M, N, K, batch=1):
    """True when abx_gemm serves an (aligned) problem of this size on the split-f16 kernels of csrc/gemm3.hip (gemm_kernel_name)."""
    return gemm_kernel_name(M, N, K, batch, split=True).startswith('gemm3_')


def pack_glu_weights(Wv, Wg, bv=None, bg=None):
    """Column order of a glu GEMM: 32-column blocks [v0 | g0 | v1 | g1 | ...] of value weights Wv (K, C) and gate weights
    Wg (K, C) for the same C output channels (C % 64 == 0).  Returns (W (K, 2C), bias (2C) or None)."""
    K, C_ = Wv.shape
    assert Wg.shape == (K, C_) and C_ % 64 == 0
    W = torch.stack([Wv.reshape(K, C_ // 32, 32), Wg.reshape(K, C_ // 32, 32)], dim=2).reshape(K, 2 * C_).contiguous()
    b = None
    if bv is not None or bg is not None:
        z = torch.zeros(C_, device=Wv.device, dtype=Wv.dtype)
        b = torch.stack([(bv if bv is not None else z).reshape(C_ // 32, 32), (bg if bg is not None else z).reshape(C_ // 32, 32)],
                        dim=1).reshape(2 * C_).contiguous()
    return W, b


_PERM16 = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)


def permute_k16(Wt):
    """Wt (K, N), K % 16 == 0 -> rows reordered inside every block of 16 as 0-3, 8-11, 4-7, 12-15: the k order in which the fused
    transition (AbxGemm.mlp) feeds its second GEMM from the accumulator registers of the first (csrc/gemm3.hip)."""
    K, N = Wt.shape
    assert K % 16 == 0
    idx = torch.tensor(_PERM16, device=Wt.device)
    return Wt.reshape(K // 16, 16, N)[:, idx, :].reshape(K, N).contiguous()


class WeightPlanes(torch.Tensor):
    """float16 tensor [Kp/16][2][N][16] of split weight planes + the power-of-two exponent they were scaled with (`w_exp`)."""
    w_exp = 0
    __torch_function__ = torch._C._disabled_torch_function_impl     # a plain data carrier: no dispatch overhead on .stride() / .shape


def split_weights(Wt):
    """Wt (K, N) packed weight (n-contiguous) -> WeightPlanes [Kp/16][2][N][16] float16: the k-tiled operand image of the split-f16
    weight GEMMs (AbxGemm.b_f16, include/abx_hip.h): with w' = w * 2^w_exp, max|w'| in [2^13, 2^14):
    p0 = f16(w'), p1 = f16(w' - p0) (the kernels derive p2 = f16(p0 * 2^-11) in registers);  w' = p0 + p1 up to 2^-23 |w'| (+ 2^-25
    absolute).  One host sync (the
    maximum) per call: weights are packed once, outside any graph capture.  Kp = K rounded up to 16."""
    K, N = Wt.shape
    _f32(Wt)
    Kp = (K + 15) // 16 * 16
    amax = float(Wt.abs().max())
    if not math.isfinite(amax):
        raise ValueError('split_weights: non-finite weight')
    w_exp = 14 - math.frexp(amax)[1] if amax > 0 else 0
    w_exp = max(-100, min(100, w_exp))
    out = torch.empty(Kp // 16, 2, N, 16, device=Wt.device, dtype=torch.float16)
    check(_lib.load().abx_split_weights_f16(_p(Wt), Wt.stride(1), Wt.stride(0), N, K, w_exp, _p(out), _stream()), 'abx_split_weights_f16')
    out = out.as_subclass(WeightPlanes)
    out.w_exp = w_exp
    return out


def weights_to_float(w3):
    """WeightPlanes -> fp32 (Kp, N) value the kernels multiply with: (p0 + p1) * 2^-w_exp."""
    v = (w3[:, 0].float() + w3[:, 1].float()) * 2.0 ** (-w3.w_exp)
    return v.permute(0, 2, 1).reshape(-1, w3.shape[2])


def _weight_planes(w3, N, K=None, what='B3'):
    assert isinstance(w3, WeightPlanes) and w3.dtype == torch.float16 and w3.is_contiguous() and w3.shape[1:] == (2, N, 16), \
        f'{what}: WeightPlanes (ops.split_weights) of N = {N} expected'
    assert K is None or w3.shape[0] * 16 >= K
    return w3


def gemm(A, B, Cout, *, ln=None, a_relu=False, bias=None, alpha=1.0, act=0, rowscale=None, gate=None, gate_sigmoid=True,
         resid=None, tune=None, B3=None, exact=None, a_pair_transpose=0, glu=False, pair=None, a_pair=False, c_pair=False, dual=None, out_ln=None, clock_probe=None, mlp=None, c_split_nA=0, c_split_tile=False,
         defer=False, range_class=None, c_plane_cols=None):
    """Cout[b] = epi(A'[b] @ B[b]).  A (b,M,K) or (M,K); B (b,K,N) or (K,N) (shared); Cout (b,M,N) or (M,N) logical tensors.
    Strides decide the kernel variant: A k- or m-contiguous, B n- or k-contiguous, Cout n-contiguous or (if its last-but-one
    stride is 1) stored transposed.  ln = (stats (rows,2) | None, csum).  rowscale (b,M)|(M,), gate/resid (b,M,N)|(M,N) logical
    tensors laid out like Cout (n-contiguous, or m-contiguous when Cout is stored transposed).
    Split-f16 operands (include/abx_hip.h, "Split-f16 operands"): B3 (K/16,2,N,16) = split_weights(B), float16 weight planes;
    A (b,K/16,2,M,16) and B (b,K/16,2,N,16) both int16 tensors of activation images: the TriangleMultiplication contraction (A: the
    pieces a0, a1; B: the planes p0, p1); Cout (b,N,L/16,2,L,16) int16 (M = L*L pair rows, m = i*L + k): the output is written
    as the operand image [n][k/16][plane][i][16] of that contraction (transposed store), channels n < c_split_nA as its A side, the
    others as its B side.  a_pair_transpose=L: GEMM row i*L+k reads A row k*L+i.
    glu=True: B holds (value, gate) column pairs (pack_glu_weights); Cout has N/2 channels = value * sigmoid(gate).
    pair=(L, Lp): the M rows are padded pair positions i*Lp + j (Lp % 4 == 0, any L); a_pair: A is the UNpadded (b, L*L, K) pair
    tensor; c_pair: Cout / gate / resid are UNpadded (b, L*L, N) pair tensors (pad rows dropped).  rowscale is indexed by GEMM row.
    dual=(A2, B3_2, csum2, bias2): Cout = epi(A' B) * sigmoid(LN(A2) @ W2 + bias2) (+ resid): A2 (b, rows, K2) k-contiguous fp32 (the
    UNpadded pair tensor when pair is given), B3_2 = split_weights of the gamma-scaled gate weights (K2, N), csum2 their column sums.
    out_ln=(gamma, beta[, eps]): LayerNorm over the N output columns right after bias / alpha / act (split-f16 path only, N <= 128).
    defer=True: nothing is launched, the filled AbxGemm is returned (for gemm_side).
    mlp=(B3_2, bias2): fused two-layer transition Cout = relu(LN(A) @ B + bias) @ W2 + bias2 (+ resid); B (K, N) is the first layer
    (N = hidden width, act must be 1, ln given), B3_2 = split_weights(permute_k16(W2t)) of the second layer W2t (N, N2), Cout / resid
    have N2 <= 192 columns and may alias A.  With `gate` (M, N) fp32 rows and act = 2 the same call is the gated tail of the triangle attention
    (AbxGemm.mlp = 2): Cout = (sigmoid(LN(A) @ B + bias) * gate) @ W2 + bias2 (+ resid)."""
    lib = _lib.load()
    g = AbxGemm()
    a_planes, b_planes, c_planes = A.dtype == torch.int16, B.dtype == torch.int16, Cout.dtype == torch.int16
    if a_planes and A.dim() == 6:      # (Bo, Bi, K/16, 2, M, 16): two-level batch (channel slices of a wider per-sample tensor)
        assert B.dtype == torch.int16 and B.dim() == 6 and B.shape[:2] == A.shape[:2]
        g.batch_inner, g.sA3i, g.sB3i = A.shape[1], A.stride(1), B.stride(1)
        bo_a, bo_b = A.stride(0), B.stride(0)
        A = A.as_strided((A.shape[0] * A.shape[1],) + tuple(A.shape[2:]), (0,) + tuple(A.stride()[2:]), A.storage_offset())
        B = B.as_strided((B.shape[0] * B.shape[1],) + tuple(B.shape[2:]), (0,) + tuple(B.stride()[2:]), B.storage_offset())
    else:
        bo_a = bo_b = None
    if a_planes:
        assert A.dim() == 5 and A.shape[2] == 2 and A.shape[4] == 16 and A.stride(4) == 1
        nb, KT, _, M, _ = A.shape
        K = KT * 16
        g.A_split, g.sA3b, g.sA3k, g.sA3p, g.sA3m = _p(A), (A.stride(0) if nb > 1 else 0), A.stride(1), A.stride(2), A.stride(3)
        if bo_a is not None:
            g.sA3b = bo_a
    else:
        if A.dim() == 2:
            A = A.unsqueeze(0)
        nb, M, K = A.shape
        _f32(A)
        g.A, g.sAb, g.sAm, g.sAk = _p(A), A.stride(0) if nb > 1 else 0, A.stride(1), A.stride(2)
        if a_pair:
            assert pair is not None and M == pair[0] * pair[0], (A.shape, pair)
            M = pair[0] * pair[1]
            if c_split_tile:        # GEMM rows = pair positions in (8 i x 16 k) blocks (AbxGemm.c_split_tile)
                M = ((pair[0] + 7) // 8 * 8) * ((pair[1] + 15) // 16 * 16)
    if b_planes:
        assert B.dim() == 5 and B.shape[2] == 2 and B.shape[4] == 16 and B.stride(4) == 1 and B.shape[1] * 16 == K and B.shape[0] == nb
        N = B.shape[3]
        g.B_split, g.sB3b, g.sB3k, g.sB3p, g.sB3n = _p(B), (B.stride(0) if nb > 1 else 0), B.stride(1), B.stride(2), B.stride(3)
        if bo_b is not None:
            g.sB3b = bo_b
    else:
        if B.dim() == 2:
            B = B.unsqueeze(0)
        assert B.shape[1] == K, (A.shape, B.shape)
        N = B.shape[2]
        _f32(B)
        g.B, g.sBb, g.sBk, g.sBn = _p(B), (B.stride(0) if B.shape[0] > 1 else 0), B.stride(1), B.stride(2)
    No = N // 2 if glu else N
    if mlp is not None:
        B32m, bias2m = mlp
        No = B32m.shape[2]
        _weight_planes(B32m, No, what='mlp B3_2')
        assert B32m.shape[0] * 16 == N
        g.mlp, g.N2, g.b2_exp = (2 if gate is not None else 1), No, B32m.w_exp
        g.B2_split, g.sB23k, g.sB23p, g.sB23n = _p(B32m), B32m.stride(0), B32m.stride(1), B32m.stride(2)
        g.bias2 = _p(bias2m)
        assert act == (2 if gate is not None else 1) and ln is not None and ln[0] is None
    if c_planes:
        L = Cout.shape[4]
        Lp = pair[1] if pair is not None else L
        assert Cout.dim() == 6 and Cout.shape == (nb, No, (Lp + 15) // 16, 2, L, 16) and (c_split_tile or M == L * Lp), (Cout.shape, nb, M, N)
        assert not c_split_tile or (a_pair and pair is not None), 'c_split_tile: the A rows come through the pair-row map (a_pair, pair=(L, Lp))'
        assert Cout.stride(5) == 1 and Cout.stride(4) == 16
        g.C_split, g.sCb, g.sCm, g.sCk, g.sCp, g.c_split_L = _p(Cout), (Cout.stride(0) if nb > 1 else 0), Cout.stride(1), Cout.stride(2), Cout.stride(3), Lp
        g.c_transposed, g.c_split_nA, g.c_split_tile = 1, int(c_split_nA), int(bool(c_split_tile))
    else:
        if Cout.dim() == 2:
            Cout = Cout.unsqueeze(0)
        assert Cout.shape == (nb, pair[0] * pair[0] if c_pair else M, No), (Cout.shape, (nb, M, No))
        _f32(Cout)
        g.C = _p(Cout)
        Cl = Cout
        g.sCb = Cl.stride(0) if nb > 1 else 0
        if Cl.stride(2) == 1:
            g.c_transposed, g.sCm = 0, Cl.stride(1)
        else:
            assert Cl.stride(1) == 1, 'Cout must be n-contiguous or m-contiguous'
            g.c_transposed, g.sCm = 1, Cl.stride(2)
    g.M, g.N, g.K, g.batch = M, N, K, nb
    g.a_pair_transpose = int(a_pair_transpose)
    if pair is not None:
        g.pair_L, g.pair_Lp, g.a_pair, g.c_pair = int(pair[0]), int(pair[1]), int(bool(a_pair)), int(bool(c_pair))
        assert c_split_tile or M == pair[0] * pair[1], (M, pair)
    g.glu = int(bool(glu))
    if ln is not None:
        stats, csum = ln                     # stats None: the kernel derives (mean, rstd) from its own A stream
        assert csum.numel() == N
        g.ln_csum, g.ln_eps = _p(_f32(csum)), 1e-5
        if stats is not None:
            assert stats.numel() == 2 * nb * M, (stats.shape, nb, M)
            g.ln_stats, g.sSb = _p(_f32(stats)), M
    g.a_relu = 1 if a_relu else 0
    g.exact = 1 if GEMM_EXACT else int(exact or 0)        # 0 by problem size, 1 exact fp32 MFMA, 2 split-f16 whenever the shape allows
    if B3 is not None:
        _weight_planes(B3, N, K)
        assert not a_planes, 'weight planes go with an fp32 A (the plane x plane contraction takes activation images on both sides)'
        g.B_split, g.sB3k, g.sB3p, g.sB3n, g.sB3b = _p(B3), B3.stride(0), B3.stride(1), B3.stride(2), 0
        g.b_f16, g.b_exp = 1, B3.w_exp
    g.tune = GEMM_TUNE if tune is None else tune
    if c_plane_cols is not None:      # (from, group): the output columns n >= from as two float16 planes of 16 x value per group (AbxGemm.c_planes_from)
        g.c_planes_from, g.c_planes_group = int(c_plane_cols[0]), int(c_plane_cols[1])
    if RANGE_CHECK and g.exact != 1:
        g.range_flag = range_ptr(Cout.device)
        g.range_tag = RANGE_TAGS[('tri_attn' if gate is not None else 'pair_transition') if mlp is not None else 'tri_mul_tail' if dual is not None else 'ipa_pair_init' if out_ln is not None
                                 else 'plane_projection' if c_planes else 'contraction' if a_planes else (range_class or 'gemm')]
    if dual is not None:
        A2, B32, csum2, bias2 = dual
        if A2.dim() == 2:
            A2 = A2.unsqueeze(0)
        _f32(A2)
        assert A2.stride(2) == 1 and A2.shape[0] == nb and A2.shape[1] == (pair[0] * pair[0] if pair is not None else M)
        K2 = A2.shape[2]
        _weight_planes(B32, N, what='dual B3_2')
        assert B32.shape[0] * 16 == K2 and csum2.numel() == N
        g.b2_exp = B32.w_exp
        g.A2, g.sA2b, g.sA2m, g.K2 = _p(A2), (A2.stride(0) if nb > 1 else 0), A2.stride(1), K2
        g.B2_split, g.sB23k, g.sB23p, g.sB23n = _p(B32), B32.stride(0), B32.stride(1), B32.stride(2)
        g.ln2_csum, g.bias2 = _p(_f32(csum2)), _p(bias2)
        if g.ln_eps == 0:
            g.ln_eps = 1e-5
    if out_ln is not None:
        assert out_ln[0].numel() == N and out_ln[1].numel() == N
        g.out_ln_w, g.out_ln_b = _p(_f32(out_ln[0])), _p(_f32(out_ln[1]))
        g.out_ln_eps = float(out_ln[2]) if len(out_ln) > 2 else 1e-5
    if clock_probe is not None:       # diagnostics: uint64[2] device accumulators (shader ticks, 100 MHz ticks)
        assert clock_probe.dtype == torch.int64 and clock_probe.numel() >= 2
        g.clock_probe = _p(clock_probe)
    g.bias = _p(bias)
    g.alpha = float(alpha)
    g.act = int(act)
    if rowscale is not None:
        rs_rows = pair[0] * pair[1] if c_split_tile else M
        assert rowscale.numel() == nb * rs_rows and rowscale.is_contiguous()
        g.rowscale, g.sRSb = _p(_f32(rowscale)), rs_rows
    if gate is not None:
        if gate.dim() == 2:
            gate = gate.unsqueeze(0)
        cd, sd = (1, 2) if g.c_transposed else (2, 1)
        assert gate.shape == (nb, M if c_planes else Cout.shape[1], N) and gate.stride(cd) == 1, 'gate must be laid out like Cout (mlp: (M, N) rows)'
        g.gate, g.sGb, g.sGm, g.gate_sigmoid = _p(_f32(gate)), (gate.stride(0) if nb > 1 else 0), gate.stride(sd), int(gate_sigmoid)
    if resid is not None:
        if resid.dim() == 2:
            resid = resid.unsqueeze(0)
        cd, sd = (1, 2) if g.c_transposed else (2, 1)
        assert resid.shape == (nb, M if c_planes else Cout.shape[1], No if mlp is not None else N) and resid.stride(cd) == 1, 'resid must be laid out like Cout'
        g.resid, g.sRb, g.sRm = _p(_f32(resid)), (resid.stride(0) if nb > 1 else 0), resid.stride(sd)
    if defer:           # the filled descriptor instead of a launch (gemm_side); the caller keeps the operand tensors alive
        return g
    check(lib.abx_gemm(C.byref(g), _stream()), 'abx_gemm')
    return Cout


def gemm_side(g_main, g_side):
    """abx_gemm_side: two GEMMs over the same rows in one launch (descriptors from gemm(..., defer=True)): a plain-store split-f16
    problem with N % 128 == 0 and a skinny (N <= 32) transposed-store projection whose tiles ride in its grid and read their A panel
    from the L2; bit-identical to the two launches, which is what the library issues when the pair does not qualify."""
    check(_lib.load().abx_gemm_side(C.byref(g_main), C.byref(g_side), _stream()), 'abx_gemm_side')


def planes_to_float(p, a_side, dim=0):
    """int16 activation images (size 2 along `dim`) of the contraction -> the float32 value they stand for: A side (p0 + p1 2^-11) 2^4,
    B side (p0 + p1) 2^-4."""
    h = p.view(torch.float16).float()
    p0, p1 = h.select(dim, 0), h.select(dim, 1)
    return (p0 + p1 / 2048.0) * 16.0 if a_side else (p0 + p1) / 16.0


def row_stats(x, out=None, eps=1e-5):
    """(mean, rstd) per row.  x (rows,K) k-contiguous (dense rows), or x (b, K, rows) channel-major given as a
    (b, rows, K) logical view whose row stride is 1."""
    lib = _lib.load()
    _f32(x)
    if x.dim() == 2:
        rows, K = x.shape
        assert x.stride(1) == 1
        if out is None:
            out = torch.empty(rows, 2, device=x.device, dtype=torch.float32)
        check(lib.abx_row_stats(_p(x), 0, x.stride(0), 1, 1, rows, K, eps, _p(out), _stream()), 'abx_row_stats')
    else:
        nb, rows, K = x.shape
        assert x.stride(1) == 1, 'channel-major layout expected'
        if out is None:
            out = torch.empty(nb * rows, 2, device=x.device, dtype=torch.float32)
        check(lib.abx_row_stats(_p(x), x.stride(0), 1, x.stride(2), nb, rows, K, eps, _p(out), _stream()), 'abx_row_stats')
    return out


def layernorm(x, gamma, beta, out=None, res=None, eps=1e-5):
    lib = _lib.load()
    rows, K = x.shape
    assert x.stride(1) == 1
    if out is None:
        out = torch.empty(rows, K, device=x.device, dtype=torch.float32)
    check(lib.abx_layernorm(_p(_f32(x)), x.stride(0), rows, K, _p(gamma), _p(beta), eps, _p(out), out.stride(0),
                            _p(res), res.stride(0) if res is not None else 0, _stream()), 'abx_layernorm')
    return out


def transpose_last2(x, out, transpose=True):
    """x (n, L, L) -> out (n, L, Lp): out[n, a, b] = x[n, b, a] (or x[n, a, b] when transpose=False), pad columns b >= L zeroed."""
    L, Lp = x.shape[-1], out.shape[-1]
    assert x.shape[-2] == L and x.is_contiguous() and out.is_contiguous() and out.shape[:-1] == x.shape[:-1] and Lp >= L
    check(_lib.load().abx_transpose_last2(_p(_f32(x)), _p(out), x.numel() // (L * L), L, Lp, int(bool(transpose)), _stream()),
          'abx_transpose_last2')
    return out


# ---- op-group entry points of the C ABI (include/abx_hip.h, csrc/blocks.hip) ---------------------------------------------------------
class LinearPack:
    """A Linear (optionally with its LayerNorm folded in) packed by abx_pack_linear: .c is the AbxLinearPack, the device buffer it points
    into is kept alive here; .Wt / .csum / .bias / .planes are tensor views of the same memory for the descriptor-level calls."""

    def __init__(self, sources, K, ln=None, permute_k16=False, device=None):
        """sources: list of (W (rows, K), b (rows) or None, glu in {0, 1, 2}); ln: (gamma, beta) of the LayerNorm to fold or None."""
        lib = _lib.load()
        dev = device if device is not None else sources[0][0].device
        N = sum(int(W.shape[0]) for W, _, _ in sources)
        nbytes = int(lib.abx_pack_linear_bytes(K, N))
        self.buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
        off = (-self.buf.data_ptr()) % 256
        base = self.buf[off:off + nbytes]
        keep = []
        arr = (AbxLinearSrc * len(sources))()
        for i, (W, b, glu) in enumerate(sources):
            W = _f32(W).contiguous()
            assert W.shape[1] == K
            keep.append(W)
            arr[i].W, arr[i].rows, arr[i].glu = _p(W), int(W.shape[0]), int(glu)
            if b is not None:
                b = _f32(b).contiguous()
                keep.append(b)
                arr[i].b = _p(b)
        gamma = beta = None
        if ln is not None:
            gamma, beta = _f32(ln[0]).contiguous(), _f32(ln[1]).contiguous()
        self.c = AbxLinearPack()
        check(lib.abx_pack_linear(arr, len(sources), K, _p(gamma), _p(beta), 1 if permute_k16 else 0, base.data_ptr(), C.byref(self.c), _stream()),
              'abx_pack_linear')
        self.K, self.N, self.w_exp = K, N, int(self.c.b_exp)

        def view(ptr, numel, dtype):
            if not ptr:
                return None
            o = ptr - base.data_ptr()
            return base[o:o + numel * torch.empty(0, dtype=dtype).element_size()].view(dtype)

        Kp = (K + 15) // 16 * 16
        self.Wt = view(self.c.Wt, K * N, torch.float32).view(K, N)
        self.csum = view(self.c.csum, N, torch.float32)
        self.bias = view(self.c.bias, N, torch.float32)
        pl = view(self.c.planes, Kp * 2 * N, torch.float16).view(Kp // 16, 2, N, 16).as_subclass(WeightPlanes)
        pl.w_exp = self.w_exp
        self.planes = pl


def _range_args(exact, name):
    if RANGE_CHECK and not exact:
        return range_ptr(torch.device('cuda', torch.cuda.current_device())), RANGE_TAGS[name]
    return None, 0


def transition_fwd(l1, l2, z, exact=False, workspace=None):
    """pair Transition in place on z (M, C) through abx_transition_fwd (one launch on the split-f16 path)."""
    lib = _lib.load()
    M = z.shape[0]
    assert z.is_contiguous() and z.shape[1] == l1.K
    if exact:
        need = int(lib.abx_transition_workspace_bytes(M, l1.N, 1))
        assert workspace is not None and workspace.numel() * workspace.element_size() >= need
    rf, rt = _range_args(exact, 'pair_transition')
    check(lib.abx_transition_fwd(C.byref(l1.c), C.byref(l2.c), _p(z), M, int(bool(exact)), _p(workspace), rf, rt, _stream()), 'abx_transition_fwd')
    return z


def tri_mul_pack(glu, out, gate):
    p = AbxTriMulPack()
    p.glu, p.out, p.gate = glu.c, out.c, gate.c
    p._keep = (glu, out, gate)
    return p


def tri_mul_workspace(B, L, device):
    """(workspace tensor, initialised) for abx_tri_mul_fwd: the operand-image region is zero-filled once."""
    lib = _lib.load()
    ws = torch.empty(int(lib.abx_tri_mul_workspace_bytes(B, L)) + 256, dtype=torch.uint8, device=device)
    ws = ws[(-ws.data_ptr()) % 256:]
    check(lib.abx_tri_mul_workspace_init(_p(ws), B, L, _stream()), 'abx_tri_mul_workspace_init')
    return ws


def tri_mul_workspace_init(ws, B, L):
    """Zero the operand-image region of a tri-mul workspace for the layout of B samples (a buffer reused with another chunk size)."""
    check(_lib.load().abx_tri_mul_workspace_init(_p(ws), B, L, _stream()), 'abx_tri_mul_workspace_init')


def tri_mul_fwd(pack, z_in, z_out, mask_f, B, L, outgoing, workspace):
    lib = _lib.load()
    assert z_in.is_contiguous() and z_out.is_contiguous() and z_in.data_ptr() != z_out.data_ptr()
    rf, rt = _range_args(False, 'contraction')
    check(lib.abx_tri_mul_fwd(C.byref(pack), _p(z_in), _p(z_out), _p(_f32(mask_f)), B, L, int(bool(outgoing)), _p(workspace), rf, rt, _stream()),
          'abx_tri_mul_fwd')
    return z_out


class TriRowPack:
    """Head-major image of a q | k | v LinearPack (abx_tri_rowpack) for the row-fused triangle attention: .c is the AbxTriRowPack, the device
    buffer it points into is kept alive here together with the source pack."""

    def __init__(self, qkv):
        lib = _lib.load()
        nbytes = int(lib.abx_tri_rowpack_bytes())
        self.buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=qkv.buf.device)
        off = (-self.buf.data_ptr()) % 256
        self.c = AbxTriRowPack()
        check(lib.abx_tri_rowpack(C.byref(qkv.c), self.buf[off:].data_ptr(), C.byref(self.c), _stream()), 'abx_tri_rowpack')
        self.qkv = qkv


def tri_attn_pack(qkv, gate, pair, out):
    p = AbxTriAttnPack()
    p.qkv, p.gate, p.pair, p.out = qkv.c, gate.c, pair.c, out.c
    p._keep = (qkv, gate, pair, out)
    p._row = None
    if qkv.buf.is_cuda and qkv.K == 192 and qkv.N == 576 and qkv.c.csum:
        p._row = TriRowPack(qkv)                    # (the row-fused route of abx_tri_attn_block_fwd / tri_attn(z rows, rowpack=))
        p.row = p._row.c
    return p


def tri_attn_block_workspace(B, L, device):
    ws = torch.empty(int(_lib.load().abx_tri_attn_block_workspace_bytes(B, L)) + 256, dtype=torch.uint8, device=device)
    return ws[(-ws.data_ptr()) % 256:]


def tri_attn_block_fwd(pack, z, mask_f, B, L, per_row, workspace, exact=False, attn_exact=None):
    """exact: the three GEMMs on the exact kernels; attn_exact: the attention kernel (default: the global GEMM_EXACT switch, as tri_attn)."""
    lib = _lib.load()
    ax = bool(GEMM_EXACT if attn_exact is None else attn_exact)
    ex = int(bool(exact)) | (2 if ax else 0)
    rf, rt = _range_args(ex == 3, 'tri_attn')
    check(lib.abx_tri_attn_block_fwd(C.byref(pack), _p(z), _p(_f32(mask_f)), B, L, int(bool(per_row)), ex, _p(workspace), rf, rt, _stream()),
          'abx_tri_attn_block_fwd')
    return z


def _tri_rowfused_ok(L):
    """True when the library takes the row-fused triangle attention for rows of length L (abx_tri_attn_rowfused_ok: L <= 352 and the
    ABX_NO_TRI_ROWFUSED switch, which only the C side reads - abx_tri_attn_block_fwd and the descriptor-level path ask the same function)."""
    return bool(_lib.load().abx_tri_attn_rowfused_ok(int(L)))


def tri_row_touch(v=-1):
    """How the row-fused kernel's issuing wave warms the L2 with the z rows (abx_tri_row_touch): 0 none, 1 the whole next row a phase ahead,
    2 per k-group just ahead of the walk.  v = 0 | 1 | 2 sets it for later launches of this process, anything else only asks; returns the
    setting that held before.  The start value is the library's (ABX_TRI_ROW_TOUCH, read on the C side only).  Same bits for all three."""
    return int(_lib.load().abx_tri_row_touch(int(v)))


_TRI_ATTN_LAST = None       # (L, exact, row-fused) of the most recent tri_attn launch: what a caller that times launches asks the name of


def tri_attn_kernel_name(L, exact=None, bias_vec=True, rowfused=None):
    """Name of the kernel the triangle attention of a row of length L runs on, for per-kernel aggregation: the library's answer
    (abx_tri_attn_plan, the dispatch of csrc/attention.hip itself) for one sample in the model's row layout - projected q | k | v rows 576 wide,
    4 heads, key-contiguous bias rows padded to 4 floats (bias_vec=False: query-contiguous, unpadded).
    rowfused: True = tri_attn on the z rows with a row pack (abx_tri_attn_rowfused_fwd), False = tri_attn on projected
    q | k | v rows (abx_tri_attn_fwd); None = whatever the most recent tri_attn call of this (L, exact) launched - the caller that times a
    launch asks right behind it - and, with no such call, what the model path does for a complex of this length: the fused kernel when the
    library admits L (abx_tri_attn_rowfused_ok: a function of L and of the ABX_NO_TRI_ROWFUSED switch, read on the C side only), the GEMMs
    of the pass are the split-f16 ones (gemm_mode) and the k | v operand images are off."""
    ex = bool(GEMM_EXACT if exact is None else exact)
    if rowfused is None:
        if _TRI_ATTN_LAST is not None and _TRI_ATTN_LAST[:2] == (int(L), ex):
            rowfused = _TRI_ATTN_LAST[2]
        else:
            rowfused = not ex and _tri_rowfused_ok(L) and gemm_mode(L) == 2 and not KV_PLANES
    P = _placeholders()
    H, D, W, Lp = 4, 48, 576, ((L + 3) // 4 * 4 if bias_vec else L)
    a = AbxTriAttn()
    base = next(P)
    a.q, a.k, a.v, a.sb, a.ss, a.sl = base, base + 4 * H * D, base + 8 * H * D, L * L * W, L * W, W
    a.bias, a.bias_sb, a.bias_sh = next(P), H * L * Lp, L * Lp
    a.bias_sq, a.bias_sk = (Lp, 1) if bias_vec else (1, L)
    a.out, a.ob, a.os, a.ol = next(P), L * L * H * D, L * H * D, H * D
    a.B, a.S, a.L, a.H, a.D, a.exact = 1, L, L, H, D, int(ex)
    rc, name = _plan_name(_lib.load().abx_tri_attn_plan, C.byref(a), int(bool(rowfused)))
    check(rc, 'abx_tri_attn_plan')
    return name


# float(log2 e) * 2^7 (include/abx_hip.h ABX_TRI_BIAS_LOG2): the factor the pair-bias projection applies (gemm(..., alpha=)) when the attention
# that reads it runs with bias_log2=True
TRI_BIAS_LOG2 = float(__import__('numpy').float32(1.4426950408889634) * __import__('numpy').float32(128.0))


KV_PLANES = env_on('ABX_KV_PLANES')       # round-6 experiment, off by default (measured slower: profiles/r06h_kb_kvplanes.txt)


def kv_planes_ok(M):
    """True when a q | k | v projection over M pair rows may write its k | v columns as operand images (gemm(..., c_plane_cols=(192, 48)) through
    gemm_side) for tri_attn(..., kv_planes=True): the launch takes the A-stationary kernel (abx_gemm_planes_ok)."""
    return bool(_lib.load().abx_gemm_planes_ok(int(M))) and not GEMM_EXACT and not (GEMM_TUNE & 2048)


def tri_attn(qkvg, biasT, keymask, out, B, L, per_row, H=4, D=48, bias_is_qk=False, exact=None, clock_probe=None, tune=0, bias_log2=False, kv_planes=False,
             rowpack=None, slot_order=-1):
    """qkvg (B*L*L, 4*H*D) = [q|k|v|gate], or (B*L*L, 3*H*D) = [q|k|v]: no gate (the gated tail applies it: gemm(..., mlp=, gate=));
    or the pair rows z (B*L*L, H*D = 192) themselves with rowpack = the TriRowPack of the LayerNorm-folded q | k | v projection: the
    row-fused kernel projects q | k | v of a row inside the attention (abx_tri_attn_rowfused_fwd: L <= 352, split-f16, bias_is_qk rows;
    bit-identical to gemm + tri_attn on the projected rows); slot_order: -1 library default, 0 = (b, row, h), 1 = (b, h, row);
    biasT (B,H,L,L) projected from the UNtransposed pair tensor (bias_is_qk=False) or
    already laid out [b,h,q,k] for this orientation (bias_is_qk=True; then (B,H,L,Lp) with rows padded to Lp % 4 == 0 floats gives
    the kernel 16-byte bias loads for any L); out (B*L*L, H*D)."""
    lib = _lib.load()
    W = qkvg.shape[1]
    fused = rowpack is not None
    assert (W == H * D) if fused else (W in (3 * H * D, 4 * H * D)), 'z rows (H*D wide) go with rowpack=, projected rows are 3 or 4 x H*D wide'
    assert qkvg.is_contiguous() and out.is_contiguous() and biasT.is_contiguous()
    a = AbxTriAttn()
    es = qkvg.element_size()
    base = qkvg.data_ptr()
    if not fused:
        a.q, a.k, a.v = base, base + H * D * es, base + 2 * H * D * es
    if W == 4 * H * D:
        a.gate = base + 3 * H * D * es
    a.sb = L * L * W
    a.ss, a.sl = (L * W, W) if per_row else (W, L * W)
    a.bias = _p(biasT)
    Lp = biasT.shape[-1] if (biasT.dim() == 4 and bias_is_qk) else L       # (B,H,L,Lp): key-contiguous rows padded to Lp floats
    assert biasT.numel() == B * H * L * Lp
    a.bias_sb, a.bias_sh = H * L * Lp, L * Lp
    a.bias_sq, a.bias_sk = (Lp, 1) if (per_row or bias_is_qk) else (1, L)
    if keymask is not None:
        a.keymask, a.km_sb = _p(_f32(keymask)), L
    C_ = H * D
    a.out, a.ob = _p(out), L * L * C_
    a.os, a.ol = (L * C_, C_) if per_row else (C_, L * C_)
    a.B, a.S, a.L, a.H, a.D = B, L, L, H, D
    a.scale = float(D ** (-0.5))
    a.exact = int(GEMM_EXACT if exact is None else exact)
    a.tune = int(tune)
    a.bias_log2 = int(bool(bias_log2))              # biasT = TRI_BIAS_LOG2 x the pair bias (AbxTriAttn.bias_log2)
    a.kv_planes = int(bool(kv_planes))              # k | v columns hold the operand images of AbxGemm.c_planes_from, not fp32 (AbxTriAttn.kv_planes)
    if RANGE_CHECK and not a.exact:
        a.range_flag, a.range_tag = range_ptr(out.device), RANGE_TAGS['tri_attn']
    if clock_probe is not None:
        assert clock_probe.dtype == torch.int64 and clock_probe.numel() >= 2
        a.clock_probe = _p(clock_probe)
    global _TRI_ATTN_LAST
    _TRI_ATTN_LAST = (int(L), bool(a.exact), fused)
    if fused:
        assert not kv_planes and not a.exact and not tune, 'the row-fused kernel: split-f16, no operand images, no tune bits'
        check(lib.abx_tri_attn_rowfused_fwd(C.byref(a), base, a.sb, a.ss, a.sl, C.byref(rowpack.c), int(slot_order), _stream()), 'abx_tri_attn_rowfused_fwd')
        return out
    check(lib.abx_tri_attn_fwd(C.byref(a), _stream()), 'abx_tri_attn_fwd')
    return out


def seq_attn_kernel_name(L, with_qblk=False):
    """Name of the seq_attn2_kernel instantiation abx_seq_attn_fwd launches for a complex of length L - the library's answer
    (abx_seq_attn_plan: the dispatch of csrc/attention.hip itself, run up to the launch; needs no GPU).  with_qblk: (name, query rows per
    workgroup) - the queries are split over ceil(L / qblk) workgroups per (sample, head).  A length the entry point refuses raises as it does."""
    qblk = C.c_int(0)
    rc, name = _plan_name(lambda b, n: _lib.load().abx_seq_attn_plan(int(L), b, n, C.byref(qblk)))
    check(rc, 'abx_seq_attn_plan')
    return (name, int(qblk.value)) if with_qblk else name


def seq_attn(qkv, biasT, keymask, gate, out, B, L, H=32, D=17):
    lib = _lib.load()
    assert qkv.is_contiguous() and biasT.is_contiguous() and gate.is_contiguous() and out.is_contiguous()
    check(lib.abx_seq_attn_fwd(_p(qkv), _p(biasT), _p(keymask), _p(gate), _p(out), B, L, H, D, float(D ** (-0.5)), _stream()),
          'abx_seq_attn_fwd')
    return out


def ipa_weights(qpack, kpack, vpack, bias2d, mask, rots, trans, pw, attn_ws, feat, B, L):
    """First launch of the IPA core: attention weights -> attn_ws, scalar / point outputs -> feat[:, :576]."""
    assert attn_ws.numel() >= B * L * L * 12 and attn_ws.is_contiguous()
    check(_lib.load().abx_ipa_weights(_p(qpack), _p(kpack), _p(vpack), _p(bias2d), _p(mask), _p(rots), _p(trans), _p(pw), _p(attn_ws),
                                      _p(feat), B, L, _stream()), 'abx_ipa_weights')


def ipa_pair(attn_ws, z, feat, B, L):
    """Second launch: attention over the pair slab z (B*L*L, 128) -> feat[:, 576:]."""
    check(_lib.load().abx_ipa_pair(_p(attn_ws), _p(z), _p(feat), B, L, _stream()), 'abx_ipa_pair')


def gemm_splitk(A, w3, partial, range_class='gemm'):
    """K-slice products of A (M, K) fp32 rows against split_weights planes w3 of a (K, N) weight: partial[s] = A[:, s*Ks:(s+1)*Ks] @
    W[s*Ks:(s+1)*Ks] for the S = partial.shape[0] slices (Ks = K / S a multiple of 16), ONE abx_gemm launch with batch = slice (operand
    windows by batch strides; split-f16 arithmetic).  The caller adds the slices in a fixed order (abx_ipa_tail's `partial` input): a
    long-K, few-row GEMM becomes S times as many blocks with a 1 / S as long k loop."""
    S, M, N = partial.shape
    K = A.shape[1]
    assert A.shape[0] == M and A.stride(1) == 1 and partial.is_contiguous() and K % (16 * S) == 0
    _weight_planes(w3, N, K, what='gemm_splitk')
    assert w3.shape[0] * 16 == K
    Ks = K // S
    g = AbxGemm()
    g.A, g.sAb, g.sAm, g.sAk = _p(_f32(A)), Ks, A.stride(0), 1
    g.B_split, g.sB3b, g.sB3k, g.sB3p, g.sB3n = _p(w3), (Ks // 16) * w3.stride(0), w3.stride(0), w3.stride(1), w3.stride(2)
    g.b_f16, g.b_exp = 1, w3.w_exp
    g.C, g.sCb, g.sCm = _p(_f32(partial)), M * N, N
    g.M, g.N, g.K, g.batch = M, N, Ks, S
    g.alpha, g.exact = 1.0, 2
    if RANGE_CHECK:
        g.range_flag, g.range_tag = range_ptr(A.device), RANGE_TAGS[range_class]
    check(_lib.load().abx_gemm(C.byref(g), _stream()), 'abx_gemm(split-K)')
    return partial


def ipa_tail(feat, s, w_final, ln1, w_t0, w_t2, w_t4, ln2, eps=1e-5, affine=None, rigid=None, partial=None):
    """The tail of an IPA layer in one launch (csrc/gemm3.hip ipa_tail_kernel; reference score_network.py:126-163):
    s <- LN1(s + feat @ W_final + b_final);  s <- LN2(s + relu(relu(s @ W0 + b0) @ W2 + b2) @ W4 + b4), in place.
    feat (M, K1) and s (M, 256) fp32 rows; w_* = (WeightPlanes of the (K, 256) weight, bias (256)); ln* = (gamma, beta).
    affine = (Wt (256, 6) fp32, bias (6)) with rigid = (fixed_i32, init_q, init_t, cur_q, cur_t, cur_R, delta_q, position_scale): also
    affine_update of the new s and the frame update of rigid_update() in the same launch.
    partial (S, M, 256): feat @ W_final already computed as S K-slice products (gemm_splitk); the kernel adds them instead of walking K1."""
    M, K1 = feat.shape
    assert s.shape == (M, 256) and feat.stride(1) == 1 and s.stride(1) == 1 and K1 % 16 == 0
    a = AbxIpaTail()
    a.feat, a.s_feat, a.s, a.s_s, a.M, a.K1, a.C = _p(_f32(feat)), feat.stride(0), _p(_f32(s)), s.stride(0), M, K1, 256
    if partial is not None:       # feat @ W_final as K-slice products (gemm_splitk), summed by the kernel in slice order
        assert partial.dim() == 3 and partial.shape[1:] == (M, 256) and partial.is_contiguous()
        a.partial, a.n_partial, a.s_partial = _p(_f32(partial)), partial.shape[0], M * 256
    for tag, (w3, bias), K in (('final', w_final, K1), ('t0', w_t0, 256), ('t2', w_t2, 256), ('t4', w_t4, 256)):
        _weight_planes(w3, 256, K, what='ipa_tail ' + tag)
        assert w3.shape[0] * 16 == K and bias.numel() == 256
        setattr(a, 'W_' + tag, _p(w3)); setattr(a, 'e_' + tag, w3.w_exp); setattr(a, 'b_' + tag, _p(_f32(bias)))
    a.ln1_w, a.ln1_b, a.ln2_w, a.ln2_b = _p(_f32(ln1[0])), _p(_f32(ln1[1])), _p(_f32(ln2[0])), _p(_f32(ln2[1]))
    a.ln_eps = float(eps)
    if affine is not None:
        wa, ba = affine
        fixed, init_q, init_t, cur_q, cur_t, cur_R, delta_q, pscale = rigid
        assert wa.shape == (256, 6) and wa.is_contiguous() and ba.numel() == 6 and fixed.dtype == torch.int32 and fixed.numel() == M
        a.W_aff, a.b_aff, a.fixed = _p(_f32(wa)), _p(_f32(ba)), _p(fixed)
        a.init_q, a.init_t, a.cur_q, a.cur_t, a.cur_R, a.delta_q = [_p(_f32(t)) for t in (init_q, init_t, cur_q, cur_t, cur_R, delta_q)]
        a.pscale = float(pscale)
    if RANGE_CHECK:
        a.range_flag, a.range_tag = range_ptr(s.device), RANGE_TAGS['ipa_tail']
    check(_lib.load().abx_ipa_tail(C.byref(a), _stream()), 'abx_ipa_tail')
    return s


def pad_planes_128(wt, bias):
    """(WeightPlanes, bias[128]) of a (K, n <= 128) weight zero-padded to 128 columns: the narrow last projections of abx_heads_tail."""
    K, n = wt.shape
    w = torch.zeros(K, 128, device=wt.device, dtype=torch.float32)
    w[:, :n] = wt
    b = torch.zeros(128, device=wt.device, dtype=torch.float32)
    if bias is not None:
        b[:n] = bias
    return split_weights(w), b


def heads_tail(s, s0, torsion, seq_head, plddt_head, un, logits, pl=None, eps=1e-5):
    """The per-residue heads in one launch (csrc/gemm3.hip heads_tail_kernel; reference sidechain.py:28-62, head.py:143-226).
    s, s0 (M, 256) fp32 rows; torsion = 7 x (WeightPlanes (K, 128), bias [128]): proj_act, proj_init_act, the four ResNet linears, the
    projection padded to 128 columns (pad_planes_128); seq_head / plddt_head = ((gamma, beta), (planes, bias) x 3), last one padded;
    un (M, 14), logits (M, 20), pl (M, 50) contiguous outputs (pl None: the pLDDT head is skipped)."""
    M = s.shape[0]
    assert s.shape == (M, 256) and s0.shape == (M, 256) and s.stride(1) == 1 and s0.stride(1) == 1
    assert un.shape == (M, 14) and un.is_contiguous() and logits.shape == (M, 20) and logits.is_contiguous()
    a = AbxHeadsTail()
    a.s, a.s_s, a.s0, a.s_s0, a.M = _p(_f32(s)), s.stride(0), _p(_f32(s0)), s0.stride(0), M
    keep = []

    def put(tag, wb, K):
        w3, bias = wb
        _weight_planes(w3, 128, K, what='heads_tail ' + tag)
        assert w3.shape[0] * 16 == K and bias.numel() == 128
        setattr(a, 'W_' + tag, _p(w3)); setattr(a, 'e_' + tag, w3.w_exp); setattr(a, 'b_' + tag, _p(_f32(bias)))
        keep.append((w3, bias))
    for tag, wb, K in zip(('act', 'init', 'r0', 'r1', 'r2', 'r3', 'proj'), torsion, (256, 256, 128, 128, 128, 128, 128)):
        put(tag, wb, K)
    (g_s, b_s), *lin_s = seq_head
    a.lns_w, a.lns_b = _p(_f32(g_s)), _p(_f32(b_s))
    for tag, wb, K in zip(('s1', 's3', 's5'), lin_s, (256, 128, 128)):
        put(tag, wb, K)
    a.un, a.logits = _p(_f32(un)), _p(_f32(logits))
    if pl is not None:
        assert pl.shape == (M, 50) and pl.is_contiguous()
        (g_p, b_p), *lin_p = plddt_head
        a.lnp_w, a.lnp_b = _p(_f32(g_p)), _p(_f32(b_p))
        for tag, wb, K in zip(('p1', 'p3', 'p5'), lin_p, (256, 128, 128)):
            put(tag, wb, K)
        a.pl = _p(_f32(pl))
    a.ln_eps = float(eps)
    if RANGE_CHECK:
        a.range_flag, a.range_tag = range_ptr(s.device), RANGE_TAGS['heads_tail']
    check(_lib.load().abx_heads_tail(C.byref(a), _stream()), 'abx_heads_tail')


def ipa_qpack_numel(B, L):
    """floats in the Q pack of abx_ipa_pack (query rows padded to blocks of 12)."""
    return _lib.load().abx_ipa_qpack_bytes(B, L) // 4


def ipa_pack(proj, rots, trans, qpack, kpack, vpack, B, L, w_s):
    assert qpack.numel() >= ipa_qpack_numel(B, L)
    check(_lib.load().abx_ipa_pack(_p(proj), _p(rots), _p(trans), _p(qpack), _p(kpack), _p(vpack), B, L, float(w_s), _stream()),
          'abx_ipa_pack')


def ipa_attn(qpack, kpack, vpack, bias2d, z, mask, rots, trans, pw, feat, B, L, attn_ws=None):
    """attn_ws: (B*L*L, 12) fp32 scratch for the attention weights (allocated here when the caller has no workspace)."""
    if attn_ws is None:
        attn_ws = torch.empty(_lib.load().abx_ipa_attn_workspace_bytes(B, L) // 4, device=feat.device, dtype=torch.float32)
    assert attn_ws.numel() >= B * L * L * 12 and attn_ws.is_contiguous()
    check(_lib.load().abx_ipa_attn(_p(qpack), _p(kpack), _p(vpack), _p(bias2d), _p(z), _p(mask), _p(rots), _p(trans), _p(pw),
                                   _p(attn_ws), _p(feat), B, L, _stream()), 'abx_ipa_attn')


_FREQS = {}


def timestep_embedding(t64, dim, out):
    import math
    assert t64.dtype == torch.float64
    key = (dim, str(t64.device))
    if key not in _FREQS:       # seqformer.py:58-59, computed by torch on the host exactly as the reference does
        half = dim // 2
        _FREQS[key] = torch.exp(torch.arange(half, dtype=torch.float32) * -(math.log(10000) / (half - 1))).to(t64.device)
    check(_lib.load().abx_timestep_embedding(_p(t64), _p(_FREQS[key]), t64.shape[0], dim, _p(out), _stream()),
          'abx_timestep_embedding')
    return out


def assemble_seq(seq_static, aa_table, seq_t, Lab, temb, prev_seq, gamma, beta, out, B, L, C_, E):
    ss_b = 0 if seq_static.shape[0] == 1 else seq_static.stride(0)
    assert seq_t.dtype == torch.int64 and seq_t.is_contiguous()
    check(_lib.load().abx_assemble_seq(_p(seq_static), ss_b, _p(aa_table), _p(seq_t), Lab, _p(temb), _p(prev_seq), _p(gamma),
                                       _p(beta), _p(out), B, L, C_, E, _stream()), 'abx_assemble_seq')
    return out


def assemble_pair(pair_static, temb, prev_pair, gamma, beta, prev_pos, pos_table, out, B, L, C_, E, stats_out=None):
    ps_b = 0 if pair_static.shape[0] == 1 else pair_static.stride(0)
    if prev_pos is not None:
        assert prev_pos.dtype == torch.int64 and prev_pos.is_contiguous()
    check(_lib.load().abx_assemble_pair(_p(pair_static), ps_b, _p(temb), _p(prev_pair), _p(gamma), _p(beta), _p(prev_pos),
                                        _p(pos_table), _p(out), _p(stats_out), B, L, C_, E, _stream()), 'abx_assemble_pair')
    return out


def assemble_pair_bias(pair_static, temb, prev_pair, gamma, beta, prev_pos, pos_table, out, w3, csum, bias, biasT, B, L, range_class='gemm'):
    """abx_assemble_pair_bias: z0 = assemble_pair(...) -> out (B, L, L, 192) and the sequence attention's pair bias
    biasT (B, 32, L*L) = Linear(LayerNorm(z0)) from the SAME pass over the pair rows (w3 = split_weights of the gamma-scaled (192, 32) weight, csum
    its column sums, bias the folded bias: Packed.ln_linear + split_narrow)."""
    ps_b = 0 if pair_static.shape[0] == 1 else pair_static.stride(0)
    assert out.is_contiguous() and out.shape[-1] == 192 and pair_static.shape[-1] == 128 and temb.shape[-1] == 32
    assert tuple(w3.shape) == (12, 2, 32, 16) and biasT.is_contiguous() and biasT.numel() == B * 32 * L * L and csum.numel() == 32
    if prev_pos is not None:
        assert prev_pos.dtype == torch.int64 and prev_pos.is_contiguous()
    flag, tag = (range_ptr(out.device), RANGE_TAGS[range_class]) if RANGE_CHECK else (None, 0)
    check(_lib.load().abx_assemble_pair_bias(_p(pair_static), ps_b, _p(temb), _p(prev_pair), _p(gamma), _p(beta), _p(prev_pos), _p(pos_table), _p(out),
                                             _p(w3), w3.w_exp, _p(_f32(csum)), _p(bias), 1e-5, _p(biasT), B, L, flag, tag, _stream()),
          'abx_assemble_pair_bias')
    return out


def opm_features(lr, feat, B, L, C_=64):
    """lr (B*L, 2*C) = [left | right] (already masked)."""
    es = lr.element_size()
    check(_lib.load().abx_opm_features(lr.data_ptr(), lr.data_ptr() + C_ * es, lr.stride(0), _p(feat), B, L, C_, _stream()),
          'abx_opm_features')
    return feat


def opm_out(lr, Wt, bias, z, B, L, range_class='gemm'):
    """OuterProductMean without its feature tensor (abx_opm_out_fwd): z (B*L*L, 192) += out_proj([l_j * r_i | l_j - r_i]) with lr (B*L, 128) =
    [left | right] (already masked) and Wt = out_proj.weight^T (128, 192); split-f16 arithmetic, range-tagged like the GEMMs."""
    assert lr.shape[1] == 128 and tuple(Wt.shape) == (128, 192) and Wt.is_contiguous() and z.is_contiguous() and z.shape[-1] == 192
    flag, tag = (range_ptr(z.device), RANGE_TAGS[range_class]) if RANGE_CHECK else (None, 0)
    check(_lib.load().abx_opm_out_fwd(_p(_f32(lr)), lr.stride(0), _p(_f32(Wt)), _p(bias), _p(_f32(z)), B, L, flag, tag, _stream()), 'abx_opm_out_fwd')
    return z


def pair_mask(mask_f, out, B, L, Lp=None):
    """out (B, L, Lp) = mask_i * mask_j, zero in the pad columns j >= L (Lp defaults to L)."""
    check(_lib.load().abx_pair_mask(_p(mask_f), _p(out), B, L, L if Lp is None else Lp, _stream()), 'abx_pair_mask')
    return out


def gather_rows(table, idx, out, rowscale=None):
    """out[r, :C] = table[idx[r]] (* rowscale[r]); out may be a column window of a wider buffer."""
    idx = idx.reshape(-1)
    assert idx.dtype == torch.int64 and idx.is_contiguous() and table.is_contiguous()
    n, C_ = idx.numel(), table.shape[1]
    check(_lib.load().abx_gather_rows(_p(table), _p(idx), _p(rowscale), _p(out), out.stride(0), n, C_, _stream()), 'abx_gather_rows')
    return out


def relpos_block(residx, table, out, B, L, Lab, max_rel):
    assert residx.dtype == torch.int32 and residx.is_contiguous()
    check(_lib.load().abx_relpos_block(_p(residx), _p(table), _p(out), B, L, Lab, table.shape[1], max_rel, _stream()),
          'abx_relpos_block')
    return out


def pair_embed_features(aa, chain_id, residx, atom14, exists_u8, aa_pair_embed, relpos_embed, distcoef, dgram_embed, sq_breaks,
                        feat512, dist196, B, L):
    assert aa.dtype == torch.int64 and chain_id.dtype == torch.int32 and residx.dtype == torch.int32 and exists_u8.dtype == torch.uint8
    check(_lib.load().abx_pair_embed_features(_p(aa), _p(chain_id), _p(residx), _p(atom14), _p(exists_u8), _p(aa_pair_embed),
                                              _p(relpos_embed), _p(distcoef), _p(dgram_embed), _p(sq_breaks), _p(feat512),
                                              _p(dist196), B, L, _stream()), 'abx_pair_embed_features')


def frames_init(rigids_t, init_q, init_t, cur_q, cur_t, cur_R, delta_q, n, pscale):
    assert rigids_t.is_contiguous() and rigids_t.dtype in (torch.float32, torch.float64)
    check(_lib.load().abx_frames_init(_p(rigids_t), int(rigids_t.dtype == torch.float64), _p(init_q), _p(init_t), _p(cur_q),
                                      _p(cur_t), _p(cur_R), _p(delta_q), n, float(pscale), _stream()), 'abx_frames_init')


def rigid_update(upd6, fixed_i32, init_q, init_t, cur_q, cur_t, cur_R, delta_q, n, pscale):
    assert fixed_i32.dtype == torch.int32
    check(_lib.load().abx_rigid_update(_p(upd6), _p(fixed_i32), _p(init_q), _p(init_t), _p(cur_q), _p(cur_t), _p(cur_R),
                                       _p(delta_q), n, float(pscale), _stream()), 'abx_rigid_update')


def scores(**kw):
    a = AbxScoreArgs()
    for k, v in kw.items():
        setattr(a, k, _p(v) if torch.is_tensor(v) else v)
    check(_lib.load().abx_scores(C.byref(a), _stream()), 'abx_scores')


def torsion_finalize(unnorm, gt, fixed_i32, angles, n):
    check(_lib.load().abx_torsion_finalize(_p(unnorm), _p(gt), _p(fixed_i32), _p(angles), n, _stream()), 'abx_torsion_finalize')


def seq_head_atoms(logits, fixed_i32, seq_t, rigids, angles, a37to14, dframes, gidx, lit, seq_0, atom14, atom37, n, seq_bias=None, L=None):
    """seq_bias: None, or the (L,20) float32 device table of abx_amd.constraints (row i % L for residue i): abx_seq_head_atoms_biased."""
    assert seq_t.dtype == torch.int64 and a37to14.dtype == torch.int64 and gidx.dtype == torch.int32
    if seq_bias is not None:
        L = seq_bias.shape[0] if L is None else int(L)
        assert seq_bias.dtype == torch.float32 and seq_bias.is_cuda and seq_bias.is_contiguous() and tuple(seq_bias.shape) == (L, 20), \
            (seq_bias.dtype, tuple(seq_bias.shape), L)
        assert n % L == 0, (n, L)
        check(_lib.load().abx_seq_head_atoms_biased(_p(logits), _p(fixed_i32), _p(seq_t), _p(rigids), _p(angles), _p(a37to14), _p(dframes),
                                                    _p(gidx), _p(lit), _p(seq_0), _p(atom14), _p(atom37), n, _p(seq_bias), L, _stream()),
              'abx_seq_head_atoms_biased')
        return
    check(_lib.load().abx_seq_head_atoms(_p(logits), _p(fixed_i32), _p(seq_t), _p(rigids), _p(angles), _p(a37to14), _p(dframes),
                                         _p(gidx), _p(lit), _p(seq_0), _p(atom14), _p(atom37), n, _stream()), 'abx_seq_head_atoms')


def prev_pos(atom37, sq_breaks, out, B, L):
    assert out.dtype == torch.int64
    check(_lib.load().abx_prev_pos(_p(atom37), _p(sq_breaks), sq_breaks.numel(), _p(out), B, L, _stream()), 'abx_prev_pos')
    return out


def plddt(logits, out, n, bins):
    check(_lib.load().abx_plddt(_p(logits), _p(out), n, bins, _stream()), 'abx_plddt')
    return out


def igso3_tables(sigma, omega, pdf, cdf, score_norms, L_terms=1000):
    check(_lib.load().abx_igso3_tables(_p(sigma), _p(omega), sigma.numel(), omega.numel(), L_terms, _p(pdf), _p(cdf),
                                       _p(score_norms), _stream()), 'abx_igso3_tables')


def reverse_step(**kw):
    """Keywords = the fields of AbxReverseArgs (include/abx_hip.h); seq_bias: the (L,20) float32 device table of abx_amd.constraints."""
    a = AbxReverseArgs()
    sb = kw.get('seq_bias')
    if sb is not None:
        assert sb.dtype == torch.float32 and sb.is_cuda and sb.is_contiguous() and tuple(sb.shape) == (kw['L'], 20), (sb.dtype, tuple(sb.shape))
    for k, v in kw.items():
        setattr(a, k, _p(v) if torch.is_tensor(v) else v)
    check(_lib.load().abx_reverse_step(C.byref(a), _stream()), 'abx_reverse_step')


_VDW = {'C': 1.7, 'N': 1.55, 'O': 1.52, 'S': 1.8}       # abx/common/residue_constants.py:381-386
_RADIUS = {}


def vdw_radius_table(device):
    """(21, 14) van-der-Waals radius of every atom14 slot by element (0 for empty slots)."""
    key = str(device)
    if key not in _RADIUS:
        from abx_amd import residue_constants as rc
        t = torch.zeros(21, 14)
        for i, r in enumerate(rc.restypes):
            for j, name in enumerate(rc.restype_name_to_atom14_names[rc.restype_1to3[r]]):
                if name:
                    t[i, j] = _VDW[name[0]]
        _RADIUS[key] = t.to(device).contiguous()
    return _RADIUS[key]


_A14MASK = {}


def atom14_mask_table(device):
    """(21, 14) bool: which atom14 slots a residue type fills (cached per device: no host-to-device copy on the step path)."""
    key = str(device)
    if key not in _A14MASK:
        from abx_amd import residue_constants as rc
        _A14MASK[key] = torch.as_tensor(rc.restype_atom14_mask).to(device=device, dtype=torch.bool).contiguous()
    return _A14MASK[key]


def clash_grad(atom14, atom_mask, aatype, chain_id, frame_trans, overlap_tolerance=1.5, between_chain_factor=0.2,
               bond_tolerance_factor=12.0, w_clash=1.0, w_bond=1.0, w_angle=1.0, residx=None):
    """Violation energies and gradients (abx_clash_grad).  atom14 (B,L,14,3) f32, atom_mask (B,L,14), aatype (B,L) int64,
    chain_id (B,L) int32, frame_trans (B,L,3); residx (B,L) int32 or None (None: neighbours are linked by chain id alone, the
    rule of cal_vio.py:51).  -> energy (B,3) [clash, bond, angle], grad_atom (B,L,14,3), grad_trans, grad_rot (B,L,3)."""
    lib = _lib.load()
    B, L = aatype.shape
    dev = atom14.device
    a = AbxGuidanceArgs()
    x = _f32(atom14).contiguous()
    m = atom_mask.to(torch.uint8).contiguous()
    aa = aatype.to(torch.int64).contiguous()
    ch = chain_id.to(torch.int32).contiguous()
    ft = _f32(frame_trans).contiguous()
    energy = torch.empty(B, 3, device=dev)
    g_atom = torch.empty(B, L, 14, 3, device=dev)
    g_t = torch.empty(B, L, 3, device=dev)
    g_r = torch.empty(B, L, 3, device=dev)
    ws = torch.empty(max(int(lib.abx_clash_grad_workspace_bytes(B, L)) // 4, 1), device=dev)
    a.atom14, a.atom_mask, a.aatype, a.chain_id, a.radius, a.frame_trans = _p(x), _p(m), _p(aa), _p(ch), _p(vdw_radius_table(dev)), _p(ft)
    if residx is not None:
        ri = residx.to(torch.int32).contiguous()
        a.residx = _p(ri)
    a.overlap_tolerance, a.between_chain_factor, a.bond_tolerance_factor = float(overlap_tolerance), float(between_chain_factor), float(bond_tolerance_factor)
    a.w_clash, a.w_bond, a.w_angle = float(w_clash), float(w_bond), float(w_angle)
    a.energy, a.grad_atom, a.grad_trans, a.grad_rot = _p(energy), _p(g_atom), _p(g_t), _p(g_r)
    a.B, a.L = B, L
    check(lib.abx_clash_grad(C.byref(a), _p(ws), _stream()), 'abx_clash_grad')
    return energy, g_atom, g_t, g_r


class ContactTables:
    """The hotspot rows and the restraint table of abx_contact_grad, built once: device copies for the kernels, host copies for the
    argument checks (no host-to-device copy on the step path).  hotspots: H <= 64 row indices; restraints: None or (idx (R,4) of
    row_i, slot_i, row_j, slot_j; par (R,3) of lo, hi, weight), R <= 256."""

    def __init__(self, device, hotspots=None, restraints=None):
        hot = torch.as_tensor([] if hotspots is None else hotspots, dtype=torch.int32).reshape(-1)
        idx, par = (torch.zeros(0, 4), torch.zeros(0, 3)) if restraints is None else restraints
        self.hot_host = hot.cpu().contiguous()
        self.idx_host = torch.as_tensor(idx).to(torch.int32).reshape(-1, 4).cpu().contiguous()
        self.par_host = torch.as_tensor(par).to(torch.float32).reshape(-1, 3).cpu().contiguous()
        assert self.idx_host.shape[0] == self.par_host.shape[0], (self.idx_host.shape, self.par_host.shape)
        self.H, self.R = int(self.hot_host.numel()), int(self.idx_host.shape[0])
        self.hot = self.hot_host.to(device) if self.H else None
        self.idx = self.idx_host.to(device) if self.R else None
        self.par = self.par_host.to(device) if self.R else None


def contact_grad(atom14, atom_mask, moved, target, frame_trans, tables=None, w_contact=0.0, d0=4.0, d1=8.0, w_hot=1.0, d_hot=8.0, beta=1.0):
    """Interface guidance energies and gradients (abx_contact_grad).  atom14 (B,L,14,3) f32 and atom_mask (B,L,14): per row the predicted
    atoms where moved (B,L) is set, the ground truth elsewhere; target (L): the partner rows; frame_trans (B,L,3); tables: a
    ContactTables or None.  -> energy (B,3) [contact, hotspot, restraint], grad_atom (B,L,14,3), grad_trans, grad_rot (B,L,3)."""
    lib = _lib.load()
    B, L = moved.shape
    dev = atom14.device
    a = AbxContactArgs()
    x = _f32(atom14).contiguous()
    m = atom_mask.to(torch.uint8).contiguous()
    mv = moved.to(torch.uint8).contiguous()
    tg = target.to(torch.uint8).contiguous()
    ft = _f32(frame_trans).contiguous()
    assert tuple(x.shape) == (B, L, 14, 3) and tuple(m.shape) == (B, L, 14) and tuple(tg.shape) == (L,) and tuple(ft.shape) == (B, L, 3)
    H, R = (tables.H, tables.R) if tables is not None else (0, 0)
    energy = torch.empty(B, 3, device=dev)
    g_atom = torch.empty(B, L, 14, 3, device=dev)
    g_t = torch.empty(B, L, 3, device=dev)
    g_r = torch.empty(B, L, 3, device=dev)
    ws = torch.empty(max(int(lib.abx_contact_grad_workspace_bytes(B, L, H)) // 4, 1), device=dev)
    a.atom14, a.atom_mask, a.moved, a.target, a.frame_trans = _p(x), _p(m), _p(mv), _p(tg), _p(ft)
    if H:
        a.hotspots, a.hotspots_host = _p(tables.hot), tables.hot_host.data_ptr()
    if R:
        a.restr_idx, a.restr_idx_host = _p(tables.idx), tables.idx_host.data_ptr()
        a.restr_par, a.restr_par_host = _p(tables.par), tables.par_host.data_ptr()
    a.w_contact, a.d0, a.d1, a.w_hot, a.d_hot, a.beta = float(w_contact), float(d0), float(d1), float(w_hot), float(d_hot), float(beta)
    a.energy, a.grad_atom, a.grad_trans, a.grad_rot = _p(energy), _p(g_atom), _p(g_t), _p(g_r)
    a.B, a.L, a.H, a.R = B, L, H, R
    check(lib.abx_contact_grad(C.byref(a), _p(ws), _stream()), 'abx_contact_grad')
    return energy, g_atom, g_t, g_r


def _structure_args(a, atom14, seq, L, Lab, gt_atom14, gt_seq, gt_exists, mask, res_mask, region=None, lead=None, extra=()):
    """Fill the part of a per-design descriptor that csrc/structure_dev.h reads (pred_*, masks, gt_*, optional region, radius, B, L,
    Lab, Lpred) - the one place where the wrappers check and normalise the structure operands.  lead: the leading shape of the complex
    tensors, (L,) shared by the batch (default) or (B, L) per structure; extra: further tensors of that leading shape.
    -> (B, Lp, Lab, own, keep): own(t, dtype) returns the pointer of a contiguous copy that `keep` holds until the launch."""
    B, Lp = atom14.shape[0], atom14.shape[1]
    Lab = int(seq.shape[1] if Lab is None else Lab)
    lead = (L,) if lead is None else lead
    assert tuple(atom14.shape[2:]) == (14, 3) and seq.shape[0] == B and seq.shape[1] >= Lab, (atom14.shape, seq.shape)
    assert tuple(gt_atom14.shape) == lead + (14, 3) and tuple(gt_exists.shape) == lead + (14,) and tuple(gt_seq.shape) == lead and \
        all(tuple(t.shape) == lead for t in extra), \
        'complex tensors: (L,...) shared by the batch' if lead == (L,) else 'complex tensors: (L,...) shared or (B,L,...) per structure'
    x = _f32(atom14)
    if not x[0].is_contiguous():                        # (a batch-strided view is read in place)
        x = x.contiguous()
    sq = seq if (seq.dtype == torch.int64 and seq.stride(1) == 1) else seq.to(torch.int64).contiguous()
    keep = [x, sq]

    def own(t, dtype):
        t = t.to(dtype).contiguous()
        keep.append(t)
        return _p(t)

    a.pred_atom14, a.pred_sb, a.Lpred = _p(x), x.stride(0), Lp
    a.pred_seq, a.pred_seq_sb = _p(sq), sq.stride(0)
    if mask is not None:
        assert tuple(mask.shape) == (B, L, 14), mask.shape
        a.pred_mask = own(mask, torch.uint8)
    if res_mask is not None:
        assert tuple(res_mask.shape) == (L,), res_mask.shape
        a.res_mask = own(res_mask, torch.uint8)
    a.gt_atom14, a.gt_exists, a.gt_seq = own(_f32(gt_atom14), torch.float32), own(gt_exists, torch.uint8), own(gt_seq, torch.int64)
    if region is not None:
        assert tuple(region.shape) == (L,), region.shape
        a.region = own(region.ne(0), torch.uint8)
    a.radius = _p(vdw_radius_table(atom14.device))
    a.B, a.L, a.Lab = B, L, Lab
    return B, Lp, Lab, own, keep


def _out_rows(a, out, B, cols, device):
    """a.out / a.out_stride: the (B, cols) float64 table, allocated here or the caller's rows (unit column stride, any row stride)."""
    if out is None:
        out = torch.empty(B, cols, dtype=torch.float64, device=device)
    assert out.dtype == torch.float64 and tuple(out.shape) == (B, cols) and out.stride(1) == 1 and out.is_cuda, f'out: (B, {cols}) float64 rows'
    a.out, a.out_stride = _p(out), out.stride(0) if B > 1 else cols
    return out


def _side_output(a, name, t, dtype, shape):
    """An optional contiguous output tensor of a descriptor (points, bonds, rows, counts, contacts): checked and bound when given."""
    if t is not None:
        what = f"{name}: ({','.join(map(str, shape))}) {str(dtype).replace('torch.', '')}"
        assert t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and t.is_cuda, what
        setattr(a, name, _p(t))


def design_scores(atom14, seq, gt_atom14, gt_seq, gt_exists, cdr_def, chain_id, Lab=None, residx=None, mask=None, res_mask=None,
                  overlap_tolerance=1.5, bond_tolerance_factor=12.0, out=None):
    """Per-structure design scores (abx_design_scores; columns: abx_amd.metrics.SCORE_COLUMNS).
    atom14 (B,Lp,14,3) f32 with Lab <= Lp <= L (rows beyond Lp take the ground-truth coordinates; the batch stride is free: a
    [:, :Lab] view of a (B,L,14,3) tensor is read in place), seq (B,>=Lab) int64 predicted tokens.
    The complex, shared by the B structures ((L,...) tensors) or one per structure ((B,L,...)): gt_atom14 (L,14,3) f32, gt_seq (L) int64,
    gt_exists (L,14), chain_id (L) int32, residx (L) int32 or None (None: neighbours are linked by chain id alone); cdr_def (L) int32.
    mask (B,L,14) or None (None: the atoms of the residue types); res_mask (L) or None.
    out: (B, 19) float64 with unit column stride and any row stride (rows of a preallocated table), or None.  No synchronisation."""
    lib = _lib.load()
    dev = atom14.device
    L = cdr_def.shape[-1]
    batched = gt_atom14.dim() == 4
    lead = (atom14.shape[0], L) if batched else (L,)
    assert tuple(cdr_def.shape) == (L,), 'complex tensors: (L,...) shared or (B,L,...) per structure'
    a = AbxDesignScoreArgs()
    B, _, _, own, keep = _structure_args(a, atom14, seq, L, Lab, gt_atom14, gt_seq, gt_exists, mask, res_mask, lead=lead, extra=(chain_id,))
    a.cdr_def, a.chain_id = own(cdr_def, torch.int32), own(chain_id, torch.int32)
    if residx is not None:
        assert tuple(residx.shape) == lead, residx.shape
        a.residx = own(residx, torch.int32)
    a.complex_batched = 1 if batched else 0
    a.overlap_tolerance, a.bond_tolerance_factor = float(overlap_tolerance), float(bond_tolerance_factor)
    out = _out_rows(a, out, B, _lib.SCORE_COLS, dev)
    ws = torch.empty(max(int(lib.abx_design_scores_workspace_bytes(B, L)), 8), dtype=torch.uint8, device=dev)
    check(lib.abx_design_scores(C.byref(a), _p(ws), _stream()), 'abx_design_scores')
    return out


_CHI_TABLES = {}


def chi_tables(device):
    """(chi_axis (21,4,2) int32, rigid_group (21,14) int32) for abx_relax: the atom14 slots of the second and third atom of every chi
    definition (-1 where the residue type has no such chi) and the rigid group of every atom14 slot (cached per device)."""
    key = str(device)
    if key not in _CHI_TABLES:
        from abx_amd import residue_constants as rc
        idx37 = torch.as_tensor(rc.chi_angles_atom_indices).long()[:, :, 1:3]                         # (21, 4, 2) atom37 indices
        a14 = torch.as_tensor(rc.restype_atom37_to_atom14).long()
        axis = torch.gather(a14[:, None, :].expand(-1, 4, -1), 2, idx37)
        axis = torch.where(torch.as_tensor(rc.chi_angles_mask)[:, :, None] > 0, axis, torch.full_like(axis, -1))
        group = torch.as_tensor(rc.restype_atom14_to_rigid_group)
        _CHI_TABLES[key] = (axis.to(device=device, dtype=torch.int32).contiguous(), group.to(device=device, dtype=torch.int32).contiguous())
    return _CHI_TABLES[key]


def relax(atom14, seq, gt_atom14, gt_seq, gt_exists, chain_id, movable, Lab=None, residx=None, mask=None, res_mask=None, n_movable=None,
          overlap_tolerance=1.5, between_chain_factor=0.2, bond_tolerance_factor=12.0, w_clash=1.0, w_bond=1.0, w_angle=1.0,
          k_restraint=0.0, eta0=0.01, rho=2.0, grow=1.2, shrink=0.5, max_iter=200, return_grad=False):
    """Violation relaxation of the movable residues of B structures of one complex (abx_relax; report columns:
    abx_amd.relax.RELAX_COLUMNS).  atom14 (B,Lp,14,3) f32 with Lab <= Lp <= L (rows beyond Lp are the ground truth's and never move; a
    batch-strided view is read in place), seq (B,>=Lab) int64 tokens; the complex as for design_scores, shared by the batch:
    gt_atom14 (L,14,3), gt_seq (L), gt_exists (L,14), chain_id (L), residx (L) or None; movable (L) bool / uint8 (rows >= Lp are ignored);
    mask (B,L,14) or None (None: the atoms of the residue types); res_mask (L) or None.  n_movable: the number of movable rows when
    the caller knows it (None: counted here, one host synchronisation).
    -> (atom14_relaxed (B,Lp,14,3) f32, report (B,11) float64[, generalised gradient (B,M,10) f32: g_t, torque, g_chi]).
    max_iter = 0 evaluates once and returns the input coordinates.  No host synchronisation when n_movable is given."""
    lib = _lib.load()
    dev = atom14.device
    L = chain_id.shape[-1]
    a = AbxRelaxArgs()
    B, Lp, _, own, keep = _structure_args(a, atom14, seq, L, Lab, gt_atom14, gt_seq, gt_exists, mask, res_mask, extra=(chain_id, movable))
    M = int(movable[:Lp].ne(0).sum()) if n_movable is None else int(n_movable)
    a.chain_id, a.movable = own(chain_id, torch.int32), own(movable, torch.uint8)
    if residx is not None:
        assert tuple(residx.shape) == (L,), residx.shape
        a.residx = own(residx, torch.int32)
    axis, group = chi_tables(dev)
    a.chi_axis, a.rigid_group = _p(axis), _p(group)
    a.overlap_tolerance, a.between_chain_factor, a.bond_tolerance_factor = float(overlap_tolerance), float(between_chain_factor), float(bond_tolerance_factor)
    a.w_clash, a.w_bond, a.w_angle = float(w_clash), float(w_bond), float(w_angle)
    a.k_restraint, a.eta0, a.rho, a.grow, a.shrink, a.max_iter = float(k_restraint), float(eta0), float(rho), float(grow), float(shrink), int(max_iter)
    out = torch.empty(B, Lp, 14, 3, device=dev)
    report = torch.empty(B, _lib.RELAX_COLS, dtype=torch.float64, device=dev)
    a.out_atom14, a.out_sb = _p(out), Lp * 42
    a.report, a.report_stride = _p(report), _lib.RELAX_COLS
    grad = None
    if return_grad:
        grad = torch.empty(B, max(M, 1), 10, device=dev)
        a.gen_grad = _p(grad)
    a.M = M
    ws = torch.empty(max(int(lib.abx_relax_workspace_bytes(B, L, M)), 8), dtype=torch.uint8, device=dev)
    check(lib.abx_relax(C.byref(a), _p(ws), _stream()), 'abx_relax')
    return (out, report, grad) if return_grad else (out, report)


def _check_sphere(sphere, dev):
    assert sphere.dtype == torch.float64 and sphere.dim() == 2 and sphere.shape[1] == 3 and sphere.is_contiguous() and sphere.device == dev, \
        'sphere: (P,3) float64 on the device of atom14'


def _workspace(workspace, need, dev):
    """The caller's workspace, checked, or (None) one of `need` bytes allocated here."""
    if workspace is None:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    assert workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == dev and workspace.numel() >= need, \
        f'workspace: at least {need} uint8 on the device of atom14'
    return workspace


def interface_scores(atom14, seq, gt_atom14, gt_seq, gt_exists, sphere, Lab=None, region=None, mask=None, res_mask=None, probe=1.4,
                     cutoff=4.0, out=None, points=None):
    """Interface analysis of B structures of one complex (abx_interface_scores; columns: abx_amd.interface.INTERFACE_COLUMNS): buried
    Shrake-Rupley surface, interface residues and antibody-antigen contacts between the rows < Lab and the rows >= Lab.
    atom14 (B,Lp,14,3) f32 with Lab <= Lp <= L (rows beyond Lp take the ground-truth coordinates; a batch-strided view is read in
    place), seq (B,>=Lab) int64 tokens; the complex, shared by the batch: gt_atom14 (L,14,3), gt_seq (L), gt_exists (L,14);
    sphere (P,3) float64 unit vectors on the device (abx_amd.interface.sphere_points); region (L) bool / uint8 or None;
    mask (B,L,14) or None (None: the atoms of the residue types); res_mask (L) or None.
    out: (B, 12) float64 with unit column stride and any row stride, or None; points: (B,L,14,2) int32 contiguous to receive
    acc_alone / acc_cplx of every slot, or None.  Three launches, no synchronisation."""
    lib = _lib.load()
    dev = atom14.device
    L = gt_seq.shape[-1]
    _check_sphere(sphere, dev)
    a = AbxInterfaceArgs()
    B, _, _, own, keep = _structure_args(a, atom14, seq, L, Lab, gt_atom14, gt_seq, gt_exists, mask, res_mask, region)
    a.sphere, a.P = _p(sphere), int(sphere.shape[0])
    a.probe, a.cutoff = float(probe), float(cutoff)
    out = _out_rows(a, out, B, _lib.IFACE_COLS, dev)
    _side_output(a, 'points', points, torch.int32, (B, L, 14, 2))
    ws = torch.empty(max(int(lib.abx_interface_scores_workspace_bytes(B, L, a.P)), 16), dtype=torch.uint8, device=dev)
    check(lib.abx_interface_scores(C.byref(a), _p(ws), _stream()), 'abx_interface_scores')
    return out


def polar_scores(atom14, seq, gt_atom14, gt_seq, gt_exists, table, Lab=None, region=None, mask=None, res_mask=None, points=None, n_points=128,
                 probe=1.4, hb_min=2.0, hb_max=3.5, hb_angle=90.0, salt=4.0, out=None, bonds=None, rows=None):
    """Polar contacts of B structures of one complex (abx_polar_scores; columns: abx_amd.polar.POLAR_COLUMNS): heavy-atom hydrogen bonds
    and salt bridges between the rows < Lab and the rows >= Lab, and the polar atoms buried by binding without a partner.
    atom14, seq, the complex, region, mask, res_mask as for interface_scores; table (21,14) int32 on the device (abx_amd.polar.
    polar_table); points (B,L,14,2) int32 contiguous, the acc_alone / acc_cplx that interface_scores returned for the SAME structures with
    n_points sphere points and `probe`, or None (columns 6-11 are -1).  hb_angle in degrees, [90, 180).
    out: (B, 14) float64 with unit column stride and any row stride, or None; bonds: (B,L,14,2) int32 contiguous to receive the same-side /
    cross-side bonds of every slot, or None; rows: (B,L,4) int32 contiguous to receive abx_amd.polar.ROW_COLUMNS of every row, or None.  One launch, no synchronisation."""
    from abx_amd.polar import cos2_of
    lib = _lib.load()
    dev = atom14.device
    L = gt_seq.shape[-1]
    assert table.dtype == torch.int32 and tuple(table.shape) == (21, 14) and table.is_contiguous() and table.device == dev, \
        'table: (21,14) int32 on the device of atom14'
    a = AbxPolarArgs()
    B, _, _, own, keep = _structure_args(a, atom14, seq, L, Lab, gt_atom14, gt_seq, gt_exists, mask, res_mask, region)
    a.table = _p(table)
    _side_output(a, 'points', points, torch.int32, (B, L, 14, 2))
    if points is not None:
        a.P, a.probe = int(n_points), float(probe)
    a.hb_min, a.hb_max, a.hb_angle, a.hb_cos2, a.salt = float(hb_min), float(hb_max), float(hb_angle), cos2_of(hb_angle), float(salt)
    out = _out_rows(a, out, B, _lib.POLAR_COLS, dev)
    _side_output(a, 'bonds', bonds, torch.int32, (B, L, 14, 2))
    _side_output(a, 'rows', rows, torch.int32, (B, L, 4))
    check(lib.abx_polar_scores(C.byref(a), None, _stream()), 'abx_polar_scores')
    return out


def developability_scores(atom14, seq, gt_atom14, gt_seq, gt_exists, chain_id, cdr_def, tables, points, Lab=None, residx=None, region=None,
                          mask=None, res_mask=None, n_points=128, q_max=None, radius=10.0, exposed=0.075, out=None, rows=None, j_chunk=0):
    """Developability of B structures of one complex (abx_developability_scores; columns: abx_amd.developability.DEVELOPABILITY_COLUMNS):
    spatial aggregation propensity, chain charges and sequence liabilities of the free antibody, the rows < Lab.
    atom14, seq, the complex, region, mask, res_mask as for interface_scores; chain_id, cdr_def (L) int32, residx (L) int32 or None as for
    design_scores; tables = (q (21,14) int64, a (21,14) float64, ref (21) float64) on the device (abx_amd.developability.weight_table for
    n_points and the probe of the surface); q_max: the largest |q| (None: read from q, one host synchronisation); points (B,L,14,2) int32
    contiguous, the acc_alone / acc_cplx that interface_scores returned for the SAME structures with n_points sphere points.
    radius: of the SAP sphere (Angstrom); exposed: smallest relative side-chain area of an exposed residue; j_chunk: weighted atoms per LDS
    chunk (0: the kernel's default).
    out: (B, 21) float64 with unit column stride and any row stride, or None; rows: (B,L,4) float64 contiguous to receive
    abx_amd.developability.ROW_COLUMNS of every row, or None.  Three launches, no synchronisation."""
    lib = _lib.load()
    dev = atom14.device
    L = gt_seq.shape[-1]
    q, ar, ref = tables
    assert q.dtype == torch.int64 and tuple(q.shape) == (21, 14) and ar.dtype == torch.float64 and tuple(ar.shape) == (21, 14) and \
        ref.dtype == torch.float64 and tuple(ref.shape) == (21,) and all(t.is_contiguous() and t.device == dev for t in tables), \
        'tables: q (21,14) int64, a (21,14) float64, ref (21) float64 on the device of atom14'
    a = AbxDevelopabilityArgs()
    B, _, _, own, keep = _structure_args(a, atom14, seq, L, Lab, gt_atom14, gt_seq, gt_exists, mask, res_mask, region, extra=(chain_id, cdr_def))
    a.chain_id, a.cdr_def = own(chain_id, torch.int32), own(cdr_def, torch.int32)
    if residx is not None:
        assert tuple(residx.shape) == (L,), residx.shape
        a.residx = own(residx, torch.int32)
    a.q, a.a, a.ref = _p(q), _p(ar), _p(ref)
    a.q_max = int(q.abs().max()) if q_max is None else int(q_max)
    assert points is not None, 'points: the (B,L,14,2) int32 counts of interface_scores'
    _side_output(a, 'points', points, torch.int32, (B, L, 14, 2))
    a.P, a.radius2, a.exposed, a.j_chunk = int(n_points), float(radius) * float(radius), float(exposed), int(j_chunk)
    out = _out_rows(a, out, B, _lib.DEV_COLS, dev)
    _side_output(a, 'rows', rows, torch.float64, (B, L, 4))
    ws = torch.empty(max(int(lib.abx_developability_scores_workspace_bytes(B, L)), 16), dtype=torch.uint8, device=dev)
    check(lib.abx_developability_scores(C.byref(a), _p(ws), _stream()), 'abx_developability_scores')
    return out


def shape_workspace_bytes(B, L, P, max_dots):
    """Bytes of the workspace of shape_scores (abx_shape_scores_workspace_bytes)."""
    return int(_lib.load().abx_shape_scores_workspace_bytes(int(B), int(L), int(P), int(max_dots)))


def shape_scores(atom14, seq, gt_atom14, gt_seq, gt_exists, sphere, points, Lab=None, region=None, mask=None, res_mask=None, probe=1.4,
                 trim=1.5, weight=0.5, max_dots=8192, out=None, j_chunk=0, workspace=None):
    """Shape complementarity of B structures of one complex (abx_shape_scores; columns: abx_amd.shape.SHAPE_COLUMNS): the Sc statistic of
    Lawrence & Colman between the rows < Lab and the rows >= Lab on the contact surface of both partners.
    atom14, seq, the complex, sphere, region, mask, res_mask, probe as for interface_scores; points (B,L,14,2) int32 contiguous, the
    acc_alone / acc_cplx that interface_scores returned for the SAME structures with this sphere and probe.  trim: width of the peripheral
    band (Angstrom); weight: of the squared distance in the exponent; max_dots: capacity of each dot list of a structure (a structure
    beyond it, or one whose dots disagree with `points`, gets a row of -1); j_chunk: dots per LDS chunk of the match (0: the default).
    out: (B, 11) float64 with unit column stride and any row stride, or None; workspace: a uint8 tensor of at least
    shape_workspace_bytes(B, L, P, max_dots) bytes, or None (allocated here).  Five launches, no synchronisation."""
    lib = _lib.load()
    dev = atom14.device
    L = gt_seq.shape[-1]
    _check_sphere(sphere, dev)
    a = AbxShapeArgs()
    B, _, _, own, keep = _structure_args(a, atom14, seq, L, Lab, gt_atom14, gt_seq, gt_exists, mask, res_mask, region)
    a.sphere, a.P = _p(sphere), int(sphere.shape[0])
    assert points is not None, 'points: the (B,L,14,2) int32 counts of interface_scores'
    _side_output(a, 'points', points, torch.int32, (B, L, 14, 2))
    a.probe, a.trim, a.weight, a.max_dots, a.j_chunk = float(probe), float(trim), float(weight), int(max_dots), int(j_chunk)
    out = _out_rows(a, out, B, _lib.SHAPE_COLS, dev)
    need = int(lib.abx_shape_scores_workspace_bytes(B, L, a.P, a.max_dots))
    workspace = _workspace(workspace, need, dev)
    check(lib.abx_shape_scores(C.byref(a), _p(workspace), _stream()), 'abx_shape_scores')
    return out


def patch_workspace_bytes(B, L, Lab):
    """Bytes of the workspace of patch_scores (abx_patch_scores_workspace_bytes)."""
    return int(_lib.load().abx_patch_scores_workspace_bytes(int(B), int(L), int(Lab)))


def patch_scores(atom14, seq, gt_atom14, gt_seq, gt_exists, chain_id, cdr_def, tables, points, Lab=None, region=None, mask=None,
                 res_mask=None, cutoff=7.5, vicinity=4.0, salt=3.2, exposed=0.075, h_max=None, q_max=None, gly=7, out=None, rows=None,
                 workspace=None):
    """Surface patches of B structures of one complex (abx_patch_scores; columns: abx_amd.patches.PATCHES_COLUMNS): patches of surface
    hydrophobicity and of positive / negative charge around the CDRs of the free antibody, its charge symmetry, and the charge pairing
    across the interface.
    atom14, seq, the complex, region, mask, res_mask as for interface_scores; chain_id, cdr_def (L) int32 as for design_scores; tables =
    (h (21) float64, q10 (21) int32, a (21,14) float64, ref (21) float64, roles (21,14) int32) on the device (abx_amd.patches.
    kyte_doolittle / charge_table, abx_amd.developability.weight_table for the surface's points and probe, abx_amd.polar.polar_table);
    h_max / q_max: the largest |h| / |q10| (None: read from the tables, one host synchronisation each); gly: the residue type whose h a
    salt-bridged row takes; points (B,L,14,2) int32 contiguous, the acc_alone / acc_cplx that interface_scores returned for the SAME
    structures.  cutoff, vicinity, salt: closest heavy-atom distances (Angstrom); exposed: smallest relative side-chain area of an
    exposed residue.
    out: (B, 18) float64 with unit column stride and any row stride, or None; rows: (B,L,4) float64 contiguous to receive
    abx_amd.patches.ROW_COLUMNS of every row, or None; workspace: a uint8 tensor of at least patch_workspace_bytes(B, L, Lab) bytes, or
    None (allocated here).  Three launches, no synchronisation."""
    lib = _lib.load()
    dev = atom14.device
    L = gt_seq.shape[-1]
    h, q10, ar, ref, roles = tables
    assert h.dtype == torch.float64 and tuple(h.shape) == (21,) and q10.dtype == torch.int32 and tuple(q10.shape) == (21,) and \
        ar.dtype == torch.float64 and tuple(ar.shape) == (21, 14) and ref.dtype == torch.float64 and tuple(ref.shape) == (21,) and \
        roles.dtype == torch.int32 and tuple(roles.shape) == (21, 14) and all(t.is_contiguous() and t.device == dev for t in tables), \
        'tables: h (21) float64, q10 (21) int32, a (21,14) float64, ref (21) float64, roles (21,14) int32 on the device of atom14'
    a = AbxPatchArgs()
    B, _, Lab, own, keep = _structure_args(a, atom14, seq, L, Lab, gt_atom14, gt_seq, gt_exists, mask, res_mask, region, extra=(chain_id, cdr_def))
    a.chain_id, a.cdr_def = own(chain_id, torch.int32), own(cdr_def, torch.int32)
    a.h, a.q10, a.a, a.ref, a.table = _p(h), _p(q10), _p(ar), _p(ref), _p(roles)
    a.h_max = float(h.abs().max()) if h_max is None else float(h_max)
    a.q_max = int(q10.abs().max()) if q_max is None else int(q_max)
    assert points is not None, 'points: the (B,L,14,2) int32 counts of interface_scores'
    _side_output(a, 'points', points, torch.int32, (B, L, 14, 2))
    a.cutoff2, a.vicinity2, a.salt2 = float(cutoff) * float(cutoff), float(vicinity) * float(vicinity), float(salt) * float(salt)
    a.exposed, a.gly = float(exposed), int(gly)
    out = _out_rows(a, out, B, _lib.PATCH_COLS, dev)
    _side_output(a, 'rows', rows, torch.float64, (B, L, 4))
    need = int(lib.abx_patch_scores_workspace_bytes(B, L, Lab))
    workspace = _workspace(workspace, need, dev)
    check(lib.abx_patch_scores(C.byref(a), _p(workspace), _stream()), 'abx_patch_scores')
    return out


def torsion_workspace_bytes(B, Lab):
    """Bytes of the workspace of torsion_scores (abx_torsion_scores_workspace_bytes)."""
    return int(_lib.load().abx_torsion_scores_workspace_bytes(int(B), int(Lab)))


def torsion_scores(atom14, seq, gt_atom14, gt_seq, gt_exists, chain_id, residx, tables, thresholds, Lab=None, region=None, mask=None,
                   res_mask=None, gly=7, pro=14, out=None, rows=None, classes=None, workspace=None):
    """Torsion analysis of B structures of one complex (abx_torsion_scores; columns: abx_amd.torsions.TORSIONS_COLUMNS): cis and twisted
    peptides, phi >= 0, the ABEGO classes, the backbone dihedrals and the chi angles against the crystal structure.
    atom14, seq, the complex, region, mask, res_mask as for accuracy_scores (only the rows < Lab are read); chain_id (L) and residx (L)
    or None as for design_scores; tables = (chi_atoms (21,4,4) int32, chi_pi (21,4) uint8) on the device (abx_amd.torsions.chi_table);
    thresholds: {name: (cos, sin)} of abx_amd.torsions.thresholds; gly / pro: the residue types of phi_pos / cis_nonpro.
    out: (B, 25) float64 with unit column stride and any row stride, or None; rows (B,Lab,8) float64 and classes (B,Lab) int32:
    contiguous tensors to receive the optional outputs, or None; workspace: a uint8 tensor of at least torsion_workspace_bytes(B, Lab)
    bytes, or None (allocated here).  One launch, no synchronisation."""
    lib = _lib.load()
    dev = atom14.device
    L = gt_seq.shape[-1]
    chi_atoms, chi_pi = tables
    assert chi_atoms.dtype == torch.int32 and tuple(chi_atoms.shape) == (21, 4, 4) and chi_pi.dtype == torch.uint8 and tuple(chi_pi.shape) == (21, 4) and \
        all(t.is_contiguous() and t.device == dev for t in tables), 'tables: chi_atoms (21,4,4) int32, chi_pi (21,4) uint8 on the device of atom14'
    a = AbxTorsionArgs()
    B, _, Lab, own, keep = _structure_args(a, atom14, seq, L, Lab, gt_atom14, gt_seq, gt_exists, mask, res_mask, region,
                                           extra=(chain_id,) + ((residx,) if residx is not None else ()))
    a.chain_id = own(chain_id, torch.int32)
    if residx is not None:
        a.residx = own(residx, torch.int32)
    a.chi_atoms, a.chi_pi = _p(chi_atoms), _p(chi_pi)
    for name in ('cis', 'trans', 'o', 'a_mid', 'a_half', 'g_half', 'chi_tol'):
        pair = getattr(a, name)
        pair[0], pair[1] = float(thresholds[name][0]), float(thresholds[name][1])
    a.gly, a.pro = int(gly), int(pro)
    out = _out_rows(a, out, B, _lib.TORSION_COLS, dev)
    _side_output(a, 'rows', rows, torch.float64, (B, Lab, 8))
    _side_output(a, 'classes', classes, torch.int32, (B, Lab))
    need = int(lib.abx_torsion_scores_workspace_bytes(B, Lab))
    workspace = _workspace(workspace, need, dev)
    check(lib.abx_torsion_scores(C.byref(a), _p(workspace), _stream()), 'abx_torsion_scores')
    return out


def secondary_workspace_bytes(B, Lab):
    """Bytes of the workspace of secondary_scores (abx_secondary_scores_workspace_bytes)."""
    return int(_lib.load().abx_secondary_scores_workspace_bytes(int(B), int(Lab)))


def secondary_scores(atom14, seq, gt_atom14, gt_seq, gt_exists, chain_id, residx, thresholds, Lab=None, region=None, mask=None, res_mask=None,
                     pro=14, out=None, rows=None, classes=None, workspace=None):
    """Secondary structure of B structures of one complex (abx_secondary_scores; columns: abx_amd.secondary.SECONDARY_COLUMNS): DSSP's
    backbone hydrogen bonds on a virtual H, turns, helices, bridges, ladders and bends over the antibody rows, against the crystal structure.
    atom14, seq, the complex, region, mask, res_mask as for accuracy_scores (only the rows < Lab are read); chain_id (L) and residx (L)
    or None as for design_scores; thresholds: dict(hb_energy, bend = (cos, sin)) of abx_amd.secondary.thresholds; pro: the residue type
    without an H.
    out: (B, 22) float64 with unit column stride and any row stride, or None; rows (B,Lab,6) int32 and classes (B,Lab) int32: contiguous
    tensors to receive the optional outputs, or None; workspace: a uint8 tensor of at least secondary_workspace_bytes(B, Lab) bytes, or
    None (allocated here).  One launch, no synchronisation."""
    lib = _lib.load()
    dev = atom14.device
    L = gt_seq.shape[-1]
    a = AbxSecondaryArgs()
    B, _, Lab, own, keep = _structure_args(a, atom14, seq, L, Lab, gt_atom14, gt_seq, gt_exists, mask, res_mask, region,
                                           extra=(chain_id,) + ((residx,) if residx is not None else ()))
    a.chain_id = own(chain_id, torch.int32)
    if residx is not None:
        a.residx = own(residx, torch.int32)
    a.hb_energy = float(thresholds['hb_energy'])
    a.bend[0], a.bend[1] = float(thresholds['bend'][0]), float(thresholds['bend'][1])
    a.pro = int(pro)
    out = _out_rows(a, out, B, _lib.SECONDARY_COLS, dev)
    _side_output(a, 'rows', rows, torch.int32, (B, Lab, 6))
    _side_output(a, 'classes', classes, torch.int32, (B, Lab))
    need = int(lib.abx_secondary_scores_workspace_bytes(B, Lab))
    workspace = _workspace(workspace, need, dev)
    check(lib.abx_secondary_scores(C.byref(a), _p(workspace), _stream()), 'abx_secondary_scores')
    return out


def accuracy_scores(atom14, seq, gt_atom14, gt_seq, gt_exists, Lab=None, region=None, mask=None, res_mask=None, plddt=None, radius=15.0,
                    contact=5.0, out=None, rows=None, counts=None, contacts=None):
    """Accuracy of B designs of one complex against its crystal structure (abx_accuracy_scores; columns: abx_amd.accuracy.
    ACCURACY_COLUMNS): all-atom / backbone / C-alpha lDDT, the pLDDT calibration, TM-score / GDT / RMSD of the C-alpha and the native
    antibody-antigen residue contacts that survive.
    atom14 (B,Lp,14,3) f32 with Lp = Lab or L (rows beyond Lp take the ground-truth coordinates; a batch-strided view is read in
    place), seq (B,>=Lab) int64 tokens; the complex, shared by the batch: gt_atom14 (L,14,3), gt_seq (L), gt_exists (L,14);
    region (L) bool / uint8 or None; mask (B,L,14) or None (None: the atoms of the residue types); res_mask (L) or None;
    plddt (B,L) f32 per-residue pLDDT of the call that produced the designs, or None.
    out: (B, 21) float64 with unit column stride and any row stride, or None; rows (B,L,4) float64, counts (B,L,3,5) int32, contacts
    (B,Lab,L-Lab) uint8: contiguous tensors to receive the optional outputs, or None.  Two launches, no synchronisation."""
    lib = _lib.load()
    dev = atom14.device
    L = gt_seq.shape[-1]
    a = AbxAccuracyArgs()
    B, _, Lab, own, keep = _structure_args(a, atom14, seq, L, Lab, gt_atom14, gt_seq, gt_exists, mask, res_mask, region)
    if plddt is not None:
        assert tuple(plddt.shape) == (B, L), plddt.shape
        a.plddt, a.plddt_sb = own(plddt, torch.float32), L
    a.lddt_radius, a.contact = float(radius), float(contact)
    out = _out_rows(a, out, B, _lib.ACC_COLS, dev)
    _side_output(a, 'rows', rows, torch.float64, (B, L, 4))
    _side_output(a, 'counts', counts, torch.int32, (B, L, 3, 5))
    _side_output(a, 'contacts', contacts, torch.uint8, (B, Lab, L - Lab))
    ws = torch.empty(max(int(lib.abx_accuracy_scores_workspace_bytes(B, L)), 16), dtype=torch.uint8, device=dev)
    check(lib.abx_accuracy_scores(C.byref(a), _p(ws), _stream()), 'abx_accuracy_scores')
    return out


def ensemble_pairs(atom14, seq, region, atoms=4, n_region=None, out=None):
    """All pairs of N structures of one complex (abx_ensemble_pairs): (3, N, N) float64 planes rmsd_fit (after the optimal proper
    rotation), rmsd_frame (no superposition) and seq_diff (differing region residues) over the set rows of `region`.
    atom14 (N,Lp,14,3) f32 (a batch-strided view is read in place), seq (N,>=Lp) int64 tokens, region (>=Lp) bool / uint8 on the
    device, atoms 1 (C-alpha) or 4 (N, CA, C, O).  n_region: the number of set rows below Lp (None: counted here, one host
    synchronisation; abx_amd.ensemble.EnsembleAnalyzer counts once per complex).  out: (3,N,N) float64 contiguous, or None.
    One launch, no synchronisation."""
    lib = _lib.load()
    dev = atom14.device
    N, Lp = atom14.shape[0], atom14.shape[1]
    assert tuple(atom14.shape[2:]) == (14, 3) and seq.shape[0] == N and seq.shape[1] >= Lp, (atom14.shape, seq.shape)
    assert region.dim() == 1 and region.shape[0] >= Lp, region.shape
    x = _f32(atom14)
    if not x[0].is_contiguous():
        x = x.contiguous()
    sq = seq if (seq.dtype == torch.int64 and seq.stride(1) == 1) else seq.to(torch.int64).contiguous()
    rg = region if (region.dtype == torch.uint8 and region.is_contiguous()) else region.ne(0).to(torch.uint8).contiguous()
    M = int(rg[:Lp].ne(0).sum()) if n_region is None else int(n_region)
    if out is None:
        out = torch.empty(3, N, N, dtype=torch.float64, device=dev)
    assert out.dtype == torch.float64 and tuple(out.shape) == (3, N, N) and out.is_contiguous() and out.is_cuda, 'out: (3,N,N) float64'
    a = AbxEnsemblePairsArgs()
    a.pred_atom14, a.pred_sb, a.Lpred = _p(x), x.stride(0) if N > 1 else Lp * 42, Lp
    a.pred_seq, a.pred_seq_sb = _p(sq), sq.stride(0) if N > 1 else sq.shape[1]
    a.region, a.atoms, a.M = _p(rg), int(atoms), M
    a.planes, a.plane_stride, a.N = _p(out), N * N, N
    check(lib.abx_ensemble_pairs(C.byref(a), None, _stream()), 'abx_ensemble_pairs')
    return out


def ensemble_cluster(planes, metric=0, cutoff=1.0, out=None):
    """Daura / GROMOS clusters on plane `metric` (0 rmsd_fit, 1 rmsd_frame) of the (3,N,N) float64 planes of ensemble_pairs and one row
    of abx_amd.ensemble.ENSEMBLE_COLUMNS per design (abx_ensemble_cluster).  -> (table (N,10) float64, centres (N) int32 padded with
    -1, n_clusters (1) int32), all on the device.  out: (N,10) float64 rows with unit column stride and any row stride, or None.
    One launch, no synchronisation."""
    lib = _lib.load()
    dev = planes.device
    N = planes.shape[1]
    assert planes.dtype == torch.float64 and tuple(planes.shape) == (3, N, N) and planes.is_contiguous() and planes.is_cuda, 'planes: (3,N,N) float64'
    if out is None:
        out = torch.empty(N, _lib.ENS_COLS, dtype=torch.float64, device=dev)
    assert out.dtype == torch.float64 and tuple(out.shape) == (N, _lib.ENS_COLS) and out.stride(1) == 1 and out.is_cuda, 'out: (N, 10) float64 rows'
    centres = torch.empty(N, dtype=torch.int32, device=dev)
    n_clusters = torch.empty(1, dtype=torch.int32, device=dev)
    a = AbxEnsembleClusterArgs()
    a.planes, a.plane_stride, a.metric, a.cutoff = _p(planes), N * N, int(metric), float(cutoff)
    a.out, a.out_stride = _p(out), out.stride(0) if N > 1 else _lib.ENS_COLS
    a.centres, a.n_clusters, a.N = _p(centres), _p(n_clusters), N
    check(lib.abx_ensemble_cluster(C.byref(a), _stream()), 'abx_ensemble_cluster')
    return out, centres, n_clusters


def distogram_pack_weight(weight):
    """impl.distogram.proj.weight (64, 192) -> the MFMA B-fragment image abx_distogram_* read (include/abx_hip.h, AbxDistogramArgs.W):
    out[k // 4][n // 16][k % 4][n % 16] = weight[n][k], (12288,) fp32 contiguous on the weight's device.  Packed once per scorer."""
    N, K = _lib.DISTO_BINS, _lib.DISTO_CHANNELS
    assert tuple(weight.shape) == (N, K), weight.shape
    return weight.detach().to(torch.float32).t().reshape(K // 4, 4, N // 16, 16).permute(0, 2, 1, 3).contiguous().reshape(-1)


def _distogram_common(a, z, w_packed, bias, keep):
    B, L = z.shape[0], z.shape[1]
    assert z.dim() == 4 and z.shape[2] == L and z.shape[3] == _lib.DISTO_CHANNELS, z.shape
    z = _f32(z)
    if not z.is_contiguous():
        z = z.contiguous()
    assert w_packed.dtype == torch.float32 and w_packed.numel() == _lib.DISTO_BINS * _lib.DISTO_CHANNELS and w_packed.is_contiguous(), \
        'w_packed: ops.distogram_pack_weight(weight)'
    bias = bias.detach().to(torch.float32).contiguous()
    assert bias.numel() == _lib.DISTO_BINS, bias.shape
    keep += [z, bias]
    a.z, a.W, a.bias, a.B, a.L = _p(z), _p(w_packed), _p(bias), B, L
    return B, L


def distogram_scores(z, w_packed, bias, breaks, sq_breaks, pb, classes, valid, cutoff=8.0, table=None, rows=True, planes=False):
    """Confidence of B designs from the distogram head (abx_distogram_scores; columns: abx_amd.confidence.CONFIDENCE_COLUMNS).
    z (B,L,L,192) f32 pair representation, w_packed = distogram_pack_weight(weight), bias (64), breaks / sq_breaks (63) f32,
    pb (B,L,3) f32 pseudo-beta coordinates, classes (L) uint8 class bits, valid (B,L) bool / uint8, all on z's device.
    -> (table (B,10) float64, rows (B,L,4) float64 or None, (p_contact, exp_dist) (B,L,L) f32 or None).  table: rows to write into
    (unit column stride, any row stride) or None.  Two launches, no synchronisation; the logits never exist in memory."""
    lib = _lib.load()
    dev = z.device
    keep = []
    a = AbxDistogramArgs()
    B, L = _distogram_common(a, z, w_packed, bias, keep)

    def own(t, dtype, shape):
        assert tuple(t.shape) == shape, (tuple(t.shape), shape)
        t = t.to(dtype).contiguous()
        keep.append(t)
        return _p(t)

    nb = _lib.DISTO_BINS - 1
    a.breaks, a.sq_breaks, a.num_breaks = own(breaks, torch.float32, (nb,)), own(sq_breaks, torch.float32, (nb,)), nb
    a.pb = own(pb, torch.float32, (B, L, 3))
    a.classes, a.valid = own(classes, torch.uint8, (L,)), own(valid.ne(0), torch.uint8, (B, L))
    a.cutoff = float(cutoff)
    if table is None:
        table = torch.empty(B, _lib.DISTO_COLS, dtype=torch.float64, device=dev)
    assert table.dtype == torch.float64 and tuple(table.shape) == (B, _lib.DISTO_COLS) and table.stride(1) == 1 and table.is_cuda, \
        'table: (B, 10) float64 rows'
    a.table, a.table_stride = _p(table), table.stride(0) if B > 1 else _lib.DISTO_COLS
    rows_t = torch.empty(B, L, 4, dtype=torch.float64, device=dev) if rows else None
    a.rows = _p(rows_t)
    pl = None
    if planes:
        pl = (torch.empty(B, L, L, device=dev), torch.empty(B, L, L, device=dev))
        a.p_contact, a.exp_dist = _p(pl[0]), _p(pl[1])
    ws = torch.empty(B, L, _lib.DISTO_ROWSUMS, dtype=torch.float64, device=dev)
    a.rowsums = _p(ws)
    check(lib.abx_distogram_scores(C.byref(a), _stream()), 'abx_distogram_scores')
    return table, rows_t, pl


def distogram_logits(z, w_packed, bias):
    """The reference's heads['distogram']['logits'] (head.py:39-44) of n designs: z (n,L,L,192) f32 -> (n,L,L,64) f32, by the kernel
    body whose values distogram_scores reduces (abx_distogram_logits: the same bits).  One launch, no synchronisation."""
    lib = _lib.load()
    keep = []
    a = AbxDistogramArgs()
    B, L = _distogram_common(a, z, w_packed, bias, keep)
    out = torch.empty(B, L, L, _lib.DISTO_BINS, device=z.device)
    check(lib.abx_distogram_logits(C.byref(a), _p(out), _stream()), 'abx_distogram_logits')
    return out
