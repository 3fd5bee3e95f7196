"""Kernel names come from the library's own dispatch (abx_gemm_plan / abx_tri_attn_plan / abx_seq_attn_plan: the dispatchers of csrc/gemm.hip,
gemm3.hip, gemm_as.hip and attention.hip run up to the launch and name the kernel there).  Descriptors on placeholder addresses, literal names; no GPU.
Run as a script with a case name, this file prints that case's name: the environment-switch tests start it as a fresh child process,
because the library reads its switches once."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
P = 1 << 40                                         # placeholder "device addresses": 16-byte aligned, 1 TiB apart, never dereferenced
ROWS = 1024 * 64                                    # 1 024 blocks of 64 rows: where the A-stationary walk starts to pay


def _ln_gemm(M, N, K=192, a=1 * P):
    """LayerNorm-folded weight GEMM on split-f16 planes: fp32 rows (M, K), planes [K/16][2][N][16], plain fp32 store."""
    from abx_amd._lib import AbxGemm
    g = AbxGemm()
    g.M, g.N, g.K, g.batch, g.alpha, g.exact = M, N, K, 1, 1.0, 2
    g.A, g.sAm, g.sAk = a, K, 1
    g.B, g.sBk, g.sBn = 2 * P, N, 1
    g.B_split, g.sB3n, g.sB3p, g.sB3k, g.b_f16 = 3 * P, 16, 16 * N, 32 * N, 1
    g.C, g.sCm = 4 * P, N
    g.ln_csum, g.bias, g.ln_eps = 5 * P, 6 * P, 1e-5
    return g


def _side(M, N=4, K=192):
    """The skinny transposed-store projection over the same rows (the pair bias next to q | k | v)."""
    s = _ln_gemm(M, N, K)
    s.B, s.B_split, s.C, s.ln_csum, s.bias = 7 * P, 8 * P, 9 * P, 10 * P, 11 * P
    s.c_transposed, s.sCm = 1, M
    return s


def _glu(L=256):
    """The tri-mul projection: glu column pairs, unpadded pair rows in through the pair-row map, operand images out in (8 i x 16 k) blocks."""
    g = _ln_gemm(L * L, 512)
    g.glu, g.c_transposed, g.C = 1, 1, None
    g.pair_L, g.pair_Lp, g.a_pair = L, L, 1
    g.C_split, g.c_split_L, g.c_split_nA, g.c_split_tile = 4 * P, L, 128, 1
    g.sCp, g.sCk, g.sCm = 16 * L, 32 * L, (L // 16) * 32 * L
    return g


def _plan(main, side=None):
    from abx_amd import _lib
    buf = ctypes.create_string_buffer(128)
    rc = _lib.load().abx_gemm_plan(ctypes.byref(main), None if side is None else ctypes.byref(side), buf, len(buf))
    return rc, buf.value.decode()


TILE = 'gemm3_kernel<128, 128, 32, 128, 0, false, 4>'


def test_a_stationary_kernel_routes():
    from abx_amd import ops
    assert ops.gemm_as_kernel_name(_ln_gemm(ROWS, 768)) == 'gemm_as_kernel<0, false, 0, false>'
    assert _plan(_ln_gemm(ROWS, 768)) == (0, 'gemm_as_kernel<0, false, 0, false>')
    assert ops.gemm_as_kernel_name(_ln_gemm(ROWS, 576), _side(ROWS)) == 'gemm_as_kernel<0, true, 0, false>'
    g = _ln_gemm(ROWS, 576)
    g.c_planes_from, g.c_planes_group = 192, 48
    assert ops.gemm_as_kernel_name(g, _side(ROWS)) == 'gemm_as_kernel<0, true, 0, true>'
    assert ops.gemm_as_kernel_name(_glu()) == 'gemm_as_kernel<1, false, 0, false>'
    # one block of 64 rows short of the launch-size rule: the tile kernel
    assert ops.gemm_as_kernel_name(_ln_gemm(1023 * 64, 768)) is None and _plan(_ln_gemm(1023 * 64, 768)) == (0, TILE)
    # rows that are not 16-byte aligned: neither split-f16 kernel takes them, the exact fp32 kernel does
    g = _ln_gemm(ROWS, 768, a=P + 4)
    assert ops.gemm_as_kernel_name(g) is None and _plan(g) == (0, 'gemm_kernel<128, 192, 64, 96, 16, true, true, false, 2>')


def test_pairs():
    from abx_amd import ops
    # N % 128 == 0: no ragged last tile for the side to ride in, the tile side kernel serves the pair
    assert _plan(_ln_gemm(ROWS, 768), _side(ROWS)) == (0, 'gemm3_side_kernel')
    assert ops.gemm_as_kernel_name(_ln_gemm(ROWS, 768), _side(ROWS)) is None
    # N = 192: below the A-stationary kernel's two N-tiles and no multiple of 128: two launches, named after the main one
    assert _plan(_ln_gemm(ROWS, 192), _side(ROWS)) == (0, 'gemm3_kernel<128, 192, 32, 192, 0, false, 3>')
    assert _plan(_ln_gemm(ROWS, 192)) == (0, 'gemm3_kernel<128, 192, 32, 192, 0, false, 3>')


def test_triangle_attention():
    from abx_amd import ops
    assert ops.tri_attn_kernel_name(352, exact=False, rowfused=False) == 'tri_attn8_kernel<192, 768, true>'
    assert ops.tri_attn_kernel_name(231, exact=False, rowfused=False) == 'tri_attn8_kernel<128, 768, true>'
    assert ops.tri_attn_kernel_name(97, exact=False, rowfused=False) == 'tri_attn8_kernel<128, 768, true>'
    assert ops.tri_attn_kernel_name(352, exact=True) == 'tri_attn_kernel'
    assert ops.tri_attn_kernel_name(352, exact=False, rowfused=True) == 'tri_attn8_rowfused_kernel'


def test_sequence_attention():
    import pytest
    from abx_amd import ops, _lib
    # keys per lane 2, 4, 6, 8, 12 by ceil(L / 64), on 1024, 1024, 1024, 512, 256 threads; both sides of every threshold
    for L, name in ((1, '2, 1024'), (128, '2, 1024'), (129, '4, 1024'), (256, '4, 1024'), (257, '6, 1024'), (352, '6, 1024'), (384, '6, 1024'),
                    (385, '8, 512'), (512, '8, 512'), (513, '12, 256'), (716, '12, 256')):
        assert ops.seq_attn_kernel_name(L) == f'seq_attn2_kernel<{name}>', L
    # the queries of a (sample, head) go to one workgroup up to L = 512, to ceil(L / 512) beyond; rows per workgroup rounded up to 4
    assert [ops.seq_attn_kernel_name(L, with_qblk=True)[1] for L in (1, 5, 352, 512, 513, 716)] == [4, 8, 352, 512, 260, 360]
    # a refused length: the code and message of the entry point, no name
    lib = _lib.load()
    for L in (717, 768, 800, 0):
        buf, qblk = ctypes.create_string_buffer(64), ctypes.c_int(-1)
        assert lib.abx_seq_attn_plan(L, buf, len(buf), ctypes.byref(qblk)) < 0 and buf.value == b'' and qblk.value == -1
        assert (b'L <= 716' if L else b'bad args') in lib.abx_last_error_string()
        with pytest.raises(_lib.AbxHipError):
            ops.seq_attn_kernel_name(L)
    assert lib.abx_seq_attn_plan(64, None, 0, None) < 0 and b'abx_seq_attn_plan' in lib.abx_last_error_string()
    buf = ctypes.create_string_buffer(64)
    assert lib.abx_seq_attn_plan(64, buf, len(buf), None) == 0 and buf.value == b'seq_attn2_kernel<2, 1024>'


def test_rejected_descriptor_returns_the_code_of_the_mode_check():
    from abx_amd import _lib
    lib = _lib.load()
    g = _ln_gemm(ROWS, 768)
    g.out_ln_w, g.out_ln_b, g.A2, g.B2_split, g.ln2_csum = 12 * P, 13 * P, 14 * P, 15 * P, 16 * P      # out_ln and dual: exclusive
    rc = lib.abx_gemm_check_modes(ctypes.byref(g))
    assert rc < 0 and b'mutually exclusive' in lib.abx_last_error_string()
    assert _plan(g) == (rc, '') and b'mutually exclusive' in lib.abx_last_error_string()


def _child(case, switch, value='1'):
    """The name of `case` in a fresh process that has `switch` set to `value` and nothing else changed."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), case], env=dict(os.environ, **{switch: value}), capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.strip().splitlines()[-1]


def test_abx_no_gemm_as_switches_the_name_too():
    from abx_amd import ops
    assert ops.gemm_as_kernel_name(_ln_gemm(ROWS, 768)) == 'gemm_as_kernel<0, false, 0, false>'
    assert _child('as_plain', 'ABX_NO_GEMM_AS') == 'None'


def test_abx_no_gemm_as_set_to_0_is_off():
    """One rule for the on / off switches (abx_env_on): set, not empty and not "0"."""
    assert _child('as_plain', 'ABX_NO_GEMM_AS', '0') == 'gemm_as_kernel<0, false, 0, false>'


def test_abx_no_dual_as_switches_the_name_too():
    from abx_amd import ops
    assert ops.gemm_kernel_name(352 * 352, 192, 128, 100, a_kcontig=False, split=True, exact=2, dual=True) == 'gemm_as_dual_kernel'
    assert _child('dual', 'ABX_NO_DUAL_AS') == 'gemm3_dual_kernel<128, 96, 32, 96, 3>'


# ---- AbxGemm.tune: the guard of gemm_prepare (ABX_TUNE_LIVE_MASK) ---------------------------------------------------------------------
RETIRED_OR_UNKNOWN = (2, 4, 6, 8, 14, 16, 32, 256, 512, 1024, 1536, 32768, 4096, 8192, 1 << 16, 1 << 30)


def _refused(main, side=None):
    from abx_amd import _lib
    rc, name = _plan(main, side)
    msg = _lib.load().abx_last_error_string()
    return rc < 0 and name == '' and b'tune' in msg, (rc, name, msg)


def _tune_cases():
    import pytest
    return pytest.mark.parametrize('tune', RETIRED_OR_UNKNOWN)


@_tune_cases()
def test_retired_and_unknown_tune_values_are_refused(tune):
    """Every value of the list names a retired variant ("Retired GEMM variants"), the ABLATE field of a library built without it, or
    no variant at all: refused with ABX_ERR_ARG, no name, and a text that says `tune`."""
    g = _ln_gemm(ROWS, 768)
    g.tune = tune
    ok, got = _refused(g)
    assert ok, (tune, got)


@_tune_cases()
def test_retired_and_unknown_tune_values_are_refused_on_the_side_descriptor(tune):
    """The same through abx_gemm_side's route (main + side, the bit on the side descriptor)."""
    s = _side(ROWS)
    s.tune = tune
    ok, got = _refused(_ln_gemm(ROWS, 768), s)
    assert ok, (tune, got)


def test_live_tune_bits_are_accepted_and_mean_what_they_meant():
    for tune, name in ((2048, TILE), (1, 'gemm_as_kernel<0, false, 0, false>'), (0, 'gemm_as_kernel<0, false, 0, false>'), (2048 | 1, TILE)):
        g = _ln_gemm(ROWS, 768)
        g.tune = tune
        assert _plan(g) == (0, name), tune


def _transition(M):
    """The fused two-layer transition: LayerNorm-folded 192 -> 768, relu, 768 -> 192 from planes in the permuted k order."""
    g = _ln_gemm(M, 768)
    g.mlp, g.act, g.N2 = 1, 1, 192
    g.B2_split, g.sB23n, g.sB23p, g.sB23k, g.bias2 = 12 * P, 16, 16 * 192, 32 * 192, 13 * P
    g.sCm = 192
    return g


def test_defaults_name_the_same_kernels_where_a_variant_used_to_hang():
    assert _plan(_side(ROWS)) == (0, 'gemm3_kernel<128, 32, 32, 32, 0, true, 6>')
    assert _plan(_transition(ROWS)) == (0, 'gemm3_mlp_kernel<2>')


def test_abx_gemm_tune_with_a_retired_value_fails_at_the_first_plan():
    """An ABX_GEMM_TUNE left over from an old recipe (512 was the narrow ring) fails at the first GEMM, with the guard's message."""
    out = _child('tune_plain', 'ABX_GEMM_TUNE', '512')
    assert out.startswith('refused:') and 'tune' in out and '512' in out, out


def test_abx_gemm_tune_with_a_retired_bit_fails_at_the_first_plan():
    out = _child('tune_plain', 'ABX_GEMM_TUNE', '256')
    assert out.startswith('refused:') and 'tune' in out and '256' in out, out


def test_abx_gemm_tune_tile_only_names_the_tile_kernel():
    assert _child('tune_plain', 'ABX_GEMM_TUNE', '2048') == TILE


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    from abx_amd import ops
    if sys.argv[1] == 'as_plain':
        print(ops.gemm_as_kernel_name(_ln_gemm(ROWS, 768)))
    elif sys.argv[1] == 'dual':
        print(ops.gemm_kernel_name(352 * 352, 192, 128, 100, a_kcontig=False, split=True, exact=2, dual=True))
    elif sys.argv[1] == 'tune_plain':           # the plain case through the product's name helper, which fills in the process's ABX_GEMM_TUNE
        from abx_amd._lib import AbxHipError
        try:
            print(ops.gemm_kernel_name(ROWS, 768, 192, 1, split=True, exact=2))
        except AbxHipError as e:
            print('refused:', e)
