"""Which kernel the library names for the pair Transition (abx_gemm_plan: the dispatch of csrc/gemm_as.hip and gemm3.hip itself): the
A-stationary fused MLP for the shape class K = 192, hidden 768, 192 outputs with a residual, at ANY number of rows; the tile kernel for every
other shape, under AbxGemm.tune bit 11 and under ABX_NO_MLP_AS.  No GPU.  Run as a script, this file prints the default name: the
environment-switch tests start it as a fresh child process, because the library reads its switches once."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
P = 1 << 40                                         # placeholder "device addresses", never dereferenced
NEW, OLD = 'gemm_as_mlp_kernel', 'gemm3_mlp_kernel<2>'


def _transition(M, K=192, NH=768, N2=192, resid=True, inplace=True):
    from abx_amd._lib import AbxGemm
    g = AbxGemm()
    g.M, g.N, g.K, g.batch, g.alpha, g.exact = M, NH, K, 1, 1.0, 2
    g.A, g.sAm, g.sAk = 1 * P, K, 1
    g.B, g.sBk, g.sBn = 2 * P, NH, 1
    g.B_split, g.sB3n, g.sB3p, g.sB3k, g.b_f16 = 3 * P, 16, 16 * NH, 32 * NH, 1
    g.C, g.sCm = (1 * P if inplace else 4 * P), N2
    g.ln_csum, g.bias, g.ln_eps = 5 * P, 6 * P, 1e-5
    g.mlp, g.act, g.N2 = 1, 1, N2
    g.B2_split, g.sB23n, g.sB23p, g.sB23k, g.bias2 = 12 * P, 16, 16 * N2, 32 * N2, 13 * P
    if resid:
        g.resid, g.sRm = 1 * P, N2
    return g


def _plan(g):
    from abx_amd import _lib
    buf = ctypes.create_string_buffer(128)
    rc = _lib.load().abx_gemm_plan(ctypes.byref(g), None, buf, len(buf))
    return rc, buf.value.decode()


def test_the_shape_class_takes_the_a_stationary_kernel_at_any_m():
    for M in (1, 64, 65, 2 * 33 * 33, 1023 * 64, 1024 * 64, 100 * 352 * 352):
        assert _plan(_transition(M)) == (0, NEW), M
        assert _plan(_transition(M, inplace=False)) == (0, NEW), M


def test_other_shapes_and_the_tile_bit_keep_the_tile_kernel():
    assert _plan(_transition(1000, K=64, NH=272, N2=96, inplace=False)) == (0, OLD)
    assert _plan(_transition(1024 * 64, NH=640)) == (0, OLD)
    assert _plan(_transition(1024 * 64, N2=96, inplace=False)) == (0, OLD)
    assert _plan(_transition(1024 * 64, resid=False)) == (0, OLD)          # the kernel IS "+ z": its epilogue always reads the residual rows
    g = _transition(1024 * 64)
    g.tune = 2048
    assert _plan(g) == (0, OLD)


def test_rows_that_partly_overlap_the_output_keep_the_tile_kernel():
    g = _transition(1024 * 64)
    g.C = 1 * P + 192 * 4 * 64            # the output starts 64 rows into the input rows: neither in place nor apart
    assert _plan(g) == (0, OLD)


def _child(value):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, ABX_NO_MLP_AS=value), capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.strip().splitlines()[-1]


def test_abx_no_mlp_as_keeps_the_tile_kernel_everywhere():
    assert _child('1') == OLD


def test_abx_no_mlp_as_set_to_0_is_off():
    assert _child('0') == NEW


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    print(_plan(_transition(1024 * 64))[1])
