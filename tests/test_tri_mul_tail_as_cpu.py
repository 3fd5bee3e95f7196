"""The tri-mul tail's dispatch as abx_amd.ops.gemm_kernel_name(dual=True, ...) reports it (abx_gemm_plan: csrc/gemm_as.hip as_dual_dispatch
itself, run up to the launch): the name bench.py prices the launch under.  No GPU needed."""


def test_dual_kernel_name_follows_the_launch_size_rule():
    from abx_amd import ops
    tile = 'gemm3_dual_kernel<128, 96, 32, 96, 3>'
    name = lambda M, batch, **kw: ops.gemm_kernel_name(M, kw.pop('N', 192), kw.pop('K', 128), batch, a_kcontig=kw.pop('a_kcontig', False), split=True,
                                                       exact=kw.pop('exact', 2), dual=True, **kw)
    M = 352 * 352
    assert name(M, 100) == 'gemm_as_dual_kernel' and name(M, 1) == 'gemm_as_dual_kernel'          # 1 936 blocks of 64 rows per sample
    assert name(128 * 128, 4) == 'gemm_as_dual_kernel' and name(128 * 128, 3) == tile             # 1 024 blocks / 768
    assert name(118 * 120, 5) == 'gemm_as_dual_kernel' and name(118 * 120, 4) == tile             # 222 blocks per sample (ragged last one)
    assert name(M, 100, exact=1) == tile and name(M, 100, a_kcontig=True) == tile
    assert name(M, 100, N=96) == tile and name(M, 100, K=192) == tile and name(M + 2, 100) == tile
