"""Kernel-level fp64 parity of abx_gemm's tile kernels at every dispatch, tile, K and alignment edge: the exact fp32 kernels of
csrc/gemm.hip and the split-f16 tile kernels of csrc/gemm3.hip against the float64 evaluation of the same operation (tests/gemm_cases.py,
whose table, references and bound are checked on the CPU in tests/test_gemm_cases_host.py).

Every case asserts the kernel instantiation the library plans for the REAL descriptor (ops.gemm(..., defer=True), then abx_gemm_plan:
real alignment counts), launches that descriptor into an output that is a view inside a larger buffer of 0xFF bytes (8 guard rows behind
the last row and 4 guard columns beside it; in its own orientation for the transposed store), and asserts a finite output, untouched
guards and the bound.

The bound.  The yardstick is the reference's own float32 evaluation (G.baseline), never a kernel: with e = G.err(GPU output) and
e32 = G.err(baseline), both (max, mean) of |out - float64|, every case asserts e.max <= K_MAX * e32.max and, from 1024 outputs on,
e.mean <= K_MEAN * e32.mean; where e32 is 0 the exact value is required.  K_MAX / K_MEAN are the smallest powers of two at or
above the largest measured ratio, capped at 4 / 2: the exact kernels are an ordered fma chain over k - which is what torch's float32
matmul on the CPU turns out to be as well - and the project already holds a split-f16 GEMM to 1.5 x / 1.2 x of the exact one
(test_gemm_split_accuracy_vs_exact).  A case above the cap is a finding: a kernel fault is fixed, anything else gets an entry in
CASE_FACTORS with its derivation beside it.

Measured ratios e / e32 on an MI355X, (max, mean) per case - the table the constants were read from (case ids as `pytest` shows them:
family-MxNxK[-bBATCH]-A<layout>-B<layout>[-T]-e<exact>[+epilogue][-mis<operand>][-off<sigma>]; the kernel of each is in gemm_cases.py):

    exact fp32 kernels                                                            max    mean
    x-small-1x1x1-Ak-Bn-e1                                                        1.000  1.000
    x-small-37x20x256-Ak-Bn-e1                                                    1.640  1.288
    x-small-513x192x192-Ak-Bn-e1                                                  1.000  1.000
    x-small-130x32x52-Ak-Bn-e1                                                    1.000  1.000
    x-small-130x32x52-Ak-Bk-e1                                                    1.000  1.000
    x-small-130x32x52-Am-Bn-e1                                                    1.000  1.000
    x-small-130x32x52-Am-Bk-e1                                                    1.000  1.000
    x-small-130x33x52-Ak-Bn-e1                                                    1.000  0.998
    x-small-130x33x52-Ak-Bk-e1                                                    1.000  0.998
    x-small-130x33x52-Am-Bn-e1                                                    1.000  0.998
    x-small-130x33x52-Am-Bk-e1                                                    1.000  0.998
    x-small-130x64x52-Ak-Bn-e1                                                    1.000  1.000
    x-small-130x64x52-Ak-Bk-e1                                                    1.000  1.000
    x-small-130x64x52-Am-Bn-e1                                                    1.000  1.000
    x-small-130x64x52-Am-Bk-e1                                                    1.000  1.000
    x-small-130x65x52-Ak-Bn-e1                                                    1.000  0.999
    x-small-130x65x52-Ak-Bk-e1                                                    1.000  0.999
    x-small-130x65x52-Am-Bn-e1                                                    1.000  0.999
    x-small-130x65x52-Am-Bk-e1                                                    1.000  0.999
    x-k-130x65x1-Ak-Bn-e1                                                         1.000  1.000
    x-k-130x65x1-Ak-Bn-e1-misA-misB                                               1.000  1.000
    x-k-130x65x1-Am-Bk-e1                                                         1.000  1.000
    x-k-130x65x15-Ak-Bn-e1                                                        1.000  0.999
    x-k-130x65x15-Ak-Bn-e1-misA-misB                                              1.000  0.999
    x-k-130x65x15-Am-Bk-e1                                                        1.000  0.999
    x-k-130x65x16-Ak-Bn-e1                                                        1.000  1.001
    x-k-130x65x16-Ak-Bn-e1-misA-misB                                              1.000  1.001
    x-k-130x65x16-Am-Bk-e1                                                        1.000  1.001
    x-k-130x65x17-Ak-Bn-e1                                                        1.000  1.000
    x-k-130x65x17-Ak-Bn-e1-misA-misB                                              1.000  1.000
    x-k-130x65x17-Am-Bk-e1                                                        1.000  1.000
    x-k-130x65x31-Ak-Bn-e1                                                        1.000  1.000
    x-k-130x65x31-Ak-Bn-e1-misA-misB                                              1.000  1.000
    x-k-130x65x31-Am-Bk-e1                                                        1.000  1.000
    x-k-130x65x32-Ak-Bn-e1                                                        1.000  1.000
    x-k-130x65x32-Ak-Bn-e1-misA-misB                                              1.000  1.000
    x-k-130x65x32-Am-Bk-e1                                                        1.000  1.000
    x-k-130x65x33-Ak-Bn-e1                                                        1.000  0.998
    x-k-130x65x33-Ak-Bn-e1-misA-misB                                              1.000  0.998
    x-k-130x65x33-Am-Bk-e1                                                        1.000  0.998
    x-launch-32640x256x16-Ak-Bn-e1                                                1.000  1.000
    x-launch-32641x256x16-Ak-Bn-e1                                                1.000  1.000
    x-launch-32641x192x16-Ak-Bn-e1                                                1.000  1.000
    x-launch-16385x448x16-Ak-Bn-e1                                                1.000  1.000
    x-launch-21889x384x17-Ak-Bn-e1                                                1.000  1.000
    x-launch-257x130x24-b128-Ak-Bn-e1                                             1.000  1.000
    x-layout-32641x256x16-Ak-Bn-e1                                                1.000  1.000
    x-layout-32641x256x17-Ak-Bn-e1                                                1.000  1.000
    x-misalign-32641x256x16-Ak-Bn-e1-misA-misB                                    1.000  1.000
    x-layout-32641x256x16-Ak-Bk-e1                                                1.000  1.000
    x-layout-32641x256x17-Ak-Bk-e1                                                1.000  1.000
    x-misalign-32641x256x16-Ak-Bk-e1-misA-misB                                    1.000  1.000
    x-layout-32641x256x16-Am-Bn-e1                                                1.000  1.000
    x-layout-32641x256x17-Am-Bn-e1                                                1.000  1.000
    x-misalign-32641x256x16-Am-Bn-e1-misA-misB                                    1.000  1.000
    x-layout-32641x256x16-Am-Bk-e1                                                1.000  1.000
    x-layout-32641x256x17-Am-Bk-e1                                                1.000  1.000
    x-misalign-32641x256x16-Am-Bk-e1-misA-misB                                    1.000  1.000
    x-layout-32641x192x16-Ak-Bn-e1                                                1.000  1.000
    x-layout-32641x192x17-Ak-Bn-e1                                                1.000  1.000
    x-misalign-32641x192x16-Ak-Bn-e1-misA-misB                                    1.000  1.000
    x-layout-32641x192x16-Ak-Bk-e1                                                1.000  1.000
    x-layout-32641x192x17-Ak-Bk-e1                                                1.000  1.000
    x-misalign-32641x192x16-Ak-Bk-e1-misA-misB                                    1.000  1.000
    x-layout-32641x192x16-Am-Bn-e1                                                1.000  1.000
    x-layout-32641x192x17-Am-Bn-e1                                                1.000  1.000
    x-misalign-32641x192x16-Am-Bn-e1-misA-misB                                    1.000  1.000
    x-layout-32641x192x16-Am-Bk-e1                                                1.000  1.000
    x-layout-32641x192x17-Am-Bk-e1                                                1.000  1.000
    x-misalign-32641x192x16-Am-Bk-e1-misA-misB                                    1.000  1.000
    x-ts-130x45x52-Ak-Bn-T-e1                                                     1.000  1.000
    x-ts-130x45x52-Ak-Bn-T-e1+gate+resid+rowscale                                 1.000  1.015
    x-ts-130x45x52-Ak-Bn-T-e1-misC                                                1.000  1.000
    x-ts-130x45x52-Ak-Bn-T-e1+gate+resid+rowscale-misC-misgate-misresid           1.000  1.015
    x-ts-130x20x52-Ak-Bn-T-e1                                                     1.000  0.982
    x-ts-130x20x52-Ak-Bn-T-e1+gate+resid+rowscale                                 0.684  0.999
    x-ts-130x20x52-Ak-Bn-T-e1-misC                                                1.000  0.982
    x-ts-130x20x52-Ak-Bn-T-e1+gate+resid+rowscale-misC-misgate-misresid           0.684  0.999
    x-ts-130x65x52-Ak-Bn-T-e1                                                     1.000  0.999
    x-ts-130x65x52-Ak-Bn-T-e1+gate+resid+rowscale                                 1.111  1.000
    x-ts-130x65x52-Ak-Bn-T-e1-misC                                                1.000  0.999
    x-ts-130x65x52-Ak-Bn-T-e1+gate+resid+rowscale-misC-misgate-misresid           1.111  1.000
    x-ts-32641x256x16-Ak-Bn-T-e1                                                  1.000  1.000
    x-ts-32641x256x16-Ak-Bn-T-e1+gate+resid+rowscale                              1.000  1.010
    x-ts-32641x256x16-Ak-Bn-T-e1-misC                                             1.000  1.000
    x-ts-32641x256x16-Ak-Bn-T-e1+gate+resid+rowscale-misC-misgate-misresid        1.000  1.010
    x-ts-32641x192x16-Ak-Bn-T-e1                                                  1.000  1.000
    x-ts-32641x192x16-Ak-Bn-T-e1+gate+resid+rowscale                              1.000  1.010
    x-ts-32641x192x16-Ak-Bn-T-e1-misC                                             1.000  1.000
    x-ts-32641x192x16-Ak-Bn-T-e1+gate+resid+rowscale-misC-misgate-misresid        1.000  1.010
    x-epi-130x65x52-Ak-Bn-e1+alpha+bias+gate+relu+resid+rowscale                  1.128  1.017
    x-epi-130x65x52-Ak-Bn-e1+alpha+bias+gate_raw+resid+rowscale+sigmoid           0.711  1.027
    x-epi-130x65x52-Ak-Bn-e1+a_relu                                               1.000  1.000
    x-epi-130x65x52-Ak-Bn-e1+alpha+bias+gate+relu+resid+rowscale-misC-misgate-misresid  1.128  1.017
    x-epi-32641x192x16-Ak-Bn-e1+alpha+bias+gate+relu+resid+rowscale               0.791  1.010
    x-epi-32641x192x16-Ak-Bn-e1+alpha+bias+gate_raw+resid+rowscale+sigmoid        1.074  1.020
    x-epi-32641x192x16-Ak-Bn-e1+a_relu                                            1.000  1.000
    x-epi-32641x192x16-Ak-Bn-e1+alpha+bias+gate+relu+resid+rowscale-misC-misgate-misresid  0.791  1.010
    x-epi-130x67x52-Ak-Bn-e1+alpha+bias+gate+relu+resid+rowscale-misA-misB-misC-misgate-misresid  1.000  0.993
    x-ln-300x192x192-Ak-Bn-e1+bias+ln_stats                                       1.023  0.989
    x-ln-300x192x192-Ak-Bn-e1+bias+ln_stats-off3                                  4.549  2.536    CASE_FACTORS
    x-ln-300x192x192-Ak-Bn-e1+bias+ln_stats-off30                                 7.339  7.461    CASE_FACTORS
    x-ln-300x192x192-Am-Bn-e1+bias+ln_stats                                       1.023  0.989
    x-ln-300x192x192-Am-Bn-e1+bias+ln_stats-off3                                  4.549  2.536    CASE_FACTORS
    x-ln-300x192x192-Am-Bn-e1+bias+ln_stats-off30                                 7.339  7.461    CASE_FACTORS
    x-ln-300x192x192-Ak-Bn-e1+bias+ln_inline                                      1.603  1.384
    x-ln-300x192x192-Ak-Bn-e1+bias+ln_inline-off3                                 2.599  1.229
    x-ln-300x192x192-Ak-Bn-e1+bias+ln_inline-off30                                0.583  0.358
    x-ln-300x192x192-Am-Bn-e1+bias+ln_inline                                      1.417  1.390    (before the fix: 0.846  1.014)
    x-ln-300x192x192-Am-Bn-e1+bias+ln_inline-off3                                 2.363  1.250    (before the fix: 4.312  3.959)
    x-ln-300x192x192-Am-Bn-e1+bias+ln_inline-off30                                0.611  0.353    (before the fix: 90.42  60.08)
    x-ln-32641x192x128-Ak-Bn-e1+bias+ln_stats                                     1.334  0.979
    x-ln-32641x192x128-Ak-Bn-e1+bias+ln_stats-off3                                2.884  2.443    CASE_FACTORS
    x-ln-32641x192x128-Ak-Bn-e1+bias+ln_stats-off30                               5.471  5.528    CASE_FACTORS
    x-ln-32641x192x128-Am-Bn-e1+bias+ln_stats                                     1.334  0.979
    x-ln-32641x192x128-Am-Bn-e1+bias+ln_stats-off3                                2.884  2.443    CASE_FACTORS
    x-ln-32641x192x128-Am-Bn-e1+bias+ln_stats-off30                               5.471  5.528    CASE_FACTORS
    x-ln-32641x192x128-Ak-Bn-e1+bias+ln_inline                                    3.080  1.470
    x-ln-32641x192x128-Ak-Bn-e1+bias+ln_inline-off3                               2.051  1.167
    x-ln-32641x192x128-Ak-Bn-e1+bias+ln_inline-off30                              0.487  0.274
    x-ln-32641x192x128-Am-Bn-e1+bias+ln_inline                                    2.286  1.460    (before the fix: 0.971  0.996)
    x-ln-32641x192x128-Am-Bn-e1+bias+ln_inline-off3                               2.105  1.159    (before the fix: 3.064  3.465)
    x-ln-32641x192x128-Am-Bn-e1+bias+ln_inline-off30                              0.487  0.271    (before the fix: 49.95  38.38)

    split-f16 tile kernels                                                        max    mean
    s-tile-64x128x16-Ak-Bweights-e2                                               0.760  1.181
    s-tile-65x128x16-Ak-Bweights-e2                                               0.996  1.225
    s-tile-129x128x32-Ak-Bweights-e2                                              0.748  1.003
    s-tile-49024x128x16-Ak-Bweights-e2                                            0.955  1.227
    s-tile-49025x128x16-Ak-Bweights-e2                                            0.819  1.236
    s-tile-130x192x16-Ak-Bweights-e2                                              1.486  1.237
    s-tile-130x190x16-Ak-Bweights-e2                                              1.176  1.195
    s-tile-130x448x16-Ak-Bweights-e2                                              0.801  1.259
    s-tile-130x768x16-Ak-Bweights-e2                                              1.017  1.228
    s-tile-130x65x16-Ak-Bweights-e2                                               0.720  1.216
    s-ring-64x128x16-Ak-Bweights-e2                                               0.760  1.181
    s-ring-130x128x16-Ak-Bweights-e2                                              1.018  1.242
    s-ring-130x192x16-Ak-Bweights-e2                                              1.486  1.237
    s-ring-64x128x32-Ak-Bweights-e2                                               0.613  1.031
    s-ring-130x128x32-Ak-Bweights-e2                                              0.635  1.011
    s-ring-130x192x32-Ak-Bweights-e2                                              0.824  1.009
    s-ring-64x128x48-Ak-Bweights-e2                                               0.525  0.911
    s-ring-130x128x48-Ak-Bweights-e2                                              0.908  0.906
    s-ring-130x192x48-Ak-Bweights-e2                                              0.677  0.935
    s-ring-64x128x64-Ak-Bweights-e2                                               0.499  0.856
    s-ring-130x128x64-Ak-Bweights-e2                                              0.742  0.865
    s-ring-130x192x64-Ak-Bweights-e2                                              0.649  0.854
    s-ring-64x128x192-Ak-Bweights-e2                                              0.533  0.716
    s-ring-130x128x192-Ak-Bweights-e2                                             0.643  0.707
    s-ring-130x192x192-Ak-Bweights-e2                                             0.675  0.716
    s-rows-1x128x32-Ak-Bweights-e2+bias                                           0.606  1.018
    s-rows-1x192x32-Ak-Bweights-e2+bias                                           0.559  0.812
    s-rows-63x128x32-Ak-Bweights-e2+bias                                          0.797  1.006
    s-rows-63x192x32-Ak-Bweights-e2+bias                                          0.659  0.986
    s-rows-64x128x32-Ak-Bweights-e2+bias                                          0.862  1.013
    s-rows-64x192x32-Ak-Bweights-e2+bias                                          0.695  1.023
    s-rows-65x128x32-Ak-Bweights-e2+bias                                          0.552  1.034
    s-rows-65x192x32-Ak-Bweights-e2+bias                                          0.857  1.008
    s-rows-127x128x32-Ak-Bweights-e2+bias                                         0.726  1.010
    s-rows-127x192x32-Ak-Bweights-e2+bias                                         0.631  1.014
    s-rows-128x128x32-Ak-Bweights-e2+bias                                         0.944  1.015
    s-rows-128x192x32-Ak-Bweights-e2+bias                                         0.516  0.995
    s-rows-129x128x32-Ak-Bweights-e2+bias                                         0.857  1.012
    s-rows-129x192x32-Ak-Bweights-e2+bias                                         0.756  0.990
    s-narrow-130x1x16-Ak-Bweights-e2+alpha+bias                                   0.988  0.996
    s-narrow-130x1x16-Ak-Bweights-T-e2+alpha+bias                                 0.988  0.996
    s-narrow-130x4x16-Ak-Bweights-e2+alpha+bias                                   0.428  1.017
    s-narrow-130x4x16-Ak-Bweights-T-e2+alpha+bias                                 0.428  1.017
    s-narrow-130x12x16-Ak-Bweights-e2+alpha+bias                                  0.544  1.122
    s-narrow-130x12x16-Ak-Bweights-T-e2+alpha+bias                                0.544  1.122
    s-narrow-130x31x16-Ak-Bweights-e2+alpha+bias                                  1.476  1.202
    s-narrow-130x31x16-Ak-Bweights-T-e2+alpha+bias                                1.476  1.202
    s-narrow-130x32x16-Ak-Bweights-e2+alpha+bias                                  0.803  1.155
    s-narrow-130x32x16-Ak-Bweights-T-e2+alpha+bias                                0.803  1.155
    s-narrow-130x1x192-Ak-Bweights-e2+alpha+bias                                  1.015  1.032
    s-narrow-130x1x192-Ak-Bweights-T-e2+alpha+bias                                1.015  1.032
    s-narrow-130x4x192-Ak-Bweights-e2+alpha+bias                                  0.756  0.714
    s-narrow-130x4x192-Ak-Bweights-T-e2+alpha+bias                                0.756  0.714
    s-narrow-130x12x192-Ak-Bweights-e2+alpha+bias                                 0.608  0.681
    s-narrow-130x12x192-Ak-Bweights-T-e2+alpha+bias                               0.608  0.681
    s-narrow-130x31x192-Ak-Bweights-e2+alpha+bias                                 0.441  0.699
    s-narrow-130x31x192-Ak-Bweights-T-e2+alpha+bias                               0.441  0.699
    s-narrow-130x32x192-Ak-Bweights-e2+alpha+bias                                 0.598  0.697
    s-narrow-130x32x192-Ak-Bweights-T-e2+alpha+bias                               0.598  0.697
    s-rowA-132x192x16-Am-Bweights-e2                                              0.992  1.234
    s-rowA-132x128x16-Am-Bweights-e2                                              0.988  1.234    (before the fix: 8.8e6  2.1e7)
    s-rowA-4x128x16-Am-Bweights-e2                                                0.974  1.277
    s-rowA-132x192x48-Am-Bweights-e2+alpha+bias+gate+relu+resid+rowscale          0.740  0.955
    s-ts-130x128x16-Ak-Bweights-T-e2                                              1.018  1.242
    s-ts-130x192x16-Ak-Bweights-T-e2                                              1.486  1.237
    s-ts-64x128x16-Ak-Bweights-T-e2                                               0.760  1.181
    s-ts-130x128x48-Ak-Bweights-T-e2+gate+resid+rowscale                          0.655  0.943
    s-ts-130x192x48-Ak-Bweights-T-e2+gate+resid+rowscale-misC-misgate-misresid    0.914  0.935
    s-epi-130x128x48-Ak-Bweights-e2+alpha+bias+gate+relu+resid+rowscale           0.693  0.946
    s-epi-130x192x48-Ak-Bweights-e2+alpha+bias+gate_raw+resid+rowscale+sigmoid-misC-misgate-misresid  1.075  1.013
    s-epi-64x128x48-Ak-Bweights-e2+a_relu+bias+relu                               0.844  1.173
    s-planes-64x64x64-b3-Aplanes-Bplanes-e2                                       0.772  0.690
    s-planes-65x65x80-b3-Aplanes-Bplanes-e2                                       0.546  0.744
    s-planes-97x97x112-b2-Aplanes-Bplanes-e2                                      0.400  0.724
    s-planes-352x352x352-b2-Aplanes-Bplanes-e2                                    0.798  0.840
    s-oln-130x128x192-Ak-Bweights-e2+bias+out_ln                                  0.752  0.769
    s-oln-130x100x192-Ak-Bweights-e2+bias+out_ln                                  0.906  0.767
    s-oln-1x128x32-Ak-Bweights-e2+bias+out_ln                                     0.559  0.843
    s-oln-127x128x32-Ak-Bweights-e2+bias+out_ln                                   0.870  1.039
    s-oln-128x128x32-Ak-Bweights-e2+bias+out_ln                                   0.621  0.997
    s-oln-129x128x32-Ak-Bweights-e2+bias+out_ln                                   0.780  0.992
    s-ln-132x192x128-Ak-Bweights-e2+bias+ln_inline                                0.967  1.125
    s-ln-132x128x128-Ak-Bweights-e2+bias+ln_inline                                1.396  1.171
    s-ln-132x192x128-Ak-Bweights-e2+bias+ln_inline-off30                          0.270  0.217
    s-ln-132x128x128-Ak-Bweights-e2+bias+ln_inline-off30                          0.368  0.227
    s-ln-132x192x128-Am-Bweights-e2+bias+ln_inline                                0.967  1.125
    s-ln-132x128x128-Am-Bweights-e2+bias+ln_inline                                1.396  1.171    (before the fix: 3.5e6  7.3e6)
    s-ln-132x192x128-Am-Bweights-e2+bias+ln_inline-off30                          0.270  0.217
    s-ln-132x128x128-Am-Bweights-e2+bias+ln_inline-off30                          0.368  0.227    (before the fix: 7.5e5  1.5e6)
    s-away-130x64x16-Ak-Bweights-e2                                               1.000  1.000
    s-away-130x33x16-Ak-Bweights-e2                                               1.000  0.999
    s-away-130x192x24-Ak-Bweights-e2                                              1.000  1.000
    s-away-130x192x16-Am-Bweights-e2                                              1.000  1.000
    s-away-2x192x16-Am-Bweights-e2                                                1.000  0.866
    s-away-130x192x16-Ak-Bweights-e2-misA                                         1.000  1.000
    s-size-32640x128x16-Ak-Bweights-e0                                            1.000  1.000
    s-size-32641x128x16-Ak-Bweights-e0                                            0.920  1.239

    single-tile fused forms (test_fused_form_row_edges)                           max    mean
    fused-mlp1-M1                                                                 0.603  0.777
    fused-mlp1-M127                                                               2.099  1.301
    fused-mlp1-M128                                                               2.143  1.268
    fused-mlp1-M129                                                               2.998  1.309
    fused-mlp2-M1                                                                 0.778  0.814
    fused-mlp2-M127                                                               0.453  0.821
    fused-mlp2-M128                                                               0.869  0.819
    fused-mlp2-M129                                                               0.761  0.809
    fused-dual-M1                                                                 0.511  0.743
    fused-dual-M127                                                               1.448  1.105
    fused-dual-M128                                                               2.076  1.108
    fused-dual-M129                                                               1.538  1.200

Outside CASE_FACTORS the largest max-ratio is 3.080 (exact kernel, inline statistics, k-contiguous rows of mean 0: the shift by the first
element costs a row whose first element is an outlier what test_gpu_pair_modules.py describes) and the largest mean-ratio 1.470 (same
case): K_MAX = 4, K_MEAN = 2.  Without a LayerNorm the exact kernels give 1.000 / 1.000 throughout - the bits of torch's float32 matmul -
and the split-f16 tiles stay within 1.49 / 1.28.

Two kernel faults were found by these cases and are fixed with them:
  - gemm_block of gemm.hip, m-contiguous A with inline statistics, added x and x^2 unshifted and formed sq / K - mean^2: 4.3 x / 4.0 x at
    rows of mean 3 sigma and 90 x / 60 x at 30 sigma (K = 192; 3.1 / 3.5 and 50 / 38 at the tri-mul tail's own K = 128).  It now shifts
    each row by its element at k = 0, operand and sums alike, as the k-contiguous path and gemm3_mainloop.h do: 2.4 / 1.3 and 0.6 / 0.4.
  - gemm3_kernel<64, 128, 32, 64, 1, ...> (the 64-row split tile with a row-contiguous A: M % 4 == 0, 64 < M, fewer than 384 tiles of
    128 x 128 and no wide tile; the network's one row-contiguous operand, the tri-mul product, meets N = 192 and the wide tile) computed
    its DMA sources for a 128-row stage, 2 k-rows of 32 lanes per instruction where a 64-row stage takes 4 of 16: errors of the size of
    the output (max 5.1, mean 1.05 against outputs of variance 1).  gemm3_mainloop.h now derives both numbers from BM.

The contracts, as equal bits of an entry point with itself: rows 0 .. 63 of a split-f16 problem do not depend on M (M = 64: the 128-row
tile because M <= 64; M = 129: the 64-row tile; M = 49025: the 128-row tile by the launch-size rule - the claim at the tile choice of
abx_gemm3_dispatch), plain and with inline LayerNorm statistics; an exact-kernel problem gives the same bits with aligned operands
(16-byte loads and stores) and with every operand one float off (scalar ones); at K = 32 (interior blocks) and at K = 33 with a zero last
column (predicated blocks); exact = 2 and exact = 0 above the size rule are the same launch.

The single-tile fused forms (AbxGemm.mlp = 1 | 2 and the dual GEMM) get their missing row edges M = 1, 127, 128, 129 here, through the
calls test_gemm_fused_transition, test_gemm_gated_tail and test_gemm_dual_proj_out_times_gate of test_gpu_kernels.py make, under the same
bound.  Needs an MI355X: `pytest -m gpu`."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import gemm_cases as G

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
K_MAX, K_MEAN = G.K_MAX, G.K_MEAN
# a case above the cap keeps its own factors here, with the derivation next to it: {case name: (k_max, k_mean)}
# 'ln_stats' at rows of mean `offset` sigma.  With the statistics GIVEN the fold cannot shift its operand (the rows go to the matrix cores
# as they are - gemm.hip, head), so the accumulator holds acc = sigma y / rstd' + mean csum[n], where y is the normalised product that the
# reference's float32 text accumulates directly: every rounding of the fma chain is relative to a value (|y| + offset |csum|) / |y| times
# larger than the reference's.  y and csum[n] are sums of the same K weights against unit-variance | unit factors, so that ratio is
# 1 + offset in the mean square, and the bound is K_MAX, K_MEAN times 1 + offset: 16 / 8 at 3 sigma, 124 / 62 at 30.  (The inline
# statistics shift and need no entry.)
CASE_FACTORS = {c.name: (K_MAX * (1 + c.offset), K_MEAN * (1 + c.offset)) for c in G.CASES if 'ln_stats' in c.epi and c.offset}


@pytest.fixture(scope='module')
def ops():
    from abx_amd import ops as _ops, _lib
    lib = _lib.load()
    assert lib.abx_init(0) == 0, lib.abx_last_error_string()
    return _ops


def bits(t):
    return t.contiguous().view(torch.int32)


def scratch(numel, fill=0xFF):
    """A flat device buffer of float32 whose every BYTE is `fill`: 0xFF reads as NaN."""
    t = torch.empty(numel, device=DEV, dtype=torch.float32)
    t.view(torch.uint8).fill_(fill)
    return t


def place(t, v):
    """The logical tensor t at the place G.layout gives it: (flat buffer, strided view)."""
    flat = scratch(v.numel + 8)
    view = flat.as_strided(v.shape, v.strides, v.offset)
    view.copy_(t.to(DEV))
    return flat, view


def launch(ops, c, x=None):
    """abx_gemm on the operands of case c (x: other logical tensors than G.inputs(c)) laid out as G.layout(c) says.  Returns (the planned
    kernel name, the output view (batch, M, N), the int32 image of everything in the output buffer that is NOT the view)."""
    from abx_amd import _lib
    x = G.inputs(c) if x is None else x
    L = G.layout(c)
    kw, keep = {}, []
    if c.a_layout == 'planes':
        A, B = x['A_planes'].to(DEV), x['B_planes'].to(DEV)
    else:
        (fa, A), (fb, B) = place(x['A'], L['A']), place(x['B'], L['B'])
        keep += [fa, fb]
        if c.b_layout == 'weights':
            kw['B3'] = ops.split_weights(B[0])
    nbuf = L['C'].offset + math.prod(L['Cbuf']) + 8
    cflat = scratch(nbuf)
    out = cflat.as_strided(L['C'].shape, L['C'].strides, L['C'].offset)
    for name in ('gate', 'resid'):
        if name in c.epi or (name == 'gate' and 'gate_raw' in c.epi):
            f_, kw[name] = place(x[name], L[name])
            keep.append(f_)
    if 'bias' in c.epi:
        kw['bias'] = x['bias'].to(DEV)
    if 'rowscale' in c.epi:
        kw['rowscale'] = x['rowscale'].to(DEV)
    if 'ln_stats' in c.epi or 'ln_inline' in c.epi:
        kw['ln'] = (x['stats'].to(DEV) if 'ln_stats' in c.epi else None, x['csum'].to(DEV))
    if 'out_ln' in c.epi:
        kw['out_ln'] = (x['oln_w'].to(DEV), x['oln_b'].to(DEV))
    g = ops.gemm(A, B, out, a_relu='a_relu' in c.epi, alpha=G.ALPHA if 'alpha' in c.epi else 1.0,
                 act=1 if 'relu' in c.epi else 2 if 'sigmoid' in c.epi else 0, gate_sigmoid='gate' in c.epi, exact=c.exact, defer=True, **kw)
    rc, name = G.plan(g)
    assert rc == 0, _lib.load().abx_last_error_string()
    ops.check(_lib.load().abx_gemm(ctypes.byref(g), ops._stream()), 'abx_gemm')
    torch.cuda.synchronize()
    inside = torch.zeros(nbuf, dtype=torch.bool, device=DEV)
    inside.as_strided(L['C'].shape, L['C'].strides, L['C'].offset).fill_(True)
    assert int(inside.sum()) == G.outputs(c)
    return name, out, cflat.view(torch.int32)[~inside]


def ratios(e, e32):
    r = lambda a, b: (a / b) if b > 0 else (0.0 if a == 0 else math.inf)
    return r(e[0], e32[0]), r(e[1], e32[1])


def assert_bound(c, e, e32, label='GEMM-CASE'):
    r_max, r_mean = ratios(e, e32)
    print(f'{label} {c.name}: e32 max {e32[0]:.3e} mean {e32[1]:.3e}; e max {e[0]:.3e} mean {e[1]:.3e}; ratio max {r_max:.3f} mean {r_mean:.3f}; {c.kernel}')
    assert G.within_bound(c, e, e32, CASE_FACTORS.get(c.name)), (c.name, round(r_max, 3), round(r_mean, 3))


@pytest.mark.parametrize('c', G.CASES, ids=G.case_id)
def test_gemm_case_parity(ops, c):
    e32 = G.baseline_err(c)
    name, out, guard = launch(ops, c)
    assert name == c.kernel
    assert bool(torch.isfinite(out).all()), int((~torch.isfinite(out)).sum())
    assert bool((guard == -1).all()), ('stores outside the output view', int((guard != -1).sum()))
    assert_bound(c, G.err(out, c), e32)


# ---- equal-bits contracts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('epi,N,K', [((), 128, 32), (('bias', 'ln_inline'), 128, 128)], ids=['plain', 'ln_inline'])
def test_split_rows_do_not_depend_on_the_row_tile(ops, epi, N, K):
    big = G.Case('rows', 49025, N, K, 1, 'k', 'weights', 'plain', 2, frozenset(epi), frozenset(), 3 if epi else 0, None, 'bits')
    x = G.inputs(big)
    res = {}
    for M, kernel in ((64, G.S128), (129, G.S64), (49025, G.S128)):
        xm = {k: (v[:, :M] if k == 'A' else v) for k, v in x.items()}
        name, out, guard = launch(ops, big._replace(M=M), xm)
        assert name == kernel % (0, 'false') and bool((guard == -1).all()) and bool(torch.isfinite(out).all())
        res[M] = bits(out[:, :64])
    assert torch.equal(res[64], res[129]) and torch.equal(res[64], res[49025])


ALL_OFF = frozenset(('A', 'B', 'C', 'gate', 'resid'))


@pytest.mark.parametrize('name', ['x-epi-130x65x52-Ak-Bn-e1+alpha+bias+gate+relu+resid+rowscale', 'x-epi-32641x192x16-Ak-Bn-e1+alpha+bias+gate+relu+resid+rowscale',
                                  'x-layout-32641x256x16-Am-Bk-e1', 'x-ts-32641x192x16-Ak-Bn-T-e1+gate+resid+rowscale'])
def test_exact_aligned_and_misaligned_operands_give_the_same_bits(ops, name):
    c = G.BY_NAME[name]
    assert not c.misalign
    n0, a, g0 = launch(ops, c)
    n1, b, g1 = launch(ops, c._replace(misalign=ALL_OFF))
    assert n0 == n1 == c.kernel and bool((g0 == -1).all()) and bool((g1 == -1).all()) and bool(torch.isfinite(a).all())
    assert torch.equal(bits(a), bits(b)), int((bits(a) != bits(b)).sum())


@pytest.mark.parametrize('M,N,kernel', [(130, 65, G.X64), (32641, 192, G.X192)])
def test_exact_interior_and_predicated_blocks_give_the_same_bits(ops, M, N, kernel):
    c = G.Case('k32', M, N, 32, 1, 'k', 'n', 'plain', 1, frozenset(('bias',)), frozenset(), 0, None, 'bits')
    x = G.inputs(c)
    x33 = dict(x, A=torch.cat([x['A'], torch.zeros(1, M, 1)], 2), B=torch.cat([x['B'], torch.zeros(1, 1, N)], 1))
    n0, a, _ = launch(ops, c)
    n1, b, _ = launch(ops, c._replace(K=33), x33)
    assert n0 == n1 == kernel % G.FLAGS['k', 'n'] and bool(torch.isfinite(a).all())
    assert torch.equal(bits(a), bits(b)), int((bits(a) != bits(b)).sum())


def test_exact_2_and_exact_0_above_the_size_rule_give_the_same_bits(ops):
    c = G.BY_NAME['s-size-32641x128x16-Ak-Bweights-e0']
    n0, a, _ = launch(ops, c)
    n1, b, _ = launch(ops, c._replace(exact=2))
    assert n0 == n1 == c.kernel and bool(torch.isfinite(a).all()) and torch.equal(bits(a), bits(b))


# ---- the row edges of the single-tile fused forms ---------------------------------------------------------------------------------------
def _norm(v):
    return F.layer_norm(v, (v.shape[-1],), None, None, G.EPS)


def fused_text(form, t, dtype):
    """The three fused forms in plain torch, `dtype` throughout, on the operands as the kernels get them: LayerNorm folded (weights scaled
    by gamma, beta in the bias - fold_ln), so the rows are normalised without an affine part."""
    t = {k: v.to(dtype) for k, v in t.items()}
    if form == 'mlp1':      # LayerNorm -> Linear -> ReLU -> Linear + residual
        return torch.relu(_norm(t['z']) @ t['w1'] + t['b1']) @ t['w2'] + t['b2'] + t['z']
    if form == 'mlp2':      # (sigmoid(LN(z) Wg + bg) * o) Wo + bo + z
        return (torch.sigmoid(_norm(t['z']) @ t['w1'] + t['b1']) * t['o']) @ t['w2'] + t['b2'] + t['z']
    return (_norm(t['x']) @ t['wo'] + t['bo']) * torch.sigmoid(_norm(t['z']) @ t['wg'] + t['bg']) + t['z']


def fold_ln(W, b, gamma, beta):
    """LayerNorm folded into the Linear (W (N, K)), float32 on the host: Wt' = gamma Wt (K, N), csum, bias' = beta Wt + b."""
    wt = W.double().t()
    wts = (gamma.double()[:, None] * wt).float().contiguous()
    return wts, wts.double().sum(0).float(), (beta.double() @ wt + b.double()).float()


@pytest.mark.parametrize('M', [1, 127, 128, 129])
@pytest.mark.parametrize('form', ['mlp1', 'mlp2', 'dual'])
def test_fused_form_row_edges(ops, form, M):
    ge = torch.Generator().manual_seed(7100 + M + 1000 * ('mlp1', 'mlp2', 'dual').index(form))
    rn = lambda *s: torch.randn(*s, generator=ge)
    K = 192
    t = {'z': rn(M, K) * 2 + 0.7}
    buf = scratch((M + 8) * K).view(M + 8, K)
    out = buf[:M]
    d = lambda v: v.to(DEV)
    zd = d(t['z'])
    ga, be = 1 + 0.1 * rn(K), 0.1 * rn(K)
    if form == 'dual':
        t['x'] = rn(M, 128)
        t['wo'], cso, t['bo'] = fold_ln(rn(192, 128) / 11, rn(192) * 0.1, 1 + 0.1 * rn(128), 0.1 * rn(128))
        t['wg'], csg, t['bg'] = fold_ln(rn(192, 192) / 14, rn(192) * 0.1, ga, be)
        xd = d(t['x']) if M % 4 else d(t['x'].t().contiguous()).t()        # channel-major product rows where M % 4 allows them
        wo, wg = d(t['wo']), d(t['wg'])
        ops.gemm(xd, wo, out, bias=d(t['bo']), ln=(None, d(cso)), B3=ops.split_weights(wo), resid=zd,
                 dual=(zd, ops.split_weights(wg), d(csg), d(t['bg'])), exact=2)
    else:
        NH = 768 if form == 'mlp1' else K
        t['w1'], cs1, t['b1'] = fold_ln(rn(NH, K) / K ** 0.5, 0.1 * rn(NH), ga, be)
        t['w2'], t['b2'] = (rn(K, NH) / NH ** 0.5).t().contiguous(), 0.1 * rn(K)
        w1, w23 = d(t['w1']), ops.split_weights(ops.permute_k16(d(t['w2'])))
        if form == 'mlp1':
            ops.gemm(zd, w1, out, bias=d(t['b1']), ln=(None, d(cs1)), B3=ops.split_weights(w1), act=1, resid=zd, exact=2, mlp=(w23, d(t['b2'])))
        else:
            t['o'] = rn(M, K) * 1.5
            ops.gemm(zd, w1, out, bias=d(t['b1']), ln=(None, d(cs1)), B3=ops.split_weights(w1), act=2, gate=d(t['o']), resid=zd, exact=2,
                     mlp=(w23, d(t['b2'])))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isnan(buf[M:]).all()), 'rows behind the last one were written'
    ref = fused_text(form, t, torch.float64)
    d32, d = (fused_text(form, t, torch.float32).double() - ref).abs(), (out.cpu().double() - ref).abs()
    e32, e = (float(d32.max()), float(d32.mean())), (float(d.max()), float(d.mean()))
    c = G.Case(f'fused-{form}-M{M}', M, K, K, 1, 'k', 'weights', 'plain', 2, frozenset(), frozenset(), 0, form, 'fused')
    assert_bound(c, e, e32, 'GEMM-FUSED')
