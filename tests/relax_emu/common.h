// Host stand-in for abx_amd/csrc/common.h (see hip/hip_runtime.h beside it): the helpers relax.hip uses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#define ABX_OK 0
#define ABX_ERR_ARG (-1)
#define ABX_LDS_LIMIT 163840
inline void abx_set_error(const char* m) { fprintf(stderr, "abx_relax (host emulation): %s\n", m); }
inline int abx_check_launch(const char*) { return 0; }
inline int abx_ensure_dynamic_lds(const void*, int, const char*) { return 0; }
#define ABX_REQUIRE(cond, msg) do { if (!(cond)) { abx_set_error(msg); return ABX_ERR_ARG; } } while (0)
inline float wave_sum(float v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64); return v; }
inline float wave_max(float v) { for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64)); return v; }
inline double wave_sum_d(double v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64); return v; }
