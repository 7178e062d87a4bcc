// lenv_tp_layout.h -- the constants and the dynamic-LDS layout of the test-population entries, for the kernels (lenv_at_layer.cuh) and for the
// host's launch plan (lenv_host.h): one formula for both, and nothing else in here.
#pragma once

#include <hip/hip_runtime.h>

namespace lenv {

constexpr int TP_TB = 16;                      // episodes of one workgroup
constexpr int TP_MAX_REPEAT = 64;              // the largest same_action_num

// Dynamic LDS in floats: two activation buffers [rows_max][W] (`act` floats each) | with the shared LayerNorm [rows_max][H | 1] for
// ln_rows_forward (`ln` floats) | the staged parameters of a staged launch.  A kernel chains its pointers from the two sizes
// (buf1 = lds + act, lnbuf = buf1 + act, wst = lnbuf + ln): handed back as a struct of pointers they cost the staged kernels the 2x unroll
// of at_layer's k-loop (docs/notebook_test_population_refactor.md).
struct TpLds { int act, ln; };
__host__ __device__ __forceinline__ TpLds tp_lds_layout(int rows_max, int W, bool ln, int H) { return TpLds{ rows_max * W, ln ? rows_max * (H | 1) : 0 }; }

}  // namespace lenv
