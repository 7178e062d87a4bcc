// lenv_at_layer.cuh -- the forward item of the test-population kernels (agent_test_population.hip, actor_test_population.hip): one Linear layer
// for the episodes of a workgroup that advance in lock-step, and the k-major staging of a weight matrix in LDS.
#pragma once

#include "lenv_gemm.cuh"

namespace lenv {

constexpr int AT_EPT = 4;                      // episodes of one forward item

// y[e][j] = (act)(sum_k x[e][k] * W[j][k] + b[j]) for the episodes e < rows of the block, j < n_out.  ST: W is the staged, transposed copy
// (element (j, k) at k * n_out + j), else the row-major matrix in global memory.  Groups without a live episode are skipped.  The caller
// synchronises.
template <bool ST>
__device__ __forceinline__ void at_layer(const float *W, const float *b, int n_in, int n_out, const float *x, int ldx, float *y, int ldy, int rows,
                                         bool activate, int act, float prelu, unsigned alive, int tid)
{
    const int groups = (rows + AT_EPT - 1) / AT_EPT;
    const bool xv4 = (ldx & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    const bool wv4 = !ST && (n_in & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0;
    for (int it = tid; it < groups * n_out; it += DNT) {
        const int g = it / n_out, j = it - g * n_out, e0 = g * AT_EPT;
        if (((alive >> e0) & ((1u << AT_EPT) - 1)) == 0) continue;
        const float *xr[AT_EPT];
        float z[AT_EPT];
#pragma unroll
        for (int u = 0; u < AT_EPT; ++u) { const int e = e0 + u < rows ? e0 + u : rows - 1; xr[u] = x + e * ldx; z[u] = 0.0f; }
        const float *wj = ST ? W + j : W + (int64_t)j * n_in;
        int k = 0;
        for (; k + 4 <= n_in; k += 4) {
            float w[4];
            if (ST) {
#pragma unroll
                for (int q = 0; q < 4; ++q) w[q] = wj[(k + q) * n_out];
            } else if (wv4) {
                const float4 t = *reinterpret_cast<const float4 *>(wj + k);
                w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) w[q] = wj[k + q];
            }
#pragma unroll
            for (int u = 0; u < AT_EPT; ++u) {
                float xv[4];
                if (xv4) {
                    const float4 t = *reinterpret_cast<const float4 *>(xr[u] + k);
                    xv[0] = t.x; xv[1] = t.y; xv[2] = t.z; xv[3] = t.w;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) xv[q] = xr[u][k + q];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) z[u] = fma32(xv[q], w[q], z[u]);
            }
        }
        for (; k < n_in; ++k) {
            const float w = ST ? wj[k * n_out] : wj[k];
#pragma unroll
            for (int u = 0; u < AT_EPT; ++u) z[u] = fma32(xr[u][k], w, z[u]);
        }
        const float bj = b[j];
#pragma unroll
        for (int u = 0; u < AT_EPT; ++u) {
            if (e0 + u >= rows) break;
            const float v = z[u] + bj;
            y[(e0 + u) * ldy + j] = activate ? act_fwd(act, prelu, v) : v;
        }
    }
}

// the staged copy of one weight matrix [n_out][n_in]: transposed in place of the row-major one
__device__ __forceinline__ void at_stage_transposed(float *dst, const float *src, int n_out, int n_in, int tid)
{
    for (int i = tid; i < n_out * n_in; i += DNT) { const int j = i / n_in, k = i - j * n_in; dst[k * n_out + j] = src[i]; }
}

}  // namespace lenv
