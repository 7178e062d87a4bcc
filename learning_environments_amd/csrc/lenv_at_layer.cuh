// lenv_at_layer.cuh -- what the test-population kernels (agent_test_population.hip, actor_test_population.hip,
// discrete_actor_test_population.hip) share: the episodes of a workgroup and their alive mask, the staging of an MLP's parameters in LDS (the
// dynamic-LDS layout itself is lenv_tp_layout.h, which the host's launch plan reads too), one Linear layer for the episodes of a workgroup that
// advance in lock-step, and the hidden layers of an MLP on top of it.
#pragma once

#include "lenv_gemm.cuh"
#include "lenv_ln.cuh"
#include "lenv_tp_layout.h"

namespace lenv {

constexpr int AT_EPT = 4;                      // episodes of one forward item

// Grid (agent, block of at most TP_TB episodes): the block's first episode, its episodes, and the episodes of the launch's fullest block.
struct TpBlock { int ep0, rows, rows_max; };
__device__ __forceinline__ TpBlock tp_block(int T)
{
    const int ep0 = blockIdx.y * TP_TB;
    return TpBlock{ ep0, T - ep0 < TP_TB ? T - ep0 : TP_TB, T < TP_TB ? T : TP_TB };
}

// Bit e of the mask: episode e of the block still runs.  Thread e retires its own episode; behind the barrier of tp_all_retired every thread
// reads the same word, so the break it decides is uniform (the next write to the mask comes behind further barriers).
__device__ __forceinline__ void tp_alive_init(unsigned *alive_mask, int rows, int tid) { if (tid == 0) *alive_mask = (1u << rows) - 1u; }   // rows <= TP_TB
__device__ __forceinline__ void tp_retire(unsigned *alive_mask, int tid) { atomicAnd(alive_mask, ~(1u << tid)); }
__device__ __forceinline__ bool tp_all_retired(const unsigned *alive_mask) { __syncthreads(); return *alive_mask == 0; }

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

// The staged copy of an MLP: the P floats as they are (biases, LayerNorm, and the matrices' places), then every matrix transposed -- the L
// trunk matrices (n_in -> H, then H -> H) and the last one [n_last][H] -- at their offsets oW[0..L].  Further matrices are the caller's.
__device__ __forceinline__ void tp_stage_mlp(float *wst, const float *gpar, int P, const int *oW, int L, int n_in, int H, int n_last, int tid)
{
    for (int p = tid; p < P; p += DNT) wst[p] = gpar[p];
    __syncthreads();
    for (int l = 0; l < L; ++l) { at_stage_transposed(wst + oW[l], gpar + oW[l], H, n_in, tid); n_in = H; }
    at_stage_transposed(wst + oW[L], gpar + oW[L], n_last, H, tid);
}

// The L hidden layers on the block's rows x [rows][ldx]: Linear + activation, from the second layer on with the shared LayerNorm (weight |
// bias at oLN) in between where ln.  Layer l writes buf0 / buf1 in turn; returns the last activation and its row stride (ln_rows_forward
// takes dense rows).  Ends behind a barrier.  LNBUF: the chunk of ln_rows_forward, every row of a block in one.
struct TpAct { const float *x; int ld; };
template <bool ST, int LNBUF>
__device__ __forceinline__ TpAct tp_trunk(const float *par, const int *oW, const int *ob, int oLN, int L, int H, bool ln, const float *x, int n_in, int ldx,
                                          float *buf0, float *buf1, float *lnbuf, int rows, int act, float prelu, unsigned alive, int tid)
{
    const int ldh = ln ? H : (H + 3) & ~3;
    for (int l = 0; l < L; ++l) {
        float *out = (l & 1) ? buf1 : buf0;
        const bool at_ln = ln && l >= 1;
        at_layer<ST>(par + oW[l], par + ob[l], n_in, H, x, ldx, out, ldh, rows, !at_ln, act, prelu, alive, tid);
        __syncthreads();
        if (at_ln) ln_rows_forward<LNBUF>(lnbuf, out, rows, H, par + oLN, par + oLN + H, nullptr, nullptr, act, prelu);
        x = out; n_in = H; ldx = ldh;
    }
    return TpAct{ x, ldx };
}

}  // namespace lenv
