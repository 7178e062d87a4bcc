// ddqn_wavechain_wide.hip -- the DDQN inner loop of default_config_mountaincar.yaml (Critic_DQN 2-256-256-3 relu, batch 128, MountainCar-v0
// VirtualEnv with SE hidden 128 leakyrelu, ten lock-step test episodes) on a TEAM of G = 1, 2 or 4 workgroups per chain.  Same semantics,
// same canonical arithmetic order and therefore the same bits as the GEMM-queue kernel (dueling_se_inner_kernel<false, 2>, which stays the
// path for every other mode: tapes, traces, *_vary, ICM, RewardEnv, test_mode 1, kernel_variant NO_WAVECHAIN / GENERIC).
//
// The 128-wide wave-chain kernels keep a layer's weight matrix as one 64 KB LDS image; a 256 x 256 matrix is 256 KB and does not fit.  Here
// the A operand of every 256-deep product comes straight from the arena, 128-byte coalesced per half-wave, and the B operand from a
// [k][32 samples] LDS image of the activation block:
//   * forward (DDQN.learn agents/DDQN.py:60-94; models/actor_critic.py:84-91): wave w computes units 32 w .. 32 w + 31 of a 32-sample job
//     with v_mfma_f32_32x32x2_f32 over the K-MAJOR weight array Wt[k][unit]; the online pass runs s and s' of a block side by side (one
//     weight read, two chains); the target pass takes two blocks of s' at a time;
//   * backward: the input gradient d_h1 reads W2 through a NATURAL copy W2n[unit][k] of the online matrix (kept in step with the K-major
//     array by the optimizer epilogue), again coalesced; the weight gradient of W2 is 64 tiles of 32 x 32 over the team, their operands the
//     [sample][unit] rows of h1 / d_h2 in the arena, torch's Adam + the Polyak update as the tile epilogue;
//   * the output layer (3 units), layer 1 (K = 2) and the small gradients are VALU chains.
// Every output is ONE k-ascending fmaf chain from 0 (v_mfma_f32_32x32x2_f32 / 16x16x4 are bitwise such chains), the bias added last: the
// canonical order of oracle/lenv_oracle.h.
//
// Team: member g owns minibatch rows [g B / G, (g + 1) B / G) in the forward and backward passes and the gradient tiles 8 g / G .. of W2;
// three team barriers per learn step (head outputs exchanged; d_h1 / d_h2 rows complete; parameters updated).  Everything outside the learn
// step (SE step, greedy action, test episodes) runs redundantly on every member, as in dueling_wavechain.hip.
#include "lenv_wavechain.cuh"
#include "lenv_chain_frame.cuh"
#include "lenv_wavechain_host.h"
#include "lenv_host.h"

namespace lenv {

using namespace wc;

namespace ww {
constexpr int S = 2, A = 3, H = 256, B = 128, Hse = 128, T = 10, K = S + A;
constexpr int ACT = LENV_ACT_RELU, SE_ACT = LENV_ACT_LEAKYRELU, ENV = LENV_ENV_MOUNTAINCAR;
constexpr int JIMG = H * 32;                 // floats of one job's [unit][32 samples] image
// parameter vector (online, target, Adam m / v alike): W1t[S][H] b1 | W2t[H][H] (K-major) b2 | W3[A][H] (natural) b3 (+1 pad)
constexpr int oW1t = 0, ob1 = oW1t + S * H, oW2t = ob1 + H, ob2 = oW2t + H * H, oW3 = ob2 + H, ob3 = oW3 + A * H, PW = ob3 + 4;
constexpr int NPAR = ob3 + A;                // 67 331 = the Critic_DQN's parameters
constexpr int NSMALL = S * H + H + H + A * H + A;      // the parameters outside W2: gradients on the VALU
static_assert(PW % 4 == 0, "float4 alignment of the vectors");
// LDS carve-up (floats, every offset a multiple of 4)
constexpr int L_DSTATE = 0;                  // double [T][4]
constexpr int L_RET = L_DSTATE + 8 * T;      // double [T]
constexpr int L_IMG = 128;                   // two job images (the test phase: [H][16] x 2)
constexpr int L_W1T = L_IMG + 2 * JIMG, L_B1 = L_W1T + S * H, L_B2 = L_B1 + H, L_W3 = L_B2 + H, L_B3 = L_W3 + A * H;
constexpr int L_SEWOUT = L_B3 + 4, L_SEBOUT = L_SEWOUT + (S + 2) * Hse, L_SEH = L_SEBOUT + 16;
constexpr int L_XS = L_SEH + 3 * Hse, L_XS2 = L_XS + B * S, L_ACT = L_XS2 + B * S, L_REW = L_ACT + B, L_DONE = L_REW + B;
constexpr int L_QV = L_DONE + B, L_DQ = L_QV + 3 * B * A, L_MISC = L_DQ + B * A;
constexpr int L_EPREW = L_MISC + 64, L_ALIVE = L_EPREW + 16, L_TLEN = L_ALIVE + 16, L_STATE = L_TLEN + 16, L_NEWROW = L_STATE + 8;
constexpr int L_TQ = L_NEWROW + 16, L_XT = L_TQ + 16 * A, L_CTX = L_XT + 16 * S, L_END = L_CTX + 64;
static_assert(L_RET + 2 * T <= L_IMG && L_END * 4 <= 160 * 1024, "LDS layout");
}  // namespace ww

// the global side of a chain, written once into LDS by thread 0 (the phase routines are out of line and read it from there)
struct WwCtx {
    float *online, *target, *adam_m, *adam_v, *w2n, *h1d, *h2d, *dh2d, *dh1d, *qx;
    float w1, w2, beta2, adam_eps, tau, omt;
    int g, G, row0, nblk, max_steps;
};
static_assert(sizeof(WwCtx) <= 64 * 4, "context slot");

struct WwArgs {
    lenv_ddqn_cfg cfg;
    const float *theta, *eps; const int32_t *worker; const float *sign;
    const float *agent_init; const uint64_t *rng_keys;
    float *arena; int64_t arena_stride;
    lenv_inner_out out;
    int64_t rb_cap; int RS;
    int P, P_se, se_net_size[3];
    int64_t a_par, a_w2n, a_dump, a_qx, a_se, a_replay, a_meter, a_bar, a_ids;      // arena offsets (floats)
    int G;                                                                          // workgroups per chain: 1, 2 or 4
    int64_t chains;
};

extern __shared__ __align__(16) float ww_lds[];

// state-dict index (net.0.weight [H][S], net.0.bias, net.2.weight [H][H], net.2.bias, net.4.weight [A][H], net.4.bias) -> arena index
__device__ __forceinline__ int ww_sd_to_arena(int p)
{
    using namespace ww;
    int o = p;
    if (o < H * S) { const int j = o / S, k = o - j * S; return oW1t + k * H + j; }
    o -= H * S;
    if (o < H) return ob1 + o;
    o -= H;
    if (o < H * H) { const int j = o >> 8, k = o & (H - 1); return oW2t + k * H + j; }
    o -= H * H;
    if (o < H) return ob2 + o;
    o -= H;
    if (o < A * H) return oW3 + o;
    return ob3 + (o - A * H);
}

#define WW_PROLOGUE                                                                                                                        \
    using namespace ww;                                                                                                                    \
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = uni(tid >> 6), li = lane & 31, h = lane >> 5;                               \
    (void)lane; (void)wave; (void)li; (void)h;                                                                                            \
    lfloat *lb = (lfloat *)ww_lds;                                                                                                         \
    typedef __attribute__((address_space(3))) const WwCtx LCtx;                                                                            \
    LCtx *c = (LCtx *)(lb + L_CTX);                                                                                                        \
    float *online = uni_ptr(c->online), *target = uni_ptr(c->target), *adam_m = uni_ptr(c->adam_m), *adam_v = uni_ptr(c->adam_v),          \
          *w2n = uni_ptr(c->w2n), *h1d = uni_ptr(c->h1d), *h2d = uni_ptr(c->h2d), *dh2d = uni_ptr(c->dh2d), *dh1d = uni_ptr(c->dh1d),       \
          *qx = uni_ptr(c->qx);                                                                                                            \
    (void)online; (void)target; (void)adam_m; (void)adam_v; (void)w2n; (void)h1d; (void)h2d; (void)dh2d; (void)dh1d; (void)qx;            \
    lfloat *img0 = lb + L_IMG, *img1 = lb + L_IMG + JIMG;                                                                                  \
    lfloat *w1t_l = lb + L_W1T, *b1_l = lb + L_B1, *b2_l = lb + L_B2, *w3_l = lb + L_W3, *b3_l = lb + L_B3;                                \
    (void)img0; (void)img1; (void)w1t_l; (void)b1_l; (void)b2_l; (void)w3_l; (void)b3_l

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 acc) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0); }

// acc[j] += sum over the 128 k-steps of a 256-deep product: A lane (li, h) of step t = Ag[(2t + h) * 256 + li] (arena; the caller adds the
// wave's 32-column offset), B lane = img_j[(2t + h) * 32 + li] (an LDS [k][32] image).  The NJ chains share every A load.
template <int NJ>
__device__ __forceinline__ void ww_chain256(const float *Ag_, lfloat *const (&img)[2], int li, int h, f32x16 (&acc)[2])
{
    using namespace ww;
    const gfloat *a = (const gfloat *)Ag_ + h * H + li;
    const lfloat *b[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) b[j] = img[j] + h * 32 + li;
#pragma unroll 2
    for (int t0 = 0; t0 < 128; t0 += 16) {
        float av[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) av[u] = a[(t0 + u) * 2 * H];
#pragma unroll
        for (int u = 0; u < 16; ++u)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[j] = mfma32(av[u], b[j][(t0 + u) * 64], acc[j]);
    }
}

// ---- one forward group of the learn step.  pass 0: the TARGET net on s' of blocks blk, blk + 1 (slot 2); pass 1: the ONLINE net on s
// (slot 0; h1 / h2 rows to the arena for the backward pass) and s' (slot 1) of block blk.  Head outputs to the team's exchange rows qx ----
static __device__ __noinline__ void ww_forward(int pass_, int blk_)
{
    WW_PROLOGUE;
    const int pass = uni(pass_), blk = uni(blk_), nblk = uni(c->nblk), row0 = uni(c->row0);
    const float *par = pass ? online : target;
    const int nj = (pass || blk + 1 < nblk) ? 2 : 1;
    lfloat *xs_l = lb + L_XS, *xs2_l = lb + L_XS2;
    auto job_rows = [&](int j) { return row0 + 32 * (pass ? blk : blk + j); };
    for (int i = tid; i < S * H; i += NT) w1t_l[i] = par[oW1t + i];
    for (int i = tid; i < H; i += NT) { b1_l[i] = par[ob1 + i]; b2_l[i] = par[ob2 + i]; }
    for (int i = tid; i < A * H; i += NT) w3_l[i] = par[oW3 + i];
    if (tid < A) b3_l[tid] = par[ob3 + tid];
    __syncthreads();
    // layer 1 (K = S): one thread per (unit, sample) -> the job images [unit][32]; the stored job's rows once more unit-wise to the arena
    for (int e = tid; e < nj * JIMG; e += NT) {
        const int j = e / JIMG, r = e - j * JIMG, u = r >> 5, i = r & 31;
        const lfloat *X = (pass && j == 0) ? xs_l : xs2_l;
        const int row = job_rows(j) + i;
        float z = 0.0f;
#pragma unroll
        for (int k = 0; k < S; ++k) z = fma32(X[row * S + k], w1t_l[k * H + u], z);
        (j == 0 ? img0 : img1)[u * 32 + i] = act_fwd(ACT, 0.0f, z + b1_l[u]);
    }
    if (pass) {
        for (int e = tid; e < JIMG; e += NT) {
            const int u = e & (H - 1), i = e >> 8, row = job_rows(0) + i;
            float z = 0.0f;
#pragma unroll
            for (int k = 0; k < S; ++k) z = fma32(xs_l[row * S + k], w1t_l[k * H + u], z);
            ((gfloat *)h1d)[row * H + u] = act_fwd(ACT, 0.0f, z + b1_l[u]);
        }
    }
    __syncthreads();
    f32x16 acc[2];
#pragma unroll
    for (int v = 0; v < 16; ++v) { acc[0][v] = 0.0f; acc[1][v] = 0.0f; }
    lfloat *const imgs[2] = { img0, img1 };
    if (nj == 2) ww_chain256<2>(par + oW2t + 32 * wave, imgs, li, h, acc);
    else ww_chain256<1>(par + oW2t + 32 * wave, imgs, li, h, acc);
    __syncthreads();                                    // every wave is done with h1: the images take h2
    // D layout: lane (sample li, half h), register 4 g4 + cc -> unit 32 wave + 8 g4 + 4 h + cc
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j < nj) {
            lfloat *im = j == 0 ? img0 : img1;
            const bool store = pass && j == 0;
            const int row = job_rows(j) + li;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int u0 = 32 * wave + 8 * g4 + 4 * h;
                f32x4 o;
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    o[cc] = act_fwd(ACT, 0.0f, acc[j][4 * g4 + cc] + b2_l[u0 + cc]);
                    im[(u0 + cc) * 32 + li] = o[cc];
                }
                if (store) *(gf4 *)((gfloat *)h2d + row * H + u0) = o;
            }
        }
    }
    __syncthreads();
    // output layer: one thread per (job, sample, action), the 256-term chain over the h2 image
    if (tid < nj * 32 * A) {
        const int j = tid / (32 * A), r = tid - j * 32 * A, i = r / A, aa = r - i * A;
        const lfloat *im = (j == 0 ? img0 : img1) + i, *w = w3_l + aa * H;
        float q = 0.0f;
#pragma unroll 16
        for (int k = 0; k < H; ++k) q = fma32(im[k * 32], w[k], q);
        q = q + b3_l[aa];
        const int slot = pass ? j : 2;
        ((gfloat *)qx)[(slot * B + job_rows(j) + i) * A + aa] = q;
    }
    __syncthreads();
}

// ---- backward pass of blocks blk (, blk + 1) of this member's s rows: d_h2 (VALU: K = A) -> LDS images + arena rows; d_h1 = relu'(h1) *
// (W2^T d_h2) on the matrix pipe over the natural copy W2n -> arena rows ----
static __device__ __noinline__ void ww_backward(int blk_)
{
    WW_PROLOGUE;
    const int blk = uni(blk_), nblk = uni(c->nblk), row0 = uni(c->row0);
    const int nb = blk + 1 < nblk ? 2 : 1;
    const lfloat *dq_l = lb + L_DQ;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j < nb) {
            lfloat *im = j == 0 ? img0 : img1;
            const int row = row0 + 32 * (blk + j) + li;
            float da[A];
#pragma unroll
            for (int aa = 0; aa < A; ++aa) da[aa] = dq_l[row * A + aa];
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int u0 = 32 * wave + 4 * (h + 2 * q4);
                const f32x4 hv = *(const gf4 *)((const gfloat *)h2d + row * H + u0);
                f32x4 o;
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    float up = 0.0f;
#pragma unroll
                    for (int aa = 0; aa < A; ++aa) up = fma32(da[aa], ((const gfloat *)online)[oW3 + aa * H + u0 + cc], up);
                    o[cc] = act_bwd(ACT, 0.0f, hv[cc], up);
                    im[(u0 + cc) * 32 + li] = o[cc];
                }
                *(gf4 *)((gfloat *)dh2d + row * H + u0) = o;
            }
        }
    }
    __syncthreads();
    f32x16 acc[2];
#pragma unroll
    for (int v = 0; v < 16; ++v) { acc[0][v] = 0.0f; acc[1][v] = 0.0f; }
    lfloat *const imgs[2] = { img0, img1 };
    if (nb == 2) ww_chain256<2>(w2n + 32 * wave, imgs, li, h, acc);
    else ww_chain256<1>(w2n + 32 * wave, imgs, li, h, acc);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j < nb) {
            const int row = row0 + 32 * (blk + j) + li;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int u0 = 32 * wave + 8 * g4 + 4 * h;
                const f32x4 hv = *(const gf4 *)((const gfloat *)h1d + row * H + u0);
                f32x4 o;
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) o[cc] = act_bwd(ACT, 0.0f, hv[cc], acc[j][4 * g4 + cc]);
                *(gf4 *)((gfloat *)dh1d + row * H + u0) = o;
            }
        }
    }
    __syncthreads();
}

// ---- gradient tiles of W2 (gW2t[k][j] = sum_i h1[i][k] d_h2[i][j], i ascending) with torch's Adam + Polyak as the epilogue: N tiles
// (kt, jt0 .. jt0 + N - 1) per wave, the A operand shared ----
template <int N>
__device__ __forceinline__ void ww_wgrad_tiles(const float *h1d, const float *dh2d, float *online, float *target, float *adam_m, float *adam_v,
                                               float *w2n, int kt, int jt0, int li, int h, const AdamConsts ac, float tau, float omt)
{
    using namespace ww;
    f32x16 acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[j][v] = 0.0f;
    const gfloat *pa = (const gfloat *)h1d + h * H + 32 * kt + li, *pb = (const gfloat *)dh2d + h * H + 32 * jt0 + li;
#pragma unroll 1
    for (int t0 = 0; t0 < B / 2; t0 += 8) {
        float av[8], bv[N][8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            av[u] = pa[(t0 + u) * 2 * H];
#pragma unroll
            for (int j = 0; j < N; ++j) bv[j][u] = pb[(t0 + u) * 2 * H + 32 * j];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int j = 0; j < N; ++j) acc[j] = mfma32(av[u], bv[j][u], acc[j]);
    }
    // D layout: lane li -> column j = 32 jt + li, register 4 g4 + cc -> row k = 32 kt + 8 g4 + 4 h + cc
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int col = 32 * (jt0 + j) + li;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int k0 = 32 * kt + 8 * g4 + 4 * h;
            float w[4], m[4], v[4], t[4];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                const int off = oW2t + (k0 + cc) * H + col;
                w[cc] = ((gfloat *)online)[off]; m[cc] = ((gfloat *)adam_m)[off]; v[cc] = ((gfloat *)adam_v)[off]; t[cc] = ((gfloat *)target)[off];
            }
            f32x4 wn;
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                const int off = oW2t + (k0 + cc) * H + col;
                adam_elem(acc[j][4 * g4 + cc], m[cc], v[cc], w[cc], t[cc], ac, tau, omt);
                ((gfloat *)adam_m)[off] = m[cc]; ((gfloat *)adam_v)[off] = v[cc]; ((gfloat *)online)[off] = w[cc]; ((gfloat *)target)[off] = t[cc];
                wn[cc] = w[cc];
            }
            *(gf4 *)((gfloat *)w2n + col * H + k0) = wn;
        }
    }
}

// ---- the parameter update of a learn step, this member's share: its W2 tiles (64 / G) ----
static __device__ __noinline__ void ww_update()
{
    WW_PROLOGUE;
    const int G = uni(c->G), g = uni(c->g);
    volatile lfloat *ctrl = (volatile lfloat *)(lb + L_MISC);
    const AdamConsts ac{ ctrl[10], ctrl[11], unif(c->w1), unif(c->w2), unif(c->beta2), unif(c->adam_eps) };
    const float tau = unif(c->tau), omt = unif(c->omt);
    {
        // (one workgroup: the wave's eight tiles in two rounds of four -- eight accumulators and their operands do not fit the registers)
        const int n = 8 / G, s = g * 8 + wave, kt = (s * n) >> 3, jt0 = (s * n) & 7;
        if (n == 2) ww_wgrad_tiles<2>(h1d, dh2d, online, target, adam_m, adam_v, w2n, kt, jt0, li, h, ac, tau, omt);
        else
            for (int r = 0; r < n; r += 4) ww_wgrad_tiles<4>(h1d, dh2d, online, target, adam_m, adam_v, w2n, kt, jt0 + r, li, h, ac, tau, omt);
    }
}

// ... and its share of the small parameters (W1t, b1, b2, W3, b3: one thread per parameter, its gradient one i-ascending chain, then Adam + Polyak)
static __device__ __noinline__ void ww_update_small()
{
    WW_PROLOGUE;
    const int G = uni(c->G), g = uni(c->g);
    volatile lfloat *ctrl = (volatile lfloat *)(lb + L_MISC);
    const AdamConsts ac{ ctrl[10], ctrl[11], unif(c->w1), unif(c->w2), unif(c->beta2), unif(c->adam_eps) };
    const float tau = unif(c->tau), omt = unif(c->omt);
    const lfloat *xs_l = lb + L_XS, *dq_l = lb + L_DQ;
    for (int e = g * NT + tid; e < NSMALL; e += G * NT) {
        float s = 0.0f;
        int off;
        if (e < S * H + H) {                            // W1t[k][j] = sum_i d_h1[i][j] x[i][k]; b1[j] = sum_i d_h1[i][j]
            const bool bias = e >= S * H;
            const int k = e >> 8, j = e & (H - 1);
            const gfloat *d = (const gfloat *)dh1d + j;
#pragma unroll 1
            for (int i0 = 0; i0 < B; i0 += 32) {
                float dv[32];
#pragma unroll
                for (int u = 0; u < 32; ++u) dv[u] = d[(i0 + u) * H];
#pragma unroll
                for (int u = 0; u < 32; ++u) s = bias ? s + dv[u] : fma32(dv[u], xs_l[(i0 + u) * S + k], s);
            }
            off = bias ? ob1 + j : oW1t + e;
        } else if (e < S * H + 2 * H) {                 // b2[j] = sum_i d_h2[i][j]
            const int j = e - (S * H + H);
            const gfloat *d = (const gfloat *)dh2d + j;
#pragma unroll 1
            for (int i0 = 0; i0 < B; i0 += 32) {
                float dv[32];
#pragma unroll
                for (int u = 0; u < 32; ++u) dv[u] = d[(i0 + u) * H];
#pragma unroll
                for (int u = 0; u < 32; ++u) s = s + dv[u];
            }
            off = ob2 + j;
        } else if (e < S * H + 2 * H + A * H) {         // W3[a][k] = sum_i dQ[i][a] h2[i][k]
            const int r = e - (S * H + 2 * H), aa = r >> 8, k = r & (H - 1);
            const gfloat *hp = (const gfloat *)h2d + k;
#pragma unroll 1
            for (int i0 = 0; i0 < B; i0 += 32) {
                float hv[32];
#pragma unroll
                for (int u = 0; u < 32; ++u) hv[u] = hp[(i0 + u) * H];
#pragma unroll
                for (int u = 0; u < 32; ++u) s = fma32(dq_l[(i0 + u) * A + aa], hv[u], s);
            }
            off = oW3 + r;
        } else {                                        // b3[a] = sum_i dQ[i][a]
            const int aa = e - (S * H + 2 * H + A * H);
            for (int i = 0; i < B; ++i) s = s + dq_l[i * A + aa];
            off = ob3 + aa;
        }
        t3v_adam1(s, online, adam_m, adam_v, target, off, ac, tau, omt);
    }
}

// ---- thin products: I <= 16 rows through the ONLINE net.  Layer 2 on v_mfma_f32_16x16x4_f32: wave w computes units 32 w .. 32 w + 31 as
// two 16-unit tiles whose A operands (64 k-steps each) the caller holds in registers; activations in [unit][16] images ----
__device__ __forceinline__ void ww_thin_load(const float *online, int wave, int lane, float (&a0)[64], float (&a1)[64])
{
    using namespace ww;
    const gfloat *wa = (const gfloat *)online + oW2t + (lane >> 4) * H + 32 * wave + (lane & 15);
#pragma unroll
    for (int t = 0; t < 64; ++t) { a0[t] = wa[4 * t * H]; a1[t] = wa[4 * t * H + 16]; }
}
__device__ __forceinline__ void ww_thin_l2(const float (&a0)[64], const float (&a1)[64], const f32x4 bv0, const f32x4 bv1, const lfloat *in_img,
                                           lfloat *out_img, int wave, int lane)
{
    const int l16 = lane & 15, q = lane >> 4;
    const lfloat *xb = in_img + q * 16 + l16;
    f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < 64; ++t) {
        const float x = xb[4 * t * 16];
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[t], x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[t], x, acc1, 0, 0, 0);
    }
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
        out_img[(32 * wave + 4 * q + cc) * 16 + l16] = act_fwd(ww::ACT, 0.0f, acc0[cc] + bv0[cc]);
        out_img[(32 * wave + 16 + 4 * q + cc) * 16 + l16] = act_fwd(ww::ACT, 0.0f, acc1[cc] + bv1[cc]);
    }
}
__device__ __forceinline__ f32x4 ww_thin_bias(const float *online, int wave, int lane, int half)
{
    return *(const gf4 *)((const gfloat *)online + ww::ob2 + 32 * wave + 16 * half + 4 * (lane >> 4));
}

// greedy forward of I <= 16 rows (LDS rows L_XT) -> Q values at L_TQ
static __device__ __noinline__ void ww_thin(int I_)
{
    WW_PROLOGUE;
    const int I = uni(I_);
    float a0[64], a1[64];
    ww_thin_load(online, wave, lane, a0, a1);
    const f32x4 bv0 = ww_thin_bias(online, wave, lane, 0), bv1 = ww_thin_bias(online, wave, lane, 1);
    lfloat *imgX = img0, *imgY = img0 + 16 * H, *xt = lb + L_XT, *tq = lb + L_TQ;
    {
        const int j = tid & (H - 1);
        float w[S];
#pragma unroll
        for (int k = 0; k < S; ++k) w[k] = online[oW1t + k * H + j];
        const float bj = online[ob1 + j];
        for (int i = tid >> 8; i < 16; i += NT >> 8) {
            float z = 0.0f;
            if (i < I) {
#pragma unroll
                for (int k = 0; k < S; ++k) z = fma32(xt[i * S + k], w[k], z);
                z = act_fwd(ACT, 0.0f, z + bj);
            }
            imgX[j * 16 + i] = z;
        }
        for (int e = tid; e < A * H; e += NT) w3_l[e] = online[oW3 + e];
        if (tid < A) b3_l[tid] = online[ob3 + tid];
    }
    __syncthreads();
    ww_thin_l2(a0, a1, bv0, bv1, imgX, imgY, wave, lane);
    __syncthreads();
    if (tid < I * A) {
        const int i = tid / A, aa = tid - i * A;
        const lfloat *im = imgY + i, *w = w3_l + aa * H;
        float q = 0.0f;
#pragma unroll 16
        for (int k = 0; k < H; ++k) q = fma32(im[k * 16], w[k], q);
        tq[i * A + aa] = q + b3_l[aa];
    }
    __syncthreads();
}

// ---- the steps of one test phase (T episodes in lock-step, BaseAgent.test agents/base_agent.py:155-227) as one routine: the online net
// does not change during it, so every wave keeps its layer-2 A operands (128 registers) for all max_steps forwards ----
static __device__ __noinline__ void ww_test_steps(uint32_t key_lo_, uint32_t key_hi_, int first_episode_)
{
    WW_PROLOGUE;
    typedef __attribute__((address_space(3))) double ldouble;
    typedef __attribute__((address_space(3))) int lint;
    ldouble *dstate = (ldouble *)(lb + L_DSTATE), *ret = (ldouble *)(lb + L_RET);
    lfloat *ep_rew = lb + L_EPREW, *tq = lb + L_TQ, *Xl = lb + L_XT;
    lint *alive = (lint *)(lb + L_ALIVE), *tlen = (lint *)(lb + L_TLEN);
    const int max_steps = uni(c->max_steps);
    const uint64_t key = ((uint64_t)uni((int)key_hi_) << 32) | (uint32_t)uni((int)key_lo_);
    const int first_episode = uni(first_episode_);
    if (tid < T) {
        double st[4];
        real_env_reset_draw(ENV, key, STREAM_TEST_RESET, (int64_t)first_episode + tid, st);
#pragma unroll
        for (int i = 0; i < 4; ++i) dstate[tid * 4 + i] = st[i];
        ep_rew[tid] = 0.0f; alive[tid] = 1; tlen[tid] = 0;
    }
    float a0[64], a1[64];
    ww_thin_load(online, wave, lane, a0, a1);
    const f32x4 bv0 = ww_thin_bias(online, wave, lane, 0), bv1 = ww_thin_bias(online, wave, lane, 1);
    lfloat *imgX = img0, *imgY = img0 + 16 * H;
    const int j = tid & (H - 1);
    float w[S];
#pragma unroll
    for (int k = 0; k < S; ++k) w[k] = online[oW1t + k * H + j];
    const float bj = online[ob1 + j];
    for (int e = tid; e < A * H; e += NT) w3_l[e] = online[oW3 + e];
    if (tid < A) b3_l[tid] = online[ob3 + tid];
    auto put_obs = [&]() {
        double st[4] = { dstate[tid * 4], dstate[tid * 4 + 1], dstate[tid * 4 + 2], dstate[tid * 4 + 3] };
        float obs[8];
        real_env_obs(ENV, st, obs);
#pragma unroll
        for (int i = 0; i < S; ++i) Xl[tid * S + i] = obs[i];
    };
    if (tid < T) put_obs();
    __syncthreads();
    for (int t = 0; t < max_steps; ++t) {
        for (int i = tid >> 8; i < 16; i += NT >> 8) {
            float z = 0.0f;
            if (i < T) {
#pragma unroll
                for (int k = 0; k < S; ++k) z = fma32(Xl[i * S + k], w[k], z);
                z = act_fwd(ACT, 0.0f, z + bj);
            }
            imgX[j * 16 + i] = z;
        }
        __syncthreads();
        ww_thin_l2(a0, a1, bv0, bv1, imgX, imgY, wave, lane);
        __syncthreads();
        if (tid < T * A) {
            const int i = tid / A, aa = tid - i * A;
            const lfloat *im = imgY + i, *wv = w3_l + aa * H;
            float q = 0.0f;
#pragma unroll 16
            for (int k = 0; k < H; ++k) q = fma32(im[k * 16], wv[k], q);
            tq[i * A + aa] = q + b3_l[aa];
        }
        __syncthreads();
        if (tid < T && alive[tid]) {                      // greedy action on the Q values, env.step
            int am = 0;
            float best = tq[tid * A];
            for (int b = 1; b < A; ++b) { const float v = tq[tid * A + b]; if (v > best) { best = v; am = b; } }
            double st[4] = { dstate[tid * 4], dstate[tid * 4 + 1], dstate[tid * 4 + 2], dstate[tid * 4 + 3] };
            double rew; int dn;
            real_env_step(ENV, st, am, rew, dn);
#pragma unroll
            for (int i = 0; i < 4; ++i) dstate[tid * 4 + i] = st[i];
            ep_rew[tid] = ep_rew[tid] + (float)rew;
            tlen[tid] = tlen[tid] + 1;
            if (dn) alive[tid] = 0;
            put_obs();
        }
        __syncthreads();
        int any = 0;
        for (int e = 0; e < T; ++e) any |= alive[e];
        if (!any) break;
    }
    if (tid < T) ret[tid] = (double)ep_rew[tid];
    if (tid == 0) {
        int n = 0;
        for (int e = 0; e < T; ++e) n += tlen[e];
        ((lint *)(lb + L_MISC + 32))[0] = n;
    }
    __syncthreads();
}

__global__ __launch_bounds__(NT) void ddqn_wavechain_wide_kernel(const WwArgs a)
{
    using namespace ww;
    const lenv_ddqn_cfg &cfg = a.cfg;
    const int tid = (int)threadIdx.x;
    // a chain on a team of G workgroups: block x + 8 k is member k % G of chain 8 (k / G) + x, so the members share an XCD
    const int G = a.G;
    const int g = G == 1 ? 0 : (int)((blockIdx.x >> 3) % G);
    const int64_t chain = G == 1 ? (int64_t)blockIdx.x : (int64_t)8 * ((blockIdx.x >> 3) / G) + (blockIdx.x & 7);
    if (chain >= a.chains) return;
    if (threadIdx.x == 0 && g == 0 && a.out.status) a.out.status[chain] = 0;

    float *lds = ww_lds;
    typedef __attribute__((address_space(3))) double ldouble;
    ldouble *ret = (ldouble *)((lfloat *)lds + L_RET);
    lfloat *se_wout = (lfloat *)lds + L_SEWOUT, *se_bout = (lfloat *)lds + L_SEBOUT, *se_h = (lfloat *)lds + L_SEH;
    lfloat *xs_l = (lfloat *)lds + L_XS, *xs2_l = (lfloat *)lds + L_XS2, *act_l = (lfloat *)lds + L_ACT, *rew_l = (lfloat *)lds + L_REW,
           *done_l = (lfloat *)lds + L_DONE, *qv = (lfloat *)lds + L_QV, *dq = (lfloat *)lds + L_DQ, *misc = (lfloat *)lds + L_MISC,
           *state = (lfloat *)lds + L_STATE, *newrow = (lfloat *)lds + L_NEWROW, *tq = (lfloat *)lds + L_TQ, *xt = (lfloat *)lds + L_XT;
    typedef __attribute__((address_space(3))) int lint;
    lint *tlen = (lint *)((lfloat *)lds + L_TLEN);
    volatile lfloat *ctrl = (volatile lfloat *)misc;
    volatile lint *ictrl = (volatile lint *)(misc + 32);

    float *arena = a.arena + chain * a.arena_stride;
    float *online = arena + a.a_par, *target = online + PW, *adam_m = target + PW, *adam_v = adam_m + PW, *w2n = arena + a.a_w2n;
    float *dumps = arena + a.a_dump, *qx = arena + a.a_qx, *rb = arena + a.a_replay;
    float *se_w0T = arena + a.a_se, *se_b0 = se_w0T + 3 * K * Hse;
    double *meter = reinterpret_cast<double *>(arena + a.a_meter);
    unsigned *team_bar = reinterpret_cast<unsigned *>(arena + a.a_bar), *ids = reinterpret_cast<unsigned *>(arena + a.a_ids);
    const int RS = a.RS;

    // ---- stage the perturbed SE (GTN_worker.py:165-175): first layers transposed into the arena, output layers into LDS ----
    {
        const float sg = a.eps ? a.sign[chain] : 0.0f;
        const float *e = a.eps ? a.eps + (int64_t)a.worker[chain] * a.P_se : nullptr;
        for (int i = tid; i < a.P_se; i += NT) {
            const float w = e ? fma32(sg, e[i], a.theta[i]) : a.theta[i];
            int net = 0, r = i;
            if (r >= a.se_net_size[0]) { r -= a.se_net_size[0]; net = 1; if (r >= a.se_net_size[1]) { r -= a.se_net_size[1]; net = 2; } }
            const int orow = net == 0 ? 0 : (net == 1 ? S : S + 1);
            if (r < Hse * K) { int j = r / K, k = r - j * K; se_w0T[(net * K + k) * Hse + j] = w; }
            else if ((r -= Hse * K) < Hse) se_b0[net * Hse + r] = w;
            else {
                r -= Hse;
                const int n_out = net == 0 ? S : 1;
                if (r < n_out * Hse) { int o = r / Hse, j = r - o * Hse; se_wout[(orow + o) * Hse + j] = w; }
                else se_bout[orow + (r - n_out * Hse)] = w;
            }
        }
    }
    // ---- fresh agent (DDQN.py:31-36): arena layout + the natural copy of W2, Adam state cleared; the team's first member fills it ----
    if (g == 0) {
        for (int p = tid; p < PW; p += NT) { online[p] = 0.0f; target[p] = 0.0f; adam_m[p] = 0.0f; adam_v[p] = 0.0f; }
        __syncthreads();
        for (int p = tid; p < a.P; p += NT) {
            const float w = a.agent_init[chain * a.P + p];
            online[ww_sd_to_arena(p)] = w; target[ww_sd_to_arena(p)] = w;
            if (p >= H * S + H && p < H * S + H + H * H) w2n[p - (H * S + H)] = w;
        }
    }
    if (tid < 64) misc[tid] = 0.0f;
    const int R = B / G, nblk = R / 32;
    if (tid == 0) {
        WwCtx cx{ online, target, adam_m, adam_v, w2n, dumps, dumps + B * H, dumps + 2 * B * H, dumps + 3 * B * H, qx,
                  (float)(1.0 - cfg.adam_beta1), (float)(1.0 - cfg.adam_beta2), (float)cfg.adam_beta2, (float)cfg.adam_eps, (float)cfg.tau,
                  (float)(1.0 - cfg.tau), g, G, g * R, nblk, cfg.max_steps };
        *(WwCtx *)((float *)lds + L_CTX) = cx;
    }
    __syncthreads();

    const uint64_t key = a.rng_keys[chain];
    int status = 0;
    int train_steps = 0, n_act = 0, learn_it = 0, n_test_ep = 0, test_steps = 0, episodes_run = 0;
    double eps_g = cfg.eps_init, b1pow = 1.0, b2pow = 1.0;
    const int rb_cap = (int)a.rb_cap;
    TeamSync tsync{ team_bar, reinterpret_cast<unsigned *>(a.arena + a.a_bar) + 8, ictrl + 5, 0u, G, false, false };
    bool team_dead = false;
    // (G = 1: the waves hand each other rows through the arena: every wave's stores are acknowledged before the barrier)
    auto team_barrier = [&]() {
        if (G == 1) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads(); return; }
        wc::team_barrier<false>(tsync, tid);
        if (tsync.dead) { team_dead = true; status = -10; }
    };
    if (G > 1 && tid == 0) ids[g] = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 15u;      // HW_REG_XCC_ID[3:0]
    team_barrier();                                        // the arena is initialised, every member's XCD id is posted
    if (G > 1) {
        bool same = true;
        const unsigned x0 = ids[0];
        for (int m = 1; m < G; ++m) same = same && ids[m] == x0;
        tsync.same_xcd = same;
    }
    if (team_dead) {                                       // not all members became resident in time: nothing was computed
        if (a.out.status) atomicMin(&a.out.status[chain], -10);
        return;
    }

    // ---- real-env test phase: T episodes in lock-step ----
    auto test_phase = [&]() {
        __syncthreads();
        ww_test_steps((uint32_t)key, (uint32_t)(key >> 32), n_test_ep);
        n_test_ep += T;
        test_steps += ictrl[0];
        __syncthreads();
    };

    const bool budgeted = cfg.step_budget > 0;
    int timed_out_at = -1;
    for (int episode = 0; episode < cfg.train_episodes; ++episode) {
        if (budgeted && (int64_t)train_steps + test_steps > cfg.step_budget) { timed_out_at = episode; break; }
        if (episode == 0) eps_g = cfg.eps_init;
        else { eps_g *= cfg.eps_decay; if (eps_g < cfg.eps_min) eps_g = cfg.eps_min; }
        const bool learning = episode >= cfg.init_episodes;
        if (tid == 0) {
            double st0[4];
            real_env_reset_draw(ENV, key, STREAM_TRAIN_RESET, episode, st0);
            float obs[8];
            real_env_obs(ENV, st0, obs);
            for (int i = 0; i < S; ++i) state[i] = obs[i];
        }
        __syncthreads();
        int ep_len = 0;
        for (int t = 0; t < cfg.max_steps; ++t) {
            const int size_after = train_steps + 1 < rb_cap ? train_steps + 1 : rb_cap;
            const int new_pos = train_steps % rb_cap;
            if (tid == 0) {                                // select_train_action (DDQN.py:96-103)
                const double u = u64_to_unit(rng_u64(key, STREAM_EPS, (uint64_t)train_steps));
                int explored = u < eps_g, action = -1;
                if (explored) action = (int)u64_to_below(rng_u64(key, STREAM_ACTION, (uint64_t)n_act), (uint32_t)A);
                ictrl[1] = explored; ictrl[2] = action;
            }
            __syncthreads();
            const int explored = ictrl[1];
            if (explored) ++n_act;
            if (!explored) {
                if (tid < S) xt[tid] = state[tid];
                __syncthreads();
                ww_thin(1);
                if (tid == 0) {
                    int am = 0; float best = tq[0];
                    for (int aa = 1; aa < A; ++aa) if (tq[aa] > best) { best = tq[aa]; am = aa; }
                    ictrl[2] = am;
                }
                __syncthreads();
            }
            const int action = ictrl[2];
            // ---- EnvWrapper.step -> VirtualEnv.step: x = [onehot(action), state] ----
            for (int uu = tid; uu < 3 * Hse; uu += NT) {
                const int net = uu / Hse, j = uu - net * Hse;
                const float *w = se_w0T + net * K * Hse + j;
                float wk[K];
#pragma unroll
                for (int k = 0; k < K; ++k) wk[k] = w[k * Hse];
                float z = 0.0f;
#pragma unroll
                for (int k = 0; k < K; ++k) z = fma32(k < A ? (k == action ? 1.0f : 0.0f) : state[k - A], wk[k], z);
                z = z + se_b0[uu];
                se_h[uu] = act_fwd(SE_ACT, cfg.se_prelu, z);
            }
            __syncthreads();
            if (tid < S + 2) {
                const int net = tid < S ? 0 : (tid == S ? 1 : 2);
                const lfloat *hh = se_h + net * Hse, *w = se_wout + tid * Hse;
                float acc = 0.0f;
                for (int j = 0; j < Hse; ++j) acc = fma32(hh[j], w[j], acc);
                acc = acc + se_bout[tid];
                if (tid < S) newrow[S + 1 + tid] = acc; else newrow[2 * S + 1 + (tid - S)] = acc;
            }
            if (tid >= 64 && tid < 64 + S) newrow[tid - 64] = state[tid - 64];
            if (tid == 128) newrow[S] = (float)action;
            __syncthreads();
            if (tid < 2 * S + 3) rb[(int64_t)new_pos * RS + tid] = newrow[tid];
            const float done_now = newrow[2 * S + 2];
            __syncthreads();
            if (tid < S) state[tid] = newrow[S + 1 + tid];
            ++ep_len; ++train_steps;
            __syncthreads();

            if (learning) {
                // ================= DDQN.learn (DDQN.py:60-94) =================
                for (int b = tid; b < B; b += NT) {
                    const int64_t n = (int64_t)learn_it * B + b;
                    const int idx = (int)rng_replay_below(key, (uint64_t)n, (uint32_t)size_after);
                    const float *row = rb + (int64_t)idx * RS;
                    float rv[2 * S + 3];
#pragma unroll
                    for (int i = 0; i < 2 * S + 3; ++i) rv[i] = row[i];
#pragma unroll
                    for (int i = 0; i < S; ++i) { xs_l[b * S + i] = rv[i]; xs2_l[b * S + i] = rv[S + 1 + i]; }
                    act_l[b] = rv[S]; rew_l[b] = rv[2 * S + 1]; done_l[b] = rv[2 * S + 2];
                }
                __syncthreads();
                for (int blk = 0; blk < nblk; blk += 2) ww_forward(0, blk);     // target net on s'
                for (int blk = 0; blk < nblk; ++blk) ww_forward(1, blk);        // online net on s and s'
                team_barrier();                            // every row's Q values are in the exchange rows
                for (int e = tid; e < 3 * B * A; e += NT) qv[e] = qx[e];
                __syncthreads();
                for (int b = tid; b < B; b += NT) {        // TD error (DDQN.py:80-85)
                    const float g32 = (float)cfg.gamma, norm = (float)(2.0 / (double)B);
                    const int ab = (int)act_l[b];
                    const float rr = rew_l[b], d = done_l[b];
                    int am = 0; float best = qv[(B + b) * A];
                    for (int aa = 1; aa < A; ++aa) { const float v = qv[(B + b) * A + aa]; if (v > best) { best = v; am = aa; } }
                    const float t1 = g32 * qv[(2 * B + b) * A + am];
                    const float t2 = 1.0f - d;
                    const float y = rr + t1 * t2;
                    const float dqb = norm * (qv[b * A + ab] - y);
                    for (int aa = 0; aa < A; ++aa) dq[b * A + aa] = aa == ab ? dqb : 0.0f;
                }
                if (tid == 0) {
                    b1pow *= cfg.adam_beta1; b2pow *= cfg.adam_beta2;
                    ctrl[10] = (float)(-(cfg.lr / (1.0 - b1pow)));
                    ctrl[11] = (float)__builtin_sqrt(1.0 - b2pow);
                }
                __syncthreads();
                for (int blk = 0; blk < nblk; blk += 2) ww_backward(blk);
                team_barrier();                            // all rows of h1 / h2 / d_h2 / d_h1 are in the arena
                ww_update();
                ww_update_small();
                team_barrier();                            // the parameters are updated everywhere
                ++learn_it;
                if (team_dead) break;
            }
            if (done_now > 0.5f) break;
        }
        ++episodes_run;
        if (team_dead) break;
        if (tid == 0 && g == 0 && a.out.episode_len) a.out.episode_len[chain * cfg.train_episodes + episode] = ep_len;
        __syncthreads();
        test_phase();
        if (tid == 0) {
            double sm = 0.0;
            for (int i = 0; i < T; ++i) sm += ret[i];
            const double tm = sm / (double)T;
            meter[episode] = tm;
            if (g == 0 && a.out.episode_test_mean) a.out.episode_test_mean[chain * cfg.train_episodes + episode] = tm;
            int brk = 0;
            if (learning) {
                int lo = episode + 1 - cfg.early_out_num; if (lo < 0) lo = 0;
                double s2 = 0.0;
                for (int i = lo; i <= episode; ++i) s2 += meter[i];
                if (s2 / ((double)(episode + 1 - lo) + 1e-9) >= cfg.solved_reward) brk = 1;
            }
            ictrl[3] = brk;
        }
        __syncthreads();
        const int brk = ictrl[3];
        __syncthreads();
        if (brk) break;
    }
    const int64_t remaining = cfg.step_budget - ((int64_t)train_steps + test_steps);
    const int test_before = test_steps;
    if (!team_dead) test_phase();
    if (budgeted) {
        if (tid == 0) {                                   // thread 0 counts and pads, ictrl[4] carries `used` to the others
            const BudgetCut cut = chain_budget_cut(tlen, T, remaining);
            chain_pad_returns(ret, cut.stop, T);
            ictrl[4] = (int)cut.used;
        }
        __syncthreads();
        test_steps = test_before + ictrl[4];
    }
    if (tid == 0 && g == 0)
        chain_close(a.out, chain, T, ret, meter, cfg.train_episodes, episodes_run, train_steps, learn_it, test_steps, timed_out_at);
    if (a.out.final_online && g == 0)
        for (int p = tid; p < a.P; p += NT) a.out.final_online[chain * a.P + p] = online[ww_sd_to_arena(p)];
    if (a.out.status && status != 0) atomicMin(&a.out.status[chain], status);
}

}  // namespace lenv

using namespace lenv;

// Host side (declared in lenv_wavechain_host.h), called by lenv_dueling_se_inner_loop_icm (dueling_se_inner_loop.hip).
// 1 when `cfg` is default_config_mountaincar.yaml's DDQN in the mode this kernel covers (the caller checks the launch mode: counter RNG, no
// trace, no per-chain hyper-parameters, same_action_num <= 1)
int lenv_wc_ddqn_wide_shape(const lenv_ddqn_cfg *cfg)
{
    using namespace ww;
    return cfg->agent_kind == 0 && cfg->env_id == ENV && cfg->state_dim == S && cfg->num_actions == A && cfg->q_hidden == H && cfg->q_layers == 2 &&
           cfg->batch_size == B && cfg->q_act == ACT && cfg->se_hidden == Hse && cfg->se_layers == 1 && cfg->se_act == SE_ACT && !cfg->se_layer_norm &&
           !cfg->q_layer_norm && cfg->test_episodes == T && cfg->synthetic_env_type == 0 && cfg->test_mode == 0 && !cfg->icm_enabled;
}

// one chain's arena: places the buffers in `a`, returns its floats
static int64_t ww_offsets(const lenv_ddqn_cfg *cfg, int64_t rb_cap, int RS, WwArgs &a)
{
    using namespace ww;
    lenv_host::ArenaCursor c;
    a.a_par = c.take(4 * (int64_t)PW); a.a_w2n = c.take((int64_t)H * H); a.a_dump = c.take(4 * (int64_t)B * H); a.a_qx = c.take(3 * (int64_t)B * A);
    a.a_se = c.take(3 * (int64_t)(K + 1) * Hse); a.a_replay = c.take(rb_cap * RS);
    a.a_meter = c.take(2 * (int64_t)(cfg->train_episodes > 0 ? cfg->train_episodes : 1));
    a.a_bar = c.take(16); a.a_ids = c.take(16);
    return c.total();
}

int64_t lenv_wc_ddqn_wide_arena_floats(const lenv_ddqn_cfg *cfg, int64_t rb_cap, int RS)
{
    WwArgs a;
    return ww_offsets(cfg, rb_cap, RS, a);
}

static size_t ww_lds_bytes() { return (size_t)ww::L_END * sizeof(float); }

// Workgroups per chain: the largest of 4 and 2 for which all 8 * ceil(chains / 8) * G workgroups are resident at once (occupancy API: one
// per CU at this kernel's LDS footprint), else 1.  cfg->team_size caps the choice (0 = automatic, 1 = the plain launch).
int lenv_wc_ddqn_wide_team(const lenv_ddqn_cfg *cfg, int64_t chains)
{
    return lenv_host::pick_team({ 4, 2 }, cfg->team_size, 0, chains, reinterpret_cast<const void *>(ddqn_wavechain_wide_kernel), NT, ww_lds_bytes());
}

int lenv_wc_ddqn_wide_launch(const lenv_ddqn_cfg *cfg, const float *theta, const float *eps, const int32_t *worker, const float *sign,
                             const float *agent_init, const uint64_t *rng_keys, int64_t chains, float *arena, int64_t arena_stride, int64_t rb_cap,
                             int RS, int P, int P_se, const int *se_net_size, const lenv_inner_out *out, hipStream_t stream)
{
    WwArgs a;
    a.cfg = *cfg;
    lenv_host::fill_population(a, theta, eps, worker, sign, agent_init, rng_keys);
    a.arena = arena; a.arena_stride = arena_stride; a.out = *out; a.rb_cap = rb_cap; a.RS = RS; a.P = P; a.P_se = P_se;
    for (int i = 0; i < 3; ++i) a.se_net_size[i] = se_net_size[i];
    if (P != ww::NPAR || RS < 2 * ww::S + 3) return LENV_ERR_UNSUPPORTED;
    if (ww_offsets(cfg, rb_cap, RS, a) > arena_stride) return LENV_ERR_WORKSPACE;
    a.chains = chains;
    a.G = lenv_wc_ddqn_wide_team(cfg, chains);
    return lenv_host::launch_team(ddqn_wavechain_wide_kernel, NT, ww_lds_bytes(), stream, a);
}
