// se_step_vec.hip -- population-batched VirtualEnv step for ACTION VECTORS (continuous action spaces: the Pendulum / MountainCarContinuous /
// HalfCheetah SEs; a one-hot row is an action vector too) with the `same_action_num` repeat of EnvWrapper.step's virtual branch
// (envs/env_wrapper.py:28-30) inside the launch.  Workgroup c steps the SE W_c = theta + sign[c]*eps[worker[c]] on its n_per_chain rows.
//
// One kernel body, two instantiations behind one entry (lenv_se_step_vec_path says which):
//   resident  -- W_c fits the 160 KiB of LDS next to the buffers of one block of rows: staged once (the structure of se_step_kernel,
//                se_step.hip), then n_per_chain x repeat evaluations;
//   streaming -- it does not (the published HalfCheetah SE: 110 739 floats): every layer of the three nets passes through LDS in K-panels
//                of KP input columns, and ALL rows of a row block are evaluated against the staged panel, so a weight leaves HBM once per
//                chain, repeat and row block instead of once per row.  A unit's running sum is parked in its output slot between panels:
//                k stays ascending.
// Both stage with 16-byte global loads of theta and of the chain's noise row and perturb on the way in.  A stage (a hidden layer of the
// three nets side by side, or their output layers) lies in LDS unit-major with a row stride of 4 * odd floats; a thread owns one unit and
// a tile of SV_RT rows, reads four weights of its unit (one conflict-free ds_read_b128) and four inputs of each row (broadcast reads).
// Arithmetic: the canonical order of mlp_forward.hip / oracle/lenv_oracle.h (acc = 0, fma over ascending k, + bias, activation; LayerNorm
// sums in index order), so both instantiations give the oracle's bits.
#include "lenv_device.cuh"

namespace lenv {

constexpr int SV_NT = 512;
constexpr int SV_RT = 8;            // rows per register tile
constexpr int SV_SB = 4;            // staging: 16-byte loads in flight per thread and operand
constexpr int SV_MAX_HIDDEN = 256, SV_MAX_LAYERS = 3, SV_MAX_IN = 256;
constexpr size_t SV_LDS_BYTES = 160 * 1024;

struct SvArgs {
    lenv_mlp_desc net[3];
    int64_t net_off[3];      // parameter offset of each net inside theta
    int64_t P;               // total parameters
    const float *theta, *eps; const int32_t *worker; const float *sign;
    int32_t n_per_chain, repeat;
    const float *state, *action;
    float *next_state, *reward, *done;
    int S, A;
    int KP, RB;              // input columns per panel (a multiple of 8; streaming only), rows per row block (a multiple of SV_RT)
    int wfloats;             // floats of LDS in front of the row buffers: every stage (resident) / one panel (streaming)
};

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));      // a 16-byte global load that needs only dword alignment

// row stride of a staged block of n columns: 4 * odd floats, so that the 16 lanes a ds_read_b128 serves per cycle (16 units, the same
// column quad) fall on 16 distinct bank quads
__host__ __device__ __forceinline__ int sv_row_stride(int n) { return ((n + 7) & ~7) + 4; }

// element i of W_c
__device__ __forceinline__ float sv_w(const SvArgs &a, const float *e, float sg, int64_t i) { return e ? fma32(sg, e[i], a.theta[i]) : a.theta[i]; }

// v[net] of three values kept in registers (a runtime-indexed local array would live in scratch memory)
template <typename T> __device__ __forceinline__ T sv_pick(int net, T v0, T v1, T v2) { return net == 0 ? v0 : (net == 1 ? v1 : v2); }

// what a stage (hidden layer l < L, or the output layer l == L) is to unit u of the three nets side by side: its net, its unit there, where
// its result goes in a row of the activation buffer and where its net's inputs start in one
struct SvUnit { int net, j, opos, ibase; };
__device__ __forceinline__ SvUnit sv_unit(bool out_stage, bool first, int u, int H, int Hp, int S)
{
    SvUnit r;
    if (!out_stage) { r.net = u / H; r.j = u - r.net * H; r.opos = r.net * Hp + r.j; }
    else { r.net = u < S ? 0 : (u == S ? 1 : 2); r.j = u < S ? u : 0; r.opos = u; }
    r.ibase = first ? 0 : r.net * Hp;
    return r;
}

// the walk through the stages of the three nets: per net the offset of the stage's weights in theta (the bias follows them) and of the
// net's shared LayerNorm weight | bias (behind its second Linear's bias: se_step.hip), and the stage's input width
struct SvWalk {
    int64_t w0, w1, w2, ln0, ln1, ln2;
    int n_in;
    __device__ __forceinline__ void begin(const SvArgs &a) { w0 = a.net_off[0]; w1 = a.net_off[1]; w2 = a.net_off[2]; ln0 = ln1 = ln2 = 0; n_in = a.S + a.A; }
    __device__ __forceinline__ void past_hidden(int l, int H, int ln_mask)
    {
        const int64_t step = (int64_t)H * n_in + H;
        w0 += step; w1 += step; w2 += step;
        if (l == 1) {
            if (ln_mask & 1) { ln0 = w0; w0 += 2 * H; }
            if (ln_mask & 2) { ln1 = w1; w1 += 2 * H; }
            if (ln_mask & 4) { ln2 = w2; w2 += 2 * H; }
        }
        n_in = H;
    }
};

// columns [k0, k0 + kp) of a stage's U weight rows -> pan[u][PS], perturbed: the whole quads of every row as 16-byte loads (quads of a row on
// consecutive lanes), then the 0..3 words a row has left one by one.  Branch-free rounds of SV_SB requests per thread and operand (a thread
// past the end repeats the last item), so that all of a round's loads are in flight before the first is used.
template <bool NOISE>
__device__ __forceinline__ void sv_stage_panel(const SvArgs &a, const float *e, float sg, float *pan, int PS, bool out_stage, bool first, int U, int H,
                                               int Hp, const SvWalk &wk, int k0, int kp, int tid)
{
    const int Q = kp >> 2, R = kp & 3;
    for (int t0 = tid; t0 < U * Q; t0 += SV_SB * SV_NT) {
        f4u tw[SV_SB], nw[SV_SB];
        float *dst[SV_SB];
#pragma unroll
        for (int b = 0; b < SV_SB; ++b) {
            const int t = t0 + b * SV_NT < U * Q ? t0 + b * SV_NT : U * Q - 1;
            const int u = t / Q, q = t - u * Q;
            const SvUnit un = sv_unit(out_stage, first, u, H, Hp, a.S);
            const int64_t g = sv_pick(un.net, wk.w0, wk.w1, wk.w2) + (int64_t)un.j * wk.n_in + k0 + 4 * q;
            dst[b] = pan + (size_t)u * PS + 4 * q;
            tw[b] = *reinterpret_cast<const f4u *>(a.theta + g);
            if (NOISE) nw[b] = *reinterpret_cast<const f4u *>(e + g);
        }
#pragma unroll
        for (int b = 0; b < SV_SB; ++b) {
            f4u w = tw[b];
            if (NOISE) { w.x = fma32(sg, nw[b].x, w.x); w.y = fma32(sg, nw[b].y, w.y); w.z = fma32(sg, nw[b].z, w.z); w.w = fma32(sg, nw[b].w, w.w); }
            *reinterpret_cast<float4 *>(dst[b]) = make_float4(w.x, w.y, w.z, w.w);
        }
    }
    for (int t0 = tid; t0 < U * R; t0 += SV_SB * SV_NT) {
        float tw[SV_SB], nw[SV_SB];
        float *dst[SV_SB];
#pragma unroll
        for (int b = 0; b < SV_SB; ++b) {
            const int t = t0 + b * SV_NT < U * R ? t0 + b * SV_NT : U * R - 1;
            const int u = t / R, k = 4 * Q + (t - u * R);
            const SvUnit un = sv_unit(out_stage, first, u, H, Hp, a.S);
            const int64_t g = sv_pick(un.net, wk.w0, wk.w1, wk.w2) + (int64_t)un.j * wk.n_in + k0 + k;
            dst[b] = pan + (size_t)u * PS + k;
            tw[b] = a.theta[g];
            if (NOISE) nw[b] = e[g];
        }
#pragma unroll
        for (int b = 0; b < SV_SB; ++b) *dst[b] = NOISE ? fma32(sg, nw[b], tw[b]) : tw[b];
    }
}

template <bool STREAM>
__global__ __launch_bounds__(SV_NT) void se_step_vec_kernel(const SvArgs a)
{
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x;
    const int64_t chain = blockIdx.x;
    const int H = a.net[0].hidden, L = a.net[0].layers, K = a.S + a.A, S = a.S;
    const int Hp = (H + 3) & ~3, Kp = (K + 3) & ~3;
    const int n_outs = S + 2;
    const int Wd = 3 * Hp > ((n_outs + 3) & ~3) ? 3 * Hp : ((n_outs + 3) & ~3);      // floats per row of an activation buffer
    const int RB = a.RB;
    float *wl = lds;                                 // resident: stage after stage [U][sv_row_stride(n_in)]; streaming: one panel [U][KP + 4]
    float *x = lds + a.wfloats;                      // [RB][Kp] action | state, zero beyond K and beyond the block's rows
    float *h0 = x + RB * Kp;                         // [RB][Wd] ping: per net Hp hidden words; the output stage: S | reward | done
    float *h1 = h0 + RB * Wd;                        // [RB][Wd] pong
    float *stat = h1 + RB * Wd;                      // [RB][3][2] mean, 1 / sqrt(var + eps) of a LayerNorm position
    float *rsum = stat + RB * 6;                     // [RB] the reward summed over the repeats so far

    const float sg = a.eps ? a.sign[chain] : 0.0f;
    const float *e = a.eps ? a.eps + (int64_t)a.worker[chain] * a.P : nullptr;
    const int ln_mask = (a.net[0].use_layer_norm ? 1 : 0) | (a.net[1].use_layer_norm ? 2 : 0) | (a.net[2].use_layer_norm ? 4 : 0);
    const int act0 = a.net[0].act, act1 = a.net[1].act, act2 = a.net[2].act;
    const float pr0 = a.net[0].prelu, pr1 = a.net[1].prelu, pr2 = a.net[2].prelu;

    if (!STREAM) {
        SvWalk wk;
        wk.begin(a);
        float *dst = wl;
        for (int l = 0; l <= L; ++l) {
            const int U = l == L ? n_outs : 3 * H, PS = sv_row_stride(wk.n_in);
            if (e) sv_stage_panel<true>(a, e, sg, dst, PS, l == L, l == 0, U, H, Hp, wk, 0, wk.n_in, tid);
            else sv_stage_panel<false>(a, e, sg, dst, PS, l == L, l == 0, U, H, Hp, wk, 0, wk.n_in, tid);
            dst += (size_t)U * PS;
            if (l < L) wk.past_hidden(l, H, ln_mask);
        }
    }

    for (int row0 = 0; row0 < a.n_per_chain; row0 += RB) {
        const int nr = a.n_per_chain - row0 < RB ? a.n_per_chain - row0 : RB;
        const int n_tiles = (nr + SV_RT - 1) / SV_RT;
        const int64_t grow = chain * a.n_per_chain + row0;
        __syncthreads();
        for (int i = tid; i < RB * Kp; i += SV_NT) {
            const int r = i / Kp, k = i - r * Kp;
            x[i] = (r < nr && k < K) ? (k < a.A ? a.action[(grow + r) * a.A + k] : a.state[(grow + r) * S + (k - a.A)]) : 0.0f;
        }
        for (int rep = 0; rep < a.repeat; ++rep) {
            const bool last = rep == a.repeat - 1;
            const float *in = x;
            int in_stride = Kp;
            float *hout = h0;
            const float *wst = wl;                   // resident: the stage's weights
            SvWalk wk;
            wk.begin(a);
            for (int l = 0; l <= L; ++l) {
                const bool out_stage = l == L;
                const int U = out_stage ? n_outs : 3 * H, n_in = wk.n_in;
                const int64_t b0 = wk.w0 + (int64_t)(out_stage ? S : H) * n_in, b1 = wk.w1 + (int64_t)(out_stage ? 1 : H) * n_in,
                              b2 = wk.w2 + (int64_t)(out_stage ? 1 : H) * n_in;
                const int KP = STREAM ? a.KP : n_in, PS = STREAM ? a.KP + 4 : sv_row_stride(n_in);
                for (int k0 = 0; k0 < n_in; k0 += KP) {
                    const int kp = n_in - k0 < KP ? n_in - k0 : KP;
                    __syncthreads();                 // `in` is complete; streaming: the panel's readers are done
                    if (STREAM) {
                        if (e) sv_stage_panel<true>(a, e, sg, wl, PS, out_stage, l == 0, U, H, Hp, wk, k0, kp, tid);
                        else sv_stage_panel<false>(a, e, sg, wl, PS, out_stage, l == 0, U, H, Hp, wk, k0, kp, tid);
                        __syncthreads();
                    }
                    const bool fin = k0 + kp == n_in;
                    for (int t = tid; t < U * n_tiles; t += SV_NT) {
                        const int tile = t / U, u = t - tile * U, rt = tile * SV_RT;
                        const SvUnit un = sv_unit(out_stage, l == 0, u, H, Hp, S);
                        const float *wrow = wst + (size_t)u * PS;
                        float *o = hout + rt * Wd + un.opos;
                        const float *xin = in + rt * in_stride + un.ibase + k0;
                        const float bias = fin ? sv_w(a, e, sg, sv_pick(un.net, b0, b1, b2) + un.j) : 0.0f;      // requested ahead of the dot products
                        float acc[SV_RT];
#pragma unroll
                        for (int i = 0; i < SV_RT; ++i) acc[i] = k0 == 0 ? 0.0f : o[i * Wd];
                        // four columns per round, two register sets: the unit's weights and the rows' inputs of the NEXT round are
                        // requested before this round's 4 x SV_RT fmas, so that the LDS latency hides behind them
                        const int kq = kp & ~3;
                        auto request = [&](int kk, float4 &w, float4 (&v)[SV_RT]) {
                            w = *reinterpret_cast<const float4 *>(wrow + kk);
#pragma unroll
                            for (int i = 0; i < SV_RT; ++i) v[i] = *reinterpret_cast<const float4 *>(xin + i * in_stride + kk);
                        };
                        auto round = [&](const float4 &w, const float4 (&v)[SV_RT]) {
#pragma unroll
                            for (int i = 0; i < SV_RT; ++i) {
                                acc[i] = fma32(v[i].x, w.x, acc[i]); acc[i] = fma32(v[i].y, w.y, acc[i]);
                                acc[i] = fma32(v[i].z, w.z, acc[i]); acc[i] = fma32(v[i].w, w.w, acc[i]);
                            }
                        };
                        int k = 0;
                        if (kq) {
                            float4 wa, wb, va[SV_RT], vb[SV_RT];
                            request(0, wa, va);
                            for (; k + 8 <= kq; k += 8) {
                                request(k + 4, wb, vb);
                                round(wa, va);
                                if (k + 8 < kq) request(k + 8, wa, va);
                                round(wb, vb);
                            }
                            if (k < kq) { round(wa, va); k += 4; }          // an odd number of quads: the last one is in the first set
                        }
                        for (; k < kp; ++k) {
                            const float w = wrow[k];
#pragma unroll
                            for (int i = 0; i < SV_RT; ++i) acc[i] = fma32(xin[i * in_stride + k], w, acc[i]);
                        }
                        if (fin) {
                            const bool raw = out_stage || (l >= 1 && ((ln_mask >> un.net) & 1));       // no activation here: the output layer, or LayerNorm comes first
                            const int act = sv_pick(un.net, act0, act1, act2);
                            const float prelu = sv_pick(un.net, pr0, pr1, pr2);
#pragma unroll
                            for (int i = 0; i < SV_RT; ++i) { const float z = acc[i] + bias; acc[i] = raw ? z : act_fwd(act, prelu, z); }
                        }
#pragma unroll
                        for (int i = 0; i < SV_RT; ++i) o[i * Wd] = acc[i];
                    }
                }
                if (out_stage) break;
                if (!STREAM) wst += (size_t)U * PS;
                wk.past_hidden(l, H, ln_mask);
                if (l >= 1 && ln_mask) {
                    __syncthreads();
                    for (int i = tid; i < nr * 3; i += SV_NT) {
                        const int r = i / 3, net = i - r * 3;
                        if (!((ln_mask >> net) & 1)) continue;
                        const float *zr = hout + r * Wd + net * Hp;
                        float sm = 0.0f, sv = 0.0f;
                        for (int j = 0; j < H; ++j) sm = sm + zr[j];
                        const float mean = sm / (float)H;
                        for (int j = 0; j < H; ++j) { const float dj = zr[j] - mean; sv = fma32(dj, dj, sv); }
                        stat[2 * i] = mean; stat[2 * i + 1] = 1.0f / __builtin_sqrtf(sv / (float)H + 1e-5f);
                    }
                    __syncthreads();
                    for (int u = tid; u < 3 * H; u += SV_NT) {
                        const int net = u / H, j = u - net * H;
                        if (!((ln_mask >> net) & 1)) continue;
                        const int64_t lo = sv_pick(net, wk.ln0, wk.ln1, wk.ln2) + j;
                        const float lw = sv_w(a, e, sg, lo), lb = sv_w(a, e, sg, lo + H);
                        const int act = sv_pick(net, act0, act1, act2);
                        const float prelu = sv_pick(net, pr0, pr1, pr2);
                        for (int r = 0; r < nr; ++r) {
                            float *o = hout + r * Wd + net * Hp + j;
                            *o = act_fwd(act, prelu, fma32((*o - stat[2 * (r * 3 + net)]) * stat[2 * (r * 3 + net) + 1], lw, lb));
                        }
                    }
                }
                in = hout;
                in_stride = Wd;
                hout = (hout == h0) ? h1 : h0;
            }
            __syncthreads();
            // hout rows: S next-state words | reward | done.  x is read by the first layer only: the next state goes back into it
            for (int i = tid; i < nr * n_outs; i += SV_NT) {
                const int r = i / n_outs, t = i - r * n_outs;
                const float v = hout[r * Wd + t];
                if (t < S) {
                    if (last) a.next_state[(grow + r) * S + t] = v; else x[r * Kp + a.A + t] = v;
                } else if (t == S) {
                    const float s = rep == 0 ? v : rsum[r] + v;          // left to right in fp32; the same thread every repeat
                    rsum[r] = s;
                    if (last) a.reward[grow + r] = s;
                } else if (last) a.done[grow + r] = v;
            }
        }
    }
}

}  // namespace lenv

using namespace lenv;

// Descriptor checks of lenv_se_step_population, the bounds of this entry and the choice of kernel: 0 resident, 1 streaming (a.KP / a.RB /
// a.wfloats and *lds_bytes filled in), or a negative LENV_ERR_*.
static int sv_plan(const lenv_mlp_desc *sn, const lenv_mlp_desc *rn, const lenv_mlp_desc *dn, int32_t n_per_chain, SvArgs &a, size_t *lds_bytes)
{
    if (!sn || !rn || !dn || n_per_chain < 1) return LENV_ERR_INVALID;
    // the three nets share input, width and depth (envs/virtual_env.py:23-31)
    if (sn->in_dim != rn->in_dim || sn->in_dim != dn->in_dim || sn->hidden != rn->hidden || sn->hidden != dn->hidden ||
        sn->layers != rn->layers || sn->layers != dn->layers || rn->out_dim != 1 || dn->out_dim != 1)
        return LENV_ERR_INVALID;
    a.net[0] = *sn; a.net[1] = *rn; a.net[2] = *dn;
    a.S = sn->out_dim; a.A = sn->in_dim - sn->out_dim;
    if (a.A < 1 || a.S < 1 || sn->layers < 1 || sn->hidden < 1) return LENV_ERR_UNSUPPORTED;
    if (sn->hidden > SV_MAX_HIDDEN || sn->layers > SV_MAX_LAYERS || sn->in_dim > SV_MAX_IN) return LENV_ERR_UNSUPPORTED;
    a.net_off[0] = 0;
    a.net_off[1] = lenv_mlp_num_params(sn);
    a.net_off[2] = a.net_off[1] + lenv_mlp_num_params(rn);
    a.P = a.net_off[2] + lenv_mlp_num_params(dn);
    const int H = sn->hidden, K = sn->in_dim, L = sn->layers;
    const int Hp = (H + 3) & ~3, Kp = (K + 3) & ~3, n_outs = a.S + 2;
    const size_t Wd = 3 * Hp > ((n_outs + 3) & ~3) ? 3 * Hp : ((n_outs + 3) & ~3);
    const size_t Umax = 3 * H > n_outs ? 3 * H : n_outs;
    const size_t row_floats = Kp + 2 * Wd + 6 + 1;                       // x | ping | pong | LayerNorm statistics | reward sum
    // resident: every stage in its padded layout next to one register tile of rows -- whatever n_per_chain is
    const size_t all_stages = (size_t)3 * H * sv_row_stride(K) + (size_t)(L - 1) * 3 * H * sv_row_stride(H) + (size_t)n_outs * sv_row_stride(H);
    const size_t resident = (all_stages + SV_RT * row_floats + 4) * sizeof(float);
    if (resident <= SV_LDS_BYTES) { a.KP = 0; a.RB = SV_RT; a.wfloats = (int)all_stages; *lds_bytes = resident; return 0; }
    // streaming: a weight is staged once per row block, so as many register tiles of rows per block (4, 2, 1) as the launch has rows for
    // and as leave the panel 32 columns; then the widest panel that fits
    for (int RB = n_per_chain > 2 * SV_RT ? 4 * SV_RT : (n_per_chain > SV_RT ? 2 * SV_RT : SV_RT); RB >= SV_RT; RB /= 2)
        for (int KP = 64; KP >= (RB > SV_RT ? 32 : 8); KP -= 8) {
            const size_t bytes = (Umax * (KP + 4) + RB * row_floats + 4) * sizeof(float);
            if (bytes <= SV_LDS_BYTES) { a.KP = KP; a.RB = RB; a.wfloats = (int)(Umax * (KP + 4)); *lds_bytes = bytes; return 1; }
        }
    return LENV_ERR_UNSUPPORTED;     // not reached inside the bounds above: 768 units x 12 floats + 8 rows x 1799 floats = 94 KiB
}

extern "C" int32_t lenv_se_step_vec_path(const lenv_mlp_desc *sn, const lenv_mlp_desc *rn, const lenv_mlp_desc *dn, int32_t n_per_chain)
{
    SvArgs a;
    size_t lds_bytes = 0;
    return sv_plan(sn, rn, dn, n_per_chain, a, &lds_bytes);
}

extern "C" int lenv_se_step_population_vec(const lenv_mlp_desc *sn, const lenv_mlp_desc *rn, const lenv_mlp_desc *dn,
                                           const float *theta, const float *eps, const int32_t *worker, const float *sign,
                                           int64_t chains, int32_t n_per_chain, int32_t repeat, const float *state, const float *action,
                                           float *next_state, float *reward, float *done, void *stream)
{
    if (!sn || !rn || !dn || !theta || !state || !action || !next_state || !reward || !done) return LENV_ERR_INVALID;
    if (eps && (!worker || !sign)) return LENV_ERR_INVALID;
    if (chains < 0 || n_per_chain < 1 || repeat < 1) return LENV_ERR_INVALID;
    if (chains == 0) return LENV_OK;                 // before the descriptor checks, as in lenv_se_step_population
    if (chains > 0x7fffffff) return LENV_ERR_UNSUPPORTED;            // the grid's x dimension
    SvArgs a;
    size_t lds_bytes = 0;
    const int path = sv_plan(sn, rn, dn, n_per_chain, a, &lds_bytes);
    if (path < 0) return path;
    a.theta = theta; a.eps = eps; a.worker = worker; a.sign = sign; a.n_per_chain = n_per_chain; a.repeat = repeat;
    a.state = state; a.action = action; a.next_state = next_state; a.reward = reward; a.done = done;
    const void *kern = path == 0 ? reinterpret_cast<const void *>(se_step_vec_kernel<false>) : reinterpret_cast<const void *>(se_step_vec_kernel<true>);
    // always the whole LDS: host threads that launch different shapes at once then all set the same value
    if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SV_LDS_BYTES) != hipSuccess) return LENV_ERR_LAUNCH;
    if (path == 0)
        hipLaunchKernelGGL(se_step_vec_kernel<false>, dim3((unsigned)chains), dim3(SV_NT), lds_bytes, static_cast<hipStream_t>(stream), a);
    else
        hipLaunchKernelGGL(se_step_vec_kernel<true>, dim3((unsigned)chains), dim3(SV_NT), lds_bytes, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? LENV_OK : LENV_ERR_LAUNCH;
}
