// se_fit.hip -- supervised fit of a population of VirtualEnvs on recorded transitions (the "Supervised Learning / MBRL Baseline" the reference
// reports for CartPole; its experiments/syn_env_evaluate_cartpole_mbrl_baseline.py leaves fit_mbrl_baseline() a NotImplementedError): Adam
// steps on F.mse_loss of the three SE nets (state, reward, done; envs/virtual_env.py:43-54) over minibatches drawn with replacement.
//
// Grid (model, net): the three nets of a model share no parameter, so each is one workgroup with no cross-workgroup synchronisation, and the
// loop over the steps runs inside the kernel.  A net's parameters, Adam moments and gradient live in LDS behind the minibatch activations
// where that fits (RES), else the parameters and moments stay in the caller's arrays and the gradient in the workspace; the arithmetic is
// the same sequence on either path.
//
// Canonical order (tests/se_fit_ref.c restates it on the CPU, bit for bit):
//   forward    orc_mlp_forward's: k-ascending fmaf chain from 0.0f, bias added last
//   loss       fmaf chain of the squared errors over rows ascending, outputs ascending inside a row, / (float)(batch * out_dim)
//   dL/dy      (float)(2.0 / (double)(batch * out_dim)) * e
//   gradient   every weight / bias gradient is a chain over the minibatch rows in ascending order (mlp_backward_one_ex's accumulation):
//              the minibatch is walked in chunks of SF_RC rows and the chains continue from chunk to chunk
//   Adam       adam_elem of lenv_gemm.cuh (torch.optim.Adam single-tensor step); beta^t continued in double from the host's powers
//
// Activations are kept TRANSPOSED in LDS ([unit][row], row stride odd): a lane per row reads them conflict-free while the weight is a
// broadcast, and a lane per unit (the gradient phases) walks rows with an odd stride between lanes.
#include "lenv_device.cuh"
#include "lenv_gemm.cuh"
#include "lenv_host.h"

namespace lenv {

constexpr int SF_NT = 1024;                       // threads of a workgroup
constexpr int SF_RC = 64;                         // minibatch rows of a chunk
constexpr size_t SF_LDS_LIMIT = 160 * 1024 - 256;

struct SfLayout { int rc, ld, o_x, o_e, o_act, o_par, ppad; size_t bytes; bool resident; };

// dynamic LDS of a workgroup, in floats: idx [batch] | xT [in][ld] | eT [out][ld] | act [layers][hidden][ld] | (RES) w, m, v, g [ppad] each.
// out / pmax are the state net's (the widest of the three): every workgroup of a launch gets the same size and takes the same path.
__host__ __device__ inline SfLayout sf_layout(int in, int hidden, int layers, int out, int batch, int pmax)
{
    SfLayout l;
    l.rc = batch < SF_RC ? batch : SF_RC;
    l.ld = l.rc | 1;
    l.o_x = (batch + 3) & ~3;
    l.o_e = l.o_x + ((in * l.ld + 3) & ~3);
    l.o_act = l.o_e + ((out * l.ld + 3) & ~3);
    l.o_par = l.o_act + ((layers * hidden * l.ld + 3) & ~3);
    l.ppad = (pmax + 3) & ~3;
    const size_t with_params = ((size_t)l.o_par + 4 * (size_t)l.ppad) * sizeof(float);
    l.resident = with_params <= SF_LDS_LIMIT;
    l.bytes = l.resident ? with_params : (size_t)l.o_par * sizeof(float);
    return l;
}

struct SfArgs {
    int32_t in_dim, hidden, layers, act, state_out, batch;
    int64_t N, step_begin, nsteps, P, ws_stride;
    int32_t p_net[3], ws_off[3];
    double lr, beta1, beta2, adam_eps, b1pow, b2pow;          // b?pow = beta?^step_begin (host, repeated multiplication from step 0)
    const float *x, *y[3];
    const uint64_t *rng_keys;
    const int32_t *batch_idx;
    float *theta, *adam_m, *adam_v, *loss, *ws;
};

// one Linear + activation over the chunk: outT[j][b] = act(chain_k inT[k][b] * W[j][k] + bias[j]); four output units per item
__device__ __forceinline__ void sf_forward(const float *inT, int n_in, const float *W, const float *bias, float *outT, int rc, int ld, int H, int act,
                                           int tid)
{
    const int nq = (H + 3) >> 2;
    for (int e = tid; e < rc * nq; e += SF_NT) {
        const int q = e / rc, b = e - q * rc, j0 = 4 * q;
        const float *w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = W + (size_t)(j0 + u < H ? j0 + u : H - 1) * n_in;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int k = 0; k < n_in; ++k) {
            const float xa = inT[k * ld + b];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = fma32(xa, w[u][k], acc[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (j0 + u < H) outT[(j0 + u) * ld + b] = act_fwd(act, 0.0f, acc[u] + bias[j0 + u]);
    }
}

// gradient of one Linear over the chunk's rows, continuing the chains in G: gW[j][i] = fma(dT[j][b], inT[i][b], gW[j][i]), gb[j] = gb[j] + dT[j][b]
// (item i == n_in is the bias); scale multiplies dT on the way in (the output layer keeps the raw errors in LDS)
__device__ __forceinline__ void sf_wgrad(const float *dT, int n_out, const float *inT, int n_in, float *gW, float *gb, int rc, int ld, float scale,
                                         bool scaled, int tid)
{
    for (int e = tid; e < n_out * (n_in + 1); e += SF_NT) {
        const int j = e / (n_in + 1), i = e - j * (n_in + 1);
        const float *dr = dT + j * ld;
        if (i < n_in) {
            const float *ir = inT + i * ld;
            float g = gW[(size_t)j * n_in + i];
            for (int b = 0; b < rc; ++b) { const float d = scaled ? scale * dr[b] : dr[b]; g = fma32(d, ir[b], g); }
            gW[(size_t)j * n_in + i] = g;
        } else {
            float g = gb[j];
            for (int b = 0; b < rc; ++b) { const float d = scaled ? scale * dr[b] : dr[b]; g = g + d; }
            gb[j] = g;
        }
    }
}

// back through one Linear and the activation in front of it, in place: aT[i][b] = act_bwd(aT[i][b], chain_j dT[j][b] * W[j][i])
__device__ __forceinline__ void sf_dgrad(const float *dT, int n_out, const float *W, float *aT, int n_in, int rc, int ld, int act, float scale,
                                         bool scaled, int tid)
{
    for (int e = tid; e < rc * n_in; e += SF_NT) {
        const int i = e / rc, b = e - i * rc;
        float acc = 0.0f;
        for (int j = 0; j < n_out; ++j) { const float d = scaled ? scale * dT[j * ld + b] : dT[j * ld + b]; acc = fma32(d, W[(size_t)j * n_in + i], acc); }
        aT[i * ld + b] = act_bwd(act, 0.0f, aT[i * ld + b], acc);
    }
}

// torch.optim.Adam single-tensor step on [0, n): four elements per thread, every load in front of the first store
__device__ __forceinline__ void sf_adam(float *w, float *m, float *v, const float *g, int n, const AdamConsts c, int tid)
{
    for (int p0 = tid; p0 < n; p0 += 4 * SF_NT) {
        float gg[4], mm[4], vv[4], ww[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = p0 + u * SF_NT < n ? p0 + u * SF_NT : p0;
            gg[u] = g[p]; mm[u] = m[p]; vv[u] = v[p]; ww[u] = w[p];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) { float t = 0.0f; adam_elem(gg[u], mm[u], vv[u], ww[u], t, c, 0.0f, 0.0f); }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = p0 + u * SF_NT;
            if (p < n) { m[p] = mm[u]; v[p] = vv[u]; w[p] = ww[u]; }
        }
    }
}

template <bool RES>
__global__ __launch_bounds__(SF_NT) void se_fit_kernel(const SfArgs a)
{
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, net = blockIdx.y;
    const int64_t model = blockIdx.x;
    const int in = a.in_dim, H = a.hidden, L = a.layers, act = a.act, B = a.batch, O = net == 0 ? a.state_out : 1;
    const int Pn = a.p_net[net], P0 = in * H + H, P1 = H * H + H;
    const SfLayout lay = sf_layout(in, H, L, a.state_out, B, a.p_net[0]);
    const int ld = lay.ld;
    int32_t *idx = reinterpret_cast<int32_t *>(lds);
    float *xT = lds + lay.o_x, *eT = lds + lay.o_e, *act0 = lds + lay.o_act, *act1 = act0 + H * ld;
    float *aL = L == 2 ? act1 : act0;
    const int64_t goff = model * a.P + (net >= 1 ? a.p_net[0] : 0) + (net == 2 ? a.p_net[1] : 0);
    float *const g_w = a.theta + goff, *const g_m = a.adam_m + goff, *const g_v = a.adam_v + goff;
    float *W, *M, *V, *G;
    if constexpr (RES) {
        W = lds + lay.o_par; M = W + lay.ppad; V = M + lay.ppad; G = V + lay.ppad;
        for (int p = tid; p < Pn; p += SF_NT) { W[p] = g_w[p]; M[p] = g_m[p]; V[p] = g_v[p]; }
    } else {
        W = g_w; M = g_m; V = g_v; G = a.ws + model * a.ws_stride + a.ws_off[net];
    }
    const float *y = a.y[net];
    float *const Wo = W + P0 + (L - 1) * P1, *const Go = G + P0 + (L - 1) * P1;
    const float scale = (float)(2.0 / (double)(B * O));
    const uint64_t key = a.rng_keys ? a.rng_keys[model] : 0;
    double b1pow = a.b1pow, b2pow = a.b2pow;
    AdamConsts ac;
    ac.w1 = (float)(1.0 - a.beta1); ac.w2 = (float)(1.0 - a.beta2); ac.beta2 = (float)a.beta2; ac.eps = (float)a.adam_eps;

    for (int64_t it = 0; it < a.nsteps; ++it) {
        const int64_t t = a.step_begin + it;
        for (int p = tid; p < Pn; p += SF_NT) G[p] = 0.0f;
        for (int j = tid; j < B; j += SF_NT) {
            int64_t r = a.batch_idx ? (int64_t)a.batch_idx[(model * a.nsteps + it) * B + j]
                                    : (int64_t)u64_to_below(rng_u64(key, STREAM_SE_FIT_BATCH, (uint64_t)(t * B + j)), (uint32_t)a.N);
            r = r < 0 ? 0 : r >= a.N ? a.N - 1 : r;          // a tape index outside the data set reads its nearest row, never past the arrays
            idx[j] = (int32_t)r;
        }
        float lsum = 0.0f;
        __syncthreads();
        for (int c0 = 0; c0 < B; c0 += SF_RC) {
            const int rc = B - c0 < SF_RC ? B - c0 : SF_RC;
            // the chunk's rows leave HBM once: inputs and targets, transposed
            for (int e = tid; e < rc * in; e += SF_NT) { const int b = e / in, k = e - b * in; xT[k * ld + b] = a.x[(int64_t)idx[c0 + b] * in + k]; }
            for (int e = tid; e < rc * O; e += SF_NT) { const int b = e / O, o = e - b * O; eT[o * ld + b] = y[(int64_t)idx[c0 + b] * O + o]; }
            __syncthreads();
            sf_forward(xT, in, W, W + in * H, act0, rc, ld, H, act, tid);
            __syncthreads();
            if (L == 2) {
                sf_forward(act0, H, W + P0, W + P0 + H * H, act1, rc, ld, H, act, tid);
                __syncthreads();
            }
            // output layer; eT turns from the targets into the errors e = y - target
            for (int e = tid; e < rc * O; e += SF_NT) {
                const int o = e / rc, b = e - o * rc;
                float acc = 0.0f;
                for (int k = 0; k < H; ++k) acc = fma32(aL[k * ld + b], Wo[o * H + k], acc);
                eT[o * ld + b] = (acc + Wo[O * H + o]) - eT[o * ld + b];
            }
            __syncthreads();
            if (tid == 0)
                for (int b = 0; b < rc; ++b)
                    for (int o = 0; o < O; ++o) { const float ev = eT[o * ld + b]; lsum = fma32(ev, ev, lsum); }
            sf_wgrad(eT, O, aL, H, Go, Go + O * H, rc, ld, scale, true, tid);
            __syncthreads();
            sf_dgrad(eT, O, Wo, aL, H, rc, ld, act, scale, true, tid);              // aL now holds dL/dz of the last hidden layer
            __syncthreads();
            if (L == 2) {
                sf_wgrad(act1, H, act0, H, G + P0, G + P0 + H * H, rc, ld, 0.0f, false, tid);
                __syncthreads();
                sf_dgrad(act1, H, W + P0, act0, H, rc, ld, act, 0.0f, false, tid);
                __syncthreads();
            }
            sf_wgrad(act0, H, xT, in, G, G + in * H, rc, ld, 0.0f, false, tid);
            __syncthreads();
        }
        if (tid == 0 && a.loss) a.loss[(model * a.nsteps + it) * 3 + net] = lsum / (float)(B * O);
        b1pow *= a.beta1; b2pow *= a.beta2;
        ac.neg_step = (float)(-(a.lr / (1.0 - b1pow)));
        ac.bc2_sqrt = (float)__builtin_sqrt(1.0 - b2pow);
        sf_adam(W, M, V, G, Pn, ac, tid);
        __syncthreads();
    }
    if constexpr (RES)
        for (int p = tid; p < Pn; p += SF_NT) { g_w[p] = W[p]; g_m[p] = M[p]; g_v[p] = V[p]; }
}

}  // namespace lenv

using namespace lenv;

namespace {

struct SfShape { int32_t p_net[3], ws_off[3]; int64_t P, ws_stride; SfLayout lay; };

int64_t sf_net_params(const lenv_mlp_desc *d)
{
    const int64_t H = d->hidden;
    return (int64_t)d->in_dim * H + H + (int64_t)(d->layers - 1) * (H * H + H) + H * d->out_dim + d->out_dim;
}

// the shapes the kernel takes (include/lenv_hip.h); batch < 0: the shape of the nets alone
int sf_shape(const lenv_mlp_desc *sn, const lenv_mlp_desc *rn, const lenv_mlp_desc *dn, int32_t batch, SfShape *s)
{
    if (!sn || !rn || !dn) return LENV_ERR_INVALID;
    const lenv_mlp_desc *nets[3] = {sn, rn, dn};
    for (const lenv_mlp_desc *d : nets) {
        if (d->in_dim != sn->in_dim || d->hidden != sn->hidden || d->layers != sn->layers || d->act != sn->act) return LENV_ERR_UNSUPPORTED;
        if (d->use_layer_norm) return LENV_ERR_UNSUPPORTED;
    }
    if (sn->act != LENV_ACT_IDENTITY && sn->act != LENV_ACT_RELU && sn->act != LENV_ACT_LEAKYRELU && sn->act != LENV_ACT_TANH) return LENV_ERR_UNSUPPORTED;
    if (sn->in_dim < 1 || sn->in_dim > 32 || sn->out_dim < 1 || sn->out_dim > 32 || rn->out_dim != 1 || dn->out_dim != 1) return LENV_ERR_UNSUPPORTED;
    if (sn->hidden < 1 || sn->hidden > 128 || sn->layers < 1 || sn->layers > 2) return LENV_ERR_UNSUPPORTED;
    if (batch >= 0 && (batch < 1 || batch > 256)) return LENV_ERR_UNSUPPORTED;
    lenv_host::ArenaCursor cur;
    s->P = 0;
    for (int k = 0; k < 3; ++k) { s->p_net[k] = (int32_t)sf_net_params(nets[k]); s->P += s->p_net[k]; s->ws_off[k] = (int32_t)cur.take(s->p_net[k]); }
    s->ws_stride = cur.total();
    s->lay = sf_layout(sn->in_dim, sn->hidden, sn->layers, sn->out_dim, batch >= 0 ? batch : 1, s->p_net[0]);
    if (s->lay.bytes > SF_LDS_LIMIT) return LENV_ERR_UNSUPPORTED;
    return LENV_OK;
}

}  // namespace

extern "C" int64_t lenv_se_fit_num_params(const lenv_mlp_desc *sn, const lenv_mlp_desc *rn, const lenv_mlp_desc *dn)
{
    SfShape s;
    const int rc = sf_shape(sn, rn, dn, -1, &s);
    return rc != LENV_OK ? rc : s.P;
}

extern "C" int64_t lenv_se_fit_lds_bytes(const lenv_mlp_desc *sn, const lenv_mlp_desc *rn, const lenv_mlp_desc *dn, int32_t batch)
{
    SfShape s;
    const int rc = sf_shape(sn, rn, dn, batch < 0 ? 0 : batch, &s);
    return rc != LENV_OK ? rc : (int64_t)s.lay.bytes;
}

extern "C" int64_t lenv_se_fit_workspace_bytes(const lenv_mlp_desc *sn, const lenv_mlp_desc *rn, const lenv_mlp_desc *dn, int32_t batch, int64_t models)
{
    SfShape s;
    const int rc = sf_shape(sn, rn, dn, batch < 0 ? 0 : batch, &s);
    if (rc != LENV_OK) return rc;
    if (models < 0) return LENV_ERR_INVALID;
    if (models >= ((int64_t)1 << 31)) return LENV_ERR_UNSUPPORTED;
    return s.lay.resident ? 0 : models * s.ws_stride * (int64_t)sizeof(float);
}

extern "C" int lenv_se_fit_population(const lenv_mlp_desc *sn, const lenv_mlp_desc *rn, const lenv_mlp_desc *dn, const float *x, const float *y_state,
                                      const float *y_reward, const float *y_done, int64_t N, int32_t batch, int64_t step_begin, int64_t step_end,
                                      double lr, double beta1, double beta2, double adam_eps, const uint64_t *rng_keys, const int32_t *batch_idx,
                                      int64_t models, float *theta, float *adam_m, float *adam_v, float *loss, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    if (!sn || !rn || !dn) return LENV_ERR_INVALID;
    if (N > 0 && (!x || !y_state || !y_reward || !y_done)) return LENV_ERR_INVALID;
    if (step_begin < 0 || step_end < step_begin || models < 0) return LENV_ERR_INVALID;
    if (N < 1 && step_end > step_begin) return LENV_ERR_INVALID;
    if (models > 0 && (!theta || !adam_m || !adam_v)) return LENV_ERR_INVALID;
    if ((rng_keys != nullptr) == (batch_idx != nullptr)) return LENV_ERR_INVALID;
    SfShape s;
    const int rc = sf_shape(sn, rn, dn, batch < 0 ? 0 : batch, &s);
    if (rc != LENV_OK) return rc;
    if (models >= ((int64_t)1 << 31) || N >= ((int64_t)1 << 31)) return LENV_ERR_UNSUPPORTED;
    const size_t need = s.lay.resident ? 0 : (size_t)models * (size_t)s.ws_stride * sizeof(float);
    if (workspace_bytes < need || (need > 0 && !workspace)) return LENV_ERR_WORKSPACE;
    if (models == 0 || step_end == step_begin) return LENV_OK;

    SfArgs a{};
    a.in_dim = sn->in_dim; a.hidden = sn->hidden; a.layers = sn->layers; a.act = sn->act; a.state_out = sn->out_dim; a.batch = batch;
    a.N = N; a.step_begin = step_begin; a.nsteps = step_end - step_begin; a.P = s.P; a.ws_stride = s.ws_stride;
    for (int k = 0; k < 3; ++k) { a.p_net[k] = s.p_net[k]; a.ws_off[k] = s.ws_off[k]; }
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.adam_eps = adam_eps;
    a.b1pow = 1.0; a.b2pow = 1.0;
    for (int64_t i = 0; i < step_begin; ++i) { a.b1pow *= beta1; a.b2pow *= beta2; }
    a.x = x; a.y[0] = y_state; a.y[1] = y_reward; a.y[2] = y_done;
    a.rng_keys = rng_keys; a.batch_idx = batch_idx;
    a.theta = theta; a.adam_m = adam_m; a.adam_v = adam_v; a.loss = loss; a.ws = static_cast<float *>(workspace);
    const dim3 grid((unsigned)models, 3);
    if (s.lay.resident) return lenv_host::launch(se_fit_kernel<true>, grid, dim3(SF_NT), s.lay.bytes, stream, a);
    return lenv_host::launch(se_fit_kernel<false>, grid, dim3(SF_NT), s.lay.bytes, stream, a);
}
