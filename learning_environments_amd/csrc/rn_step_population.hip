// rn_step_population.hip -- one step of a RewardEnv (a vector-state real env + a perturbed reward net) for a whole NES population in one launch:
// the non-virtual half of EnvWrapper.step_population.  Workgroup c owns chain c: it steps the env's fp64 physics on the chain's action up to
// `repeat` times (the same_action_num loop of EnvWrapper._step_real, envs/env_wrapper.py:48-70: shaped rewards summed, stop after the step that
// reports done, TimeLimit included) and shapes every step's reward with W_c = theta + sign[c]*eps[worker[c]] (RewardEnv._calc_reward,
// envs/reward_env.py:68-133, all eleven types).
//
// Nothing is restated here: the physics are real_env_step / ContEnv<ENV> of lenv_device.cuh (what lenv_real_env_step / lenv_cont_env_step and the
// fused loops call), the net is rn_eval_row of lenv_rn.cuh (the fused loops' wg_rn_eval is its 512-thread instantiation), the info vector is
// cheetah_info_row and the shaping rn_shaped_reward.  A hidden unit's sum is the k-ascending fmaf chain whatever the lane stride, so the group
// size does not show in the bits: one wave per chain for nets up to 64 wide, four waves (a lane per unit up to 256) above.
//
// theta: a one-hidden-layer net and the Linear(info_dim, 1) of types 101 / 102 are perturbed once into LDS (rn_theta_in_lds); a deeper net
// (up to 3 x 256 x 256 floats) is perturbed on the way into the fmaf chain, element by element from global memory -- every weight is used once
// per evaluation, so a staged copy would only add a round trip.  Layout: lenv_mlp_desc's, the shared LayerNorm's weight | bias behind the second
// Linear, as lenv_rn_shape_rows takes it.
// The env's fp64 state: the continuous envs keep it in LDS and a lane computes one word (cont_env_step_kernel's split); the discrete envs'
// four words sit in every lane's registers and every lane steps them (an fp64 chain costs a wave the same on one lane or 64), which leaves
// reward, done and the elapsed count uniform without a hand-over.  phi(s') of one repeat is phi(s) of the next, except for types 3 / 4, whose
// phi([s | info]) reads the info of the step at hand.
#include <hip/hip_runtime.h>
#include "../../include/lenv_hip.h"
#include "lenv_rn.cuh"
#include "lenv_host.h"

namespace lenv {

constexpr int RSP_MAXH = 256, RSP_MAXIN = 64, RSP_MAXSD = 17, RSP_MAXREPEAT = 64;

struct RspArgs {
    int env_id, max_steps, type, S, SD, A, info_dim, H, act, L, ln, repeat;
    int P, lds_theta;                 // floats of theta; whether W_c is staged in LDS
    float prelu, gamma;
    const float *theta, *eps; const int32_t *worker; const float *sign;
    const void *action;               // int32 [chains] | float [chains, A]
    double *state; int32_t *elapsed;
    float *obs, *reward, *done;
};

// W_c formed where it is read: what rn_eval_row needs of a parameter pointer
struct RspPerturbed {
    const float *theta, *eps;
    float sign;
    __device__ __forceinline__ RspPerturbed operator+(int o) const { return RspPerturbed{ theta + o, eps + o, sign }; }
    __device__ __forceinline__ float operator[](int i) const { return fma32(sign, eps[i], theta[i]); }
};

// one step of a continuous env from x into nx (LDS), the split of cont_env_step_kernel (mlp_forward.hip); every lane follows the reward, the
// done flag and the step count.  Ends with a barrier: on / info / nx are complete.
template <int ENV>
__device__ __forceinline__ void rsp_cont_step(int tid, const double *x, double *nx, const float *act, bool want_info, int max_steps, float *on,
                                              float *info, int &el, float &r32, int &dn)
{
    using E = ContEnv<ENV>;
    if (tid < E::SD) nx[tid] = E::step_word(tid, x, act);
    const double pre = E::reward_pre(x, act);
    __syncthreads();
    el = el + 1;
    r32 = (float)E::reward_post(nx, pre);
    dn = (E::done(nx) || el >= max_steps) ? 1 : 0;
    if (tid < E::S) on[tid] = E::obs(tid, nx);
    if constexpr (E::INFO == 4) { if (tid == 0 && want_info) cheetah_info_row(info, nx, pre); }
    __syncthreads();
}

template <int NT, bool FLY>
__global__ __launch_bounds__(NT) void rn_step_population_kernel(const RspArgs a)
{
    extern __shared__ __align__(16) float wlds[];                  // W_c when a.lds_theta
    __shared__ double xs[2][RSP_MAXSD];
    __shared__ float obuf[2][RSP_MAXIN], info[4], ctrl[16], hbuf[2][RSP_MAXH];
    const int tid = threadIdx.x, t = a.type, S = a.S, SD = a.SD;
    const int64_t c = blockIdx.x;
    const bool cont = a.env_id == LENV_ENV_PENDULUM || a.env_id == LENV_ENV_CMC || a.env_id == LENV_ENV_CHEETAH_STANDIN;
    const float sg = a.eps ? a.sign[c] : 0.0f;
    const float *e = a.eps ? a.eps + (int64_t)a.worker[c] * a.P : nullptr;
    if (a.lds_theta) for (int i = tid; i < a.P; i += NT) wlds[i] = e ? fma32(sg, e[i], a.theta[i]) : a.theta[i];
    if (tid == 0) { ctrl[0] = 0.0f; ctrl[1] = 0.0f; }

    const RnRow row{ t, S, a.info_dim, a.H, a.L, a.act, a.prelu, a.ln != 0, a.lds_theta ? wlds : a.theta, hbuf[0], hbuf[1], ctrl };
    auto rn_eval = [&](const float *o, int slot) {
        if constexpr (FLY) rn_eval_row<NT, true>(row, RspPerturbed{ a.theta, e, sg }, o, info, slot);
        else rn_eval_row<NT, true>(row, row.par, o, info, slot);
    };

    int el = a.elapsed[c], cur = 0, dn = 0;
    double st[4] = { 0.0, 0.0, 0.0, 0.0 };
    if (cont) { if (tid < SD) xs[0][tid] = a.state[c * SD + tid]; }
    else { for (int k = 0; k < 4; ++k) st[k] = a.state[c * 4 + k]; }
    __syncthreads();
    float *os = obuf[0], *on = obuf[1];
    const bool want_info = rn_type_info_in(t) || t > 100;
    if (t >= 1 && t <= 4) {                                        // phi(s) of the first repeat: s = the observation of the state handed in
        if (a.env_id == LENV_ENV_PENDULUM) { if (tid < S) os[tid] = ContEnv<LENV_ENV_PENDULUM>::obs(tid, xs[0]); }
        else if (a.env_id == LENV_ENV_CMC) { if (tid < S) os[tid] = ContEnv<LENV_ENV_CMC>::obs(tid, xs[0]); }
        else if (a.env_id == LENV_ENV_CHEETAH_STANDIN) { if (tid < S) os[tid] = ContEnv<LENV_ENV_CHEETAH_STANDIN>::obs(tid, xs[0]); }
        else if (tid == 0) real_env_obs(a.env_id, st, os);
        __syncthreads();
        if (t <= 2) rn_eval(os, 0);
    }

    const float g32 = a.gamma;
    double sum = 0.0;
    for (int rep = 0; rep < a.repeat; ++rep) {
        float r32;
        if (cont) {
            const float *act = static_cast<const float *>(a.action) + c * a.A;
            if (a.env_id == LENV_ENV_PENDULUM) rsp_cont_step<LENV_ENV_PENDULUM>(tid, xs[cur], xs[cur ^ 1], act, want_info, a.max_steps, on, info, el, r32, dn);
            else if (a.env_id == LENV_ENV_CMC) rsp_cont_step<LENV_ENV_CMC>(tid, xs[cur], xs[cur ^ 1], act, want_info, a.max_steps, on, info, el, r32, dn);
            else rsp_cont_step<LENV_ENV_CHEETAH_STANDIN>(tid, xs[cur], xs[cur ^ 1], act, want_info, a.max_steps, on, info, el, r32, dn);
            cur ^= 1;
        } else {
            double rew;
            real_env_step(a.env_id, st, static_cast<const int32_t *>(a.action)[c], rew, dn);
            el = el + 1;
            if (el >= a.max_steps) dn = 1;                         // gym.wrappers.TimeLimit
            if (tid == 0) real_env_obs(a.env_id, st, on);
            r32 = (float)rew;
            __syncthreads();
        }
        if (t == 3 || t == 4) rn_eval(os, 0);                      // phi([s | info]): info is this step's
        if (t != 0) rn_eval(on, 1);                                // phi(s') / phi([s' | info]) / w . info
        const float phi_s2 = ctrl[1];
        sum = sum + (double)rn_shaped_reward(t, r32, g32, ctrl[0], phi_s2);
        if (dn || rep + 1 == a.repeat) break;                      // uniform
        __syncthreads();                                           // every lane has read ctrl[0] / ctrl[1]
        if (tid == 0) ctrl[0] = phi_s2;
        float *t2 = os; os = on; on = t2;
    }

    if (tid < S) a.obs[c * S + tid] = on[tid];
    if (cont) { if (tid < SD) a.state[c * SD + tid] = xs[cur][tid]; }
    else if (tid == 0) { for (int k = 0; k < 4; ++k) a.state[c * 4 + k] = st[k]; }
    if (tid == 0) { a.reward[c] = (float)sum; a.done[c] = dn ? 1.0f : 0.0f; a.elapsed[c] = el; }
}

}  // namespace lenv

using namespace lenv;

static bool rsp_type_known(int t) { return (t >= 0 && t <= 8) || t == 101 || t == 102; }

// observation / fp64 state / action / info widths of the six vector-state real envs; false: not one of them
static bool rsp_env_dims(int env_id, int &S, int &SD, int &A, int &INFO)
{
    switch (env_id) {
    case LENV_ENV_CARTPOLE: S = 4; SD = 4; A = 1; INFO = 0; return true;
    case LENV_ENV_ACROBOT: S = 6; SD = 4; A = 1; INFO = 0; return true;
    case LENV_ENV_MOUNTAINCAR: S = 2; SD = 4; A = 1; INFO = 0; return true;
    case LENV_ENV_PENDULUM: { using E = ContEnv<LENV_ENV_PENDULUM>; S = E::S; SD = E::SD; A = E::A; INFO = E::INFO; return true; }
    case LENV_ENV_CMC: { using E = ContEnv<LENV_ENV_CMC>; S = E::S; SD = E::SD; A = E::A; INFO = E::INFO; return true; }
    case LENV_ENV_CHEETAH_STANDIN: { using E = ContEnv<LENV_ENV_CHEETAH_STANDIN>; S = E::S; SD = E::SD; A = E::A; INFO = E::INFO; return true; }
    default: return false;
    }
}

extern "C" int lenv_rn_step_population(int32_t env_id, int32_t max_steps, int32_t type, const lenv_mlp_desc *rn, int32_t state_dim, int32_t info_dim,
                                       double gamma, const float *theta, const float *eps, const int32_t *worker, const float *sign, int64_t chains,
                                       int32_t repeat, const void *action, double *state, int32_t *elapsed, float *obs, float *reward, float *done,
                                       void *stream)
{
    RspArgs a{};
    int INFO = 0;
    if (!rsp_type_known(type)) return LENV_ERR_UNSUPPORTED;                 // reward_env.py:49,58: NotImplementedError
    if (!rsp_env_dims(env_id, a.S, a.SD, a.A, INFO)) return LENV_ERR_UNSUPPORTED;
    if (!action || !state || !elapsed || !obs || !reward || !done || chains < 0 || repeat < 1) return LENV_ERR_INVALID;
    if (eps && (!worker || !sign)) return LENV_ERR_INVALID;
    if (type != 0 && !theta) return LENV_ERR_INVALID;
    if (chains == 0) return LENV_OK;                                        // before the descriptor checks, as in lenv_se_step_population
    if (chains > 0x7fffffff || repeat > RSP_MAXREPEAT) return LENV_ERR_UNSUPPORTED;
    if (state_dim != a.S) return LENV_ERR_INVALID;
    const bool uses_info = rn_type_info_in(type) || type > 100;
    if (uses_info && (INFO == 0 || info_dim != INFO)) return LENV_ERR_INVALID;   // reward_env.py:96,113,126: ValueError('No info dict ...')
    a.env_id = env_id; a.max_steps = max_steps; a.type = type; a.info_dim = uses_info ? info_dim : 0; a.repeat = repeat; a.gamma = (float)gamma;
    if (type >= 1 && type <= 8) {
        if (!rn) return LENV_ERR_INVALID;
        const int D = rn_type_info_in(type) ? state_dim + info_dim : state_dim;
        if (rn->layers < 1 || rn->layers > 4 || rn->out_dim != 1 || rn->in_dim != D || rn->hidden < 1 || rn->hidden > RSP_MAXH || D > RSP_MAXIN) return LENV_ERR_UNSUPPORTED;
        a.H = rn->hidden; a.act = rn->act; a.prelu = rn->prelu; a.L = rn->layers; a.ln = (rn->use_layer_norm && rn->layers >= 2) ? 1 : 0;
        a.P = (int)lenv_mlp_num_params(rn);
    } else {
        a.P = type > 100 ? info_dim : 0;
    }
    a.lds_theta = (type != 0 && rn_theta_in_lds(type, a.L)) ? 1 : 0;
    a.theta = theta; a.eps = type != 0 ? eps : nullptr; a.worker = worker; a.sign = sign;
    a.action = action; a.state = state; a.elapsed = elapsed; a.obs = obs; a.reward = reward; a.done = done;
    const size_t lds_bytes = a.lds_theta ? (size_t)a.P * sizeof(float) : 0;
    const bool fly = type != 0 && !a.lds_theta && a.eps;
    const dim3 grid((unsigned)chains);
    if (a.H <= 64) {
        if (fly) return lenv_host::launch(rn_step_population_kernel<64, true>, grid, dim3(64), lds_bytes, stream, a);
        return lenv_host::launch(rn_step_population_kernel<64, false>, grid, dim3(64), lds_bytes, stream, a);
    }
    if (fly) return lenv_host::launch(rn_step_population_kernel<256, true>, grid, dim3(256), lds_bytes, stream, a);
    return lenv_host::launch(rn_step_population_kernel<256, false>, grid, dim3(256), lds_bytes, stream, a);
}
