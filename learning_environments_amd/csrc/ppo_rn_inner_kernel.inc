// ppo_rn_inner_kernel.inc -- the body of the PPO inner-loop kernel, included three times by ppo_rn_inner_loop.hip (inside namespace lenv):
//   PPO_RN_KERNEL ppo_rn_inner_kernel,    PPO_RN_SEG false: lenv_ppo_rn_inner_loop, one launch from the first episode to the final test
//   PPO_RN_KERNEL ppo_rn_segment_kernel,  PPO_RN_SEG true:  lenv_ppo_rn_inner_loop_segment, the episodes [a.ep_begin, a.ep_end)
//   PPO_RN_KERNEL ppo_icm_segment_kernel, PPO_RN_SEG true, PPO_RN_ICM true: lenv_ppo_icm_inner_loop[_segment], PPO(icm=True)
// SEG: what the loop carries from episode to episode outside the arena -- the counters, the Adam bias-correction powers, actor_old's action_std
// (LDS), the status -- is read from / written to the chain's resume record (include/lenv_hip.h); the reward net is staged by every segment, the
// agent only by the first; the closing part runs in the segment in which the chain ends.  Everything SEG adds stands under `if constexpr (SEG)`:
// ppo_rn_inner_kernel compiles to the instruction stream it had before the segments existed.  Two kernels of their own names rather than one
// template with a SEG parameter or a shared inlined body: the first would rename the kernels the other entry point launches, the second
// changes how the compiler reads the kernel arguments and with it the code of both.
// ICM (PPO.py:46-62,144-145,183-184): the chain's Intrinsic Curiosity Module (lenv_icm.cuh) lives in the arena next to a next-observation row
// buffer XN; learn() adds the intrinsic rewards of the module AS IT IS to the rows' rewards before the return scan and trains the module once,
// on all rows, after the last epoch; the module's Adam has its own step counter (resume words 22..23).  Everything ICM adds stands under
// `if constexpr (ICM)`.
template <int ENV>
__global__ __launch_bounds__(DNT) void PPO_RN_KERNEL(const PpoArgs a)
{
    constexpr bool SEG = PPO_RN_SEG;
    constexpr bool ICM = PPO_RN_ICM;
    static_assert(SEG || !ICM, "the ICM instantiation always has segment capability");
    using EnvT = ContEnv<ENV>;
    extern __shared__ __align__(16) float lds[];
    const lenv_ppo_cfg &cfg = a.cfg;
    const int tid = threadIdx.x;
    const int64_t chain = blockIdx.x;
    int64_t *rec = nullptr;
    const bool fresh = !SEG || a.ep_begin == 0;          // the arena is initialised by this launch
    if constexpr (SEG) {
        rec = a.resume + chain * LENV_PPO_RESUME_WORDS;
        if (!fresh) {                                    // uniform per chain
            if (rec[1] == 1) return;                     // finished in an earlier segment: the chain and its outputs stay as they are
            if (rec[0] != (int64_t)a.ep_begin) { if (tid == 0 && a.out.status) a.out.status[chain] = -10; return; }
        }
    }
    if (tid == 0 && a.out.status) { if (fresh) a.out.status[chain] = 0; }
    constexpr int S = EnvT::S, A = EnvT::A, SD = EnvT::SD;
    const int H = cfg.hidden, L = cfg.layers, T = cfg.test_episodes, Hrn = cfg.rn_hidden, rn_layers = cfg.rn_layers, rn_act = cfg.rn_act;
    const int N = a.N, act_id = cfg.act, info_dim = cfg.info_dim, rtype = cfg.reward_env_type;
    const float prelu = cfg.prelu;
    PpoMlp mo_actor, mo_critic;
    ppo_mlp(mo_actor, S, H, L, A);
    ppo_mlp(mo_critic, S, H, L, 1);
    const int oA = a.oA, oC = a.oC, PP = a.PP;

    // ---- LDS carve-up ----
    float *Ps = lds, *Qs = Ps + GemmShape<PP_MAXI>::PS_FLOATS;
    GemmCmd *cmds = reinterpret_cast<GemmCmd *>(Qs + GemmShape<PP_MAXI>::QS_FLOATS);
    float *rn_w = reinterpret_cast<float *>(cmds + GEMM_QUEUE_MAX);   // reward net with one hidden layer: W0 [Hrn][D] | b0 | Wout | bout
    float *rn_h = rn_w + ((a.P_rn_lds + 3) & ~3);        // [Hrn]
    float *rn_h2 = rn_h + ((Hrn + 3) & ~3);              // [Hrn]
    float *rowh = rn_h2 + ((Hrn + 3) & ~3);              // [2][PP_MAXW] hidden rows of the one-row actor
    float *misc = rowh + 2 * PP_MAXW;                    // [64]
    float *stdv = misc + 64;                             // [48]: std_old [8] | std0 [8] | stdc [8] | log(std_old) [8] | log(std0) [8] | raw actor outputs [8]
    float *state = stdv + 48;                            // [20] current observation
    float *tstate = state + 20;                          // [20] the test episode's
    float *action = tstate + 20;                         // [8]
    float *taction = action + 8;                         // [8]
    float *newrow = taction + 8;                         // [64] s | a | s' | info [4] at 2S + A + 4
    double *xs_d = reinterpret_cast<double *>((reinterpret_cast<uintptr_t>(newrow + 64) + 7) & ~(uintptr_t)7);   // [20] train env state
    double *xt_d = xs_d + 20;                            // [20] test env state
    double *ret = xt_d + 20;                             // [PP_MAXT]
    volatile float *ctrl = misc;
    volatile int *ictrl = reinterpret_cast<volatile int *>(misc + 32);
    // the control words in use: ctrl[12..17] (reward net, LayerNorm rows, the returns' mean / std), ctrl[20..21] (ICM: its Adam's bias
    // corrections), ictrl[3] = misc[35];
    // misc[MISC_STATUS_FOLD] (an int): the SEG instantiations' fold of the threads' status codes
    constexpr int MISC_STATUS_FOLD = 48;

    float *arena = a.arena + chain * a.arena_stride;
    float *params = arena + a.a_params, *adam_m = arena + a.a_m, *adam_v = arena + a.a_v, *grad = arena + a.a_grad;
    float *X = arena + a.a_x, *ACT = arena + a.a_act, *REW = arena + a.a_rew, *DONE = arena + a.a_done, *RET = arena + a.a_ret;
    float *OLDLP = arena + a.a_oldlp, *MEAN = arena + a.a_mean, *VAL = arena + a.a_val, *DZ = arena + a.a_dz, *GS = arena + a.a_gs, *DV = arena + a.a_dv;
    float *ha[PP_MAXL], *hc[PP_MAXL], *dbuf[2] = { arena + a.a_d[0], arena + a.a_d[1] };
    for (int l = 0; l < PP_MAXL; ++l) { ha[l] = arena + a.a_ha[l]; hc[l] = arena + a.a_hc[l]; }
    double *meter = reinterpret_cast<double *>(arena + a.a_meter);
    float *XN = arena + a.a_xn;                           // ICM: next observation of every row [N][S] (s' is not the next row's s
                                                         // at an episode end or with same_action_num > 1)

    // ---- stage the perturbed reward network (GTN_worker.py:165-175) and the fresh agent (PPO.py:35-44) ----
    {
        const float sg = a.eps ? a.sign[chain] : 0.0f;
        const float *e = a.eps ? a.eps + (int64_t)a.worker[chain] * a.P_rn : nullptr;
        float *dst = rn_theta_in_lds(rtype, rn_layers) ? rn_w : arena + a.a_rn;
        for (int i = tid; i < a.P_rn; i += DNT) dst[i] = e ? fma32(sg, e[i], a.theta[i]) : a.theta[i];
    }
    if (fresh) for (int p = tid; p < PP; p += DNT) { params[p] = 0.0f; adam_m[p] = 0.0f; adam_v[p] = 0.0f; grad[p] = 0.0f; }
    __syncthreads();
    if (fresh) for (int p = tid; p < a.P; p += DNT) {
        const int q = p < A ? p : (p < A + a.Pa ? oA + (p - A) : oC + (p - A - a.Pa));
        params[q] = a.agent_init[chain * a.P + p];
    }
    // fresh ICM (continuous actions: the action vector is the model input, MSE inverse loss -- icm_baseline.py:118-119)
    IcmNet icm;
    double icm_pows[2] = { 1.0, 1.0 };
    if constexpr (ICM) {
        icm_build(icm, S, A, a.icm_F, a.icm_H, /*discrete=*/false);
        float *ip = arena + a.a_icm[IB_P], *im = arena + a.a_icm[IB_M], *iv = arena + a.a_icm[IB_V];
        if (fresh) for (int p = tid; p < icm.P; p += DNT) { ip[p] = a.icm_init[chain * a.P_icm + p]; im[p] = 0.0f; iv[p] = 0.0f; }
    }
    if (tid < 64) misc[tid] = 0.0f;
    if (tid < 48) stdv[tid] = 0.0f;
    __syncthreads();
    if (fresh) { if (tid < A) stdv[tid] = params[tid]; }  // actor_old.action_std
    else if constexpr (SEG) { if (tid < A) stdv[tid] = __uint_as_float((unsigned)rec[14 + tid]); }      // ... as the last segment's act / learn left it
    __syncthreads();

    const uint64_t key = a.rng_keys ? a.rng_keys[chain] : 0;
    const bool tape = cfg.rng_mode == LENV_RNG_TAPE;
    const int k_rep = cfg.same_action_num > 1 ? cfg.same_action_num : 1;
    const float g32 = (float)cfg.gamma;
    int status = 0;
    int64_t n_actn = 0, n_testn = 0, n_test_ep = 0, time_step = 0;
    int n_rows = 0, train_steps = 0, test_steps = 0, episodes_run = 0, learn_calls = 0;
    double pows[2] = { 1.0, 1.0 };
    if constexpr (SEG) {
        if (!fresh) {                                    // every thread its copy, like the counters of a single launch
            status = (int)rec[2];
            n_actn = rec[3]; n_testn = rec[4]; n_test_ep = rec[5]; time_step = rec[6]; n_rows = (int)rec[7];
            train_steps = (int)rec[8]; test_steps = (int)rec[9]; episodes_run = (int)rec[10]; learn_calls = (int)rec[11];
            for (int i = 0; i < 2; ++i) pows[i] = __longlong_as_double(rec[12 + i]);
            if constexpr (ICM) for (int i = 0; i < 2; ++i) icm_pows[i] = __longlong_as_double(rec[22 + i]);
        }
    }
    GemmQueue gq(cmds);

    // ---- a net on ONE row: thread j owns output j of a layer (k ascending from 0, then + bias, activation); raw outputs to out (LDS) ----
    auto net_row1 = [&](const float *par, const PpoMlp &mo, const float *x, float *out) {
        const float *in = x;
        int n_in = mo.in;
        for (int l = 0; l <= mo.L; ++l) {
            const bool last = l == mo.L;
            const int n_out = last ? mo.out : mo.H;
            const float *W = par + mo.oW[l], *bb = par + mo.ob[l];
            float *h = last ? out : rowh + (l & 1) * PP_MAXW;
            for (int j = tid; j < n_out; j += DNT) {
                const float *w = W + (int64_t)j * n_in;
                float z = 0.0f;
                int k = 0;
                for (; k + 16 <= n_in; k += 16) {          // 16 weights requested before the first fmaf
                    float wv[16];
#pragma unroll
                    for (int u = 0; u < 16; ++u) wv[u] = w[k + u];
#pragma unroll
                    for (int u = 0; u < 16; ++u) z = fma32(in[k + u], wv[u], z);
                }
                for (; k < n_in; ++k) z = fma32(in[k], w[k], z);
                z = z + bb[j];
                h[j] = last ? z : act_fwd(act_id, prelu, z);
            }
            __syncthreads();
            in = h; n_in = mo.H;
        }
    };
    // Actor_PPO.forward of actor_old (actor_critic.py:45-49): std_old clamped in place to >= 0.001, a = tanh(net(s)) + z * std_old.  `idx` = the
    // row of the draw (tape row / counter index)
    auto act = [&](const float *obs, float *act_out, const float *noise, int64_t noise_rows, int64_t idx, uint32_t stream) {
        net_row1(params + oA, mo_actor, obs, stdv + 40);
        if (tid < A) {
            float sd = stdv[tid];
            if (sd < 0.001f) sd = 0.001f;
            stdv[tid] = sd;
            float zn;
            if (tape) { if (idx >= noise_rows) { status = -7; zn = 0.0f; } else zn = noise[(chain * noise_rows + idx) * A + tid]; }
            else zn = (float)det_normal(key, stream, (uint64_t)(idx * A + tid));
            act_out[tid] = det_tanhf(lenv_tanh_table, stdv[40 + tid]) + zn * sd;
        }
        __syncthreads();
    };

    // phi = reward_net(obs [| info]) -> ctrl[slot] (lenv_rn.cuh; theta sits where rn_theta_in_lds put it)
    const RnRow rn_row{ rtype, S, info_dim, Hrn, rn_layers, rn_act, cfg.rn_prelu, false, rn_theta_in_lds(rtype, rn_layers) ? rn_w : arena + a.a_rn, rn_h, rn_h2, ctrl };
    auto rn_eval = [&](const float *obs, const float *info, int slot) { wg_rn_eval(rn_row, obs, info, slot); };

    // ---- BaseAgent.test (base_agent.py:155-227) on the real env: T episodes one after the other (the reference draws their noise episode by
    // episode); in counter mode the draw of (episode, agent step) has a fixed index.  Every thread follows the env's fp64 state in LDS, so the
    // reward sum and the done flag are uniform without a hand-over.
    auto test_phase = [&]() {
        const int64_t nag = (cfg.max_steps + k_rep - 1) / k_rep;
        for (int te = 0; te < T; ++te) {
            const int64_t row = n_test_ep;
            for (int i = tid; i < SD; i += DNT) {
                double v;
                if (tape) { if (row >= a.tapes.test_reset_stride) { status = -5; v = 0.0; } else v = a.tapes.test_reset[(chain * a.tapes.test_reset_stride + row) * SD + i]; }
                else v = EnvT::reset_word(key, STREAM_TEST_RESET, row, i);
                xt_d[i] = v;
            }
            const int64_t noise0 = tape ? n_testn : n_test_ep * nag;
            int64_t used = 0;
            ++n_test_ep;
            float ep_reward = 0.0f;
            int tt = 0;
            bool dn = false;
            __syncthreads();
            for (int ta = 0; ta < cfg.max_steps && !dn; ta += k_rep) {
                if (tid < S) tstate[tid] = EnvT::obs(tid, xt_d);
                __syncthreads();
                act(tstate, taction, a.tapes.test_noise, a.tapes.test_noise_stride, noise0 + used, STREAM_PPO_TEST_NOISE);
                ++used;
                double rsum = 0.0;
                for (int r_ = 0; r_ < k_rep; ++r_) {
                    double nx = 0.0;
                    if (tid < SD) nx = EnvT::step_word(tid, xt_d, taction);
                    const double pre = EnvT::reward_pre(xt_d, taction);     // the part of the reward that sees the OLD state
                    __syncthreads();
                    if (tid < SD) xt_d[tid] = nx;
                    __syncthreads();
                    rsum = rsum + EnvT::reward_post(xt_d, pre);
                    ++tt; ++test_steps;
                    if (EnvT::done(xt_d) || tt >= cfg.max_steps) { dn = true; break; }
                }
                ep_reward = ep_reward + (float)rsum;
            }
            if (tape) n_testn += used;
            if (tid == 0) ret[te] = (double)ep_reward;
            __syncthreads();
        }
    };

    auto mlp_forward = [&](const float *par, const PpoMlp &mo, int I, float *const *hid, float *out, bool final_tanh) {
        const float *in = X;
        int n_in = mo.in;
        for (int l = 0; l < mo.L; ++l) {
            gq.gemm(in, n_in, 1, par + mo.oW[l], n_in, 1, I, mo.H, n_in, epi_bias_act(hid[l], mo.H, par + mo.ob[l], act_id, prelu));
            in = hid[l]; n_in = mo.H;
        }
        const float *W = par + mo.oW[mo.L], *bb = par + mo.ob[mo.L];
        if (final_tanh) gq.gemm(in, n_in, 1, W, n_in, 1, I, mo.out, n_in, epi_bias_tanh(out, mo.out, 0, bb, 1.0f, nullptr, 0));
        else gq.gemm(in, n_in, 1, W, n_in, 1, I, mo.out, n_in, epi_bias(out, mo.out, 0, bb));
    };
    // parameter gradients for dOut [I][out]: weight gradients reduce over the rows (r ascending), bias gradients are row-ascending sums
    auto mlp_backward = [&](const float *par, const PpoMlp &mo, int I, float *const *hid, const float *dOut, float *gpar) {
        const int Hh = mo.H, O = mo.out;
        gq.gemm(dOut, 1, O, hid[mo.L - 1], 1, Hh, O, Hh, I, epi_store(gpar + mo.oW[mo.L], Hh));
        gq.colsum(dOut, I, O, O, gpar + mo.ob[mo.L]);
        float *dcur = dbuf[0];
        gq.gemm(dOut, O, 1, par + mo.oW[mo.L], 1, Hh, I, Hh, O, epi_act_bwd(dcur, Hh, hid[mo.L - 1], Hh, act_id, prelu));
        for (int l = mo.L - 1; l >= 0; --l) {
            const int n_in = l == 0 ? mo.in : Hh;
            const float *inp = l == 0 ? X : hid[l - 1];
            gq.gemm(dcur, 1, Hh, inp, 1, n_in, Hh, n_in, I, epi_store(gpar + mo.oW[l], n_in));
            gq.colsum(dcur, I, Hh, Hh, gpar + mo.ob[l]);
            if (l > 0) {
                float *dn = dbuf[(mo.L - l) & 1];
                gq.gemm(dcur, Hh, 1, par + mo.oW[l], 1, n_in, I, n_in, Hh, epi_act_bwd(dn, n_in, hid[l - 1], n_in, act_id, prelu));
                dcur = dn;
            }
        }
    };

    // ================= PPO.learn (PPO.py:136-188) on rows [0, n) =================
    auto learn = [&](int n) {
        auto icm_step = [&]() {
            return IcmStep{ gq, Ps, Qs, arena, a.a_icm, ctrl, 20, icm, icm_pows, a.icm_lr, a.icm_beta, a.icm_eta, cfg.adam_beta1,
                            cfg.adam_beta2, cfg.adam_eps, n, X, S, XN, S, /*continuous=*/true };
        };
        auto icm_action = [&](int b, int i) { return ACT[b * A + i]; };
        // rewards += icm.compute_intrinsic_rewards(states, next_states, actions): the module as the last call left it (PPO.py:144-145)
        if constexpr (ICM) icm_rewards<PP_MAXI>(icm_step(), icm_action, [&](int b, float r) { REW[b] = REW[b] + r; });
        // discounted returns: one backward scan that restarts where done > 0.5, then (R - mean) / (std + 1e-5) with the unbiased std; the scan
        // and the two fp64 sums run left to right in thread 0 over an LDS copy of the rows' rewards / done flags (the idle staging buffer)
        for (int i = tid; i < n; i += DNT) { Ps[i] = REW[i]; Ps[PP_MAXN + i] = DONE[i]; }
        __syncthreads();
        if (tid == 0) {
            float disc = 0.0f;
            for (int i = n - 1; i >= 0; --i) {
                if (Ps[PP_MAXN + i] > 0.5f) disc = 0.0f;
                disc = Ps[i] + g32 * disc;
                Ps[i] = disc;
            }
            double sm = 0.0, sq = 0.0;
            for (int i = 0; i < n; ++i) sm += (double)Ps[i];
            const double mean = sm / (double)n;
            for (int i = 0; i < n; ++i) { const double d = (double)Ps[i] - mean; sq += d * d; }
            ctrl[16] = (float)mean; ctrl[17] = (float)__builtin_sqrt(sq / (double)(n - 1));
        }
        __syncthreads();
        {
            const float meanf = ctrl[16], stdf = ctrl[17];
            for (int i = tid; i < n; i += DNT) RET[i] = (Ps[i] - meanf) / (stdf + 1e-5f);
        }
        __syncthreads();
        PpoRowConsts rc;
        rc.inv_n = 1.0f / (float)n; rc.lo = (float)(1.0 - cfg.eps_clip); rc.hi = (float)(1.0 + cfg.eps_clip);
        rc.gent = -((float)cfg.ent_coef * rc.inv_n); rc.cv = (float)(cfg.vf_coef * 2.0 / (double)n);
        for (int it = 0; it < cfg.ppo_epochs; ++it) {
            mlp_forward(params + oA, mo_actor, n, ha, MEAN, true);
            mlp_forward(params + oC, mo_critic, n, hc, VAL, false);
            gq.run<PP_MAXI>(Ps, Qs);
            // evaluate's clamp of action_std to >= 0.01 comes after the log-probabilities: they see std0, the entropy and autograd's saved
            // tensors stdc, and the parameter keeps stdc
            if (tid < A) {
                const float s0 = params[tid], sc = s0 < 0.01f ? 0.01f : s0;
                params[tid] = sc;
                stdv[8 + tid] = s0; stdv[16 + tid] = sc;
                stdv[24 + tid] = (float)det_log((double)stdv[tid]); stdv[32 + tid] = (float)det_log((double)s0);
            }
            __syncthreads();
            {
                float so[A], lo_[A], s0[A], l0[A], sc[A];
#pragma unroll
                for (int k = 0; k < A; ++k) { so[k] = stdv[k]; s0[k] = stdv[8 + k]; sc[k] = stdv[16 + k]; lo_[k] = stdv[24 + k]; l0[k] = stdv[32 + k]; }
                for (int i = tid; i < n; i += DNT) {
                    float av[A], mv[A], dz[A], gs[A], dv;
#pragma unroll
                    for (int k = 0; k < A; ++k) { av[k] = ACT[i * A + k]; mv[k] = MEAN[i * A + k]; }
                    float olp;
                    if (it == 0) { olp = ppo_logprob<A>(av, mv, so, lo_); OLDLP[i] = olp; }      // old_logprobs: the same net, actor_old's own std
                    else olp = OLDLP[i];
                    ppo_row_grads<A>(rc, av, mv, s0, l0, sc, olp, RET[i], VAL[i], dz, gs, dv);
#pragma unroll
                    for (int k = 0; k < A; ++k) { DZ[i * A + k] = dz[k]; GS[i * A + k] = gs[k]; }
                    DV[i] = dv;
                }
            }
            __syncthreads();
            gq.colsum(GS, n, A, A, grad);
            mlp_backward(params + oA, mo_actor, n, ha, DZ, grad + oA);
            mlp_backward(params + oC, mo_critic, n, hc, DV, grad + oC);
            gq.run<PP_MAXI>(Ps, Qs);
            // torch.optim.Adam, one step counter for all parameters
            pows[0] *= cfg.adam_beta1; pows[1] *= cfg.adam_beta2;
            const AdamConsts ac{ (float)(-(cfg.lr / (1.0 - pows[0]))), (float)__builtin_sqrt(1.0 - pows[1]), (float)(1.0 - cfg.adam_beta1),
                                 (float)(1.0 - cfg.adam_beta2), (float)cfg.adam_beta2, (float)cfg.adam_eps };
            wg_adam(params, adam_m, adam_v, grad, 0, PP, ac, nullptr, 0.0f, 0.0f);
            __syncthreads();
        }
        if constexpr (ICM) icm_train<PP_MAXI>(icm_step(), icm_action);      // icm.train(states, next_states, actions) (PPO.py:183-184)
        if (tid < A) stdv[tid] = params[tid];             // actor_old.load_state_dict(actor.state_dict())
        if (a.out.learn_step && learn_calls < a.out.learn_cap) {
            const int64_t k = chain * a.out.learn_cap + learn_calls;
            if (tid == 0) a.out.learn_step[k] = train_steps;
            if (a.out.learn_params) {
                for (int p = tid; p < a.P; p += DNT) {
                    const int q = p < A ? p : (p < A + a.Pa ? oA + (p - A) : oC + (p - A - a.Pa));
                    a.out.learn_params[k * a.P + p] = params[q];
                }
            }
        }
        ++learn_calls;
        __syncthreads();
    };

    bool early_out = false;                               // SEG: the loop ended at the early out
    const int ep_first = SEG ? a.ep_begin : 0, ep_last = SEG ? a.ep_end : cfg.train_episodes;
    for (int episode = ep_first; episode < ep_last; ++episode) {
        // env.reset(): RewardEnv.reset -> real_env.reset() (reward_env.py:141-143)
        for (int i = tid; i < SD; i += DNT) {
            double v;
            if (tape) { if (episode >= a.tapes.train_reset_stride) { status = -5; v = 0.0; } else v = a.tapes.train_reset[(chain * a.tapes.train_reset_stride + episode) * SD + i]; }
            else v = EnvT::reset_word(key, STREAM_TRAIN_RESET, (int64_t)episode, i);
            xs_d[i] = v;
        }
        __syncthreads();
        if (tid < S) state[tid] = EnvT::obs(tid, xs_d);
        __syncthreads();
        if (rtype == 1 || rtype == 2) rn_eval(state, nullptr, 12);   // phi(s) of the reset state (carried from step to step)
        int ep_len = 0, env_steps = 0;
        for (int t = 0; t < cfg.max_steps; t += k_rep) {         // PPO.py:83 range(0, max_episode_steps, same_action_num)
            time_step += k_rep;
            act(state, action, a.tapes.act_noise, a.tapes.act_noise_stride, n_actn, STREAM_PPO_ACT_NOISE);
            ++n_actn;
            // ---- EnvWrapper.step -> RewardEnv.step -> real_env.step + TimeLimit, same_action_num times or until done; the shaped rewards of
            // the repeats are summed as python floats (env_wrapper.py:56-61); `state` follows the repeats ----
            if (tid < S) newrow[tid] = state[tid];
            if (tid >= 64 && tid < 64 + A) newrow[S + tid - 64] = action[tid - 64];
            double rsum = 0.0;
            bool dn = false;
            for (int r_ = 0; r_ < k_rep; ++r_) {
                double nx = 0.0;
                if (tid < SD) nx = EnvT::step_word(tid, xs_d, action);
                const double pre = EnvT::reward_pre(xs_d, action);      // the part of the reward that sees the OLD state (every thread: uniform)
                __syncthreads();
                if (tid < SD) xs_d[tid] = nx;
                __syncthreads();
                ++env_steps;
                dn = EnvT::done(xs_d) || env_steps >= cfg.max_steps;    // the env's own flag or TimeLimit (uniform)
                if (tid < S) newrow[S + A + tid] = EnvT::obs(tid, xs_d);
                float *info = newrow + 2 * S + A + 4;                   // [4] info vector of this step (fp32, as torch.tensor(list(info.values())))
                if constexpr (EnvT::INFO == 4) {
                    if (tid == 64 && rtype >= 3) cheetah_info_row(info, xs_d, pre);
                }
                __syncthreads();
                if (rtype == 3 || rtype == 4) rn_eval(state, info, 12);  // phi([s | info]): not cacheable, info is this step's
                rn_eval(newrow + S + A, info, 13);                      // phi(s') / phi([s' | info]) / w . info
                {
                    const float r32 = (float)EnvT::reward_post(xs_d, pre), phi_s = ctrl[12], phi_s2 = ctrl[13];
                    const float shaped = rn_shaped_reward(rtype, r32, g32, phi_s, phi_s2);
                    rsum = rsum + (double)shaped;
                    __syncthreads();                                    // every thread has read ctrl[12] / ctrl[13]
                    if (tid == 0) ctrl[12] = phi_s2;
                }
                if (tid < S) state[tid] = newrow[S + A + tid];           // RewardEnv.state = next_state
                __syncthreads();
                if (dn) break;
            }
            // replay_buffer.add: the on-policy row (s, a, r, done)
            const float shaped_sum = (float)rsum, done_f = dn ? 1.0f : 0.0f;
            if (n_rows < N) {
                if (tid < S) X[n_rows * S + tid] = newrow[tid];
                if (tid >= 64 && tid < 64 + A) ACT[n_rows * A + tid - 64] = newrow[S + tid - 64];
                if (tid == 128) { REW[n_rows] = shaped_sum; DONE[n_rows] = done_f; }
                if constexpr (ICM) { if (tid >= 192 && tid < 192 + S) XN[n_rows * S + tid - 192] = newrow[S + A + tid - 192]; }
                ++n_rows;
            } else status = -4;
            if (a.out.trace_reward && train_steps < a.out.trace_cap) {
                const int64_t k = chain * a.out.trace_cap + train_steps;
                if (tid < S) { a.out.trace_state[k * S + tid] = newrow[tid]; a.out.trace_next_state[k * S + tid] = newrow[S + A + tid]; }
                if (tid < A) a.out.trace_action[k * A + tid] = newrow[S + tid];
                if (tid == 0) { a.out.trace_reward[k] = shaped_sum; if (a.out.trace_done) a.out.trace_done[k] = done_f; }
            }
            ep_len += k_rep; ++train_steps;
            __syncthreads();
            if ((double)time_step / (double)cfg.max_steps > cfg.update_episodes) {      // PPO.py:100 (a float comparison)
                learn(n_rows);
                n_rows = 0; time_step = 0;
            }
            if (dn) break;
        }
        ++episodes_run;
        if (tid == 0 && a.out.episode_len) a.out.episode_len[chain * cfg.train_episodes + episode] = ep_len;
        test_phase();                                      // per-episode test on the real env (PPO.py:110-112)
        if (tid == 0) {
            double sm = 0.0;
            for (int i = 0; i < T; ++i) sm += ret[i];
            const double tm = sm / (double)T;
            meter[episode] = tm;
            if (a.out.episode_test_mean) a.out.episode_test_mean[chain * cfg.train_episodes + episode] = tm;
            // early out (PPO.py:117-124, base_agent.py:49-62): break_env = the real env, the real rule
            ictrl[3] = episode >= cfg.init_episodes && meter_env_solved(meter, episode + 1, cfg.early_out_num, false, cfg.solved_reward, 0.0, episode, cfg.init_episodes);
        }
        __syncthreads();
        const int brk = ictrl[3];
        __syncthreads();
        if (brk) { if constexpr (SEG) early_out = true; break; }
    }
    if constexpr (SEG) {
        if (!early_out && a.ep_end < cfg.train_episodes) {
            // the chain goes on in the next segment: a checkpoint (cumulative stats, the parameters so far) and the record
            int *st_fold = reinterpret_cast<int *>(misc + MISC_STATUS_FOLD);     // the minimum of the threads' status codes (0 after the clear of misc)
            if (status != 0) { atomicMin(st_fold, status); if (a.out.status) atomicMin(&a.out.status[chain], status); }
            if (a.out.final_params) {
                for (int p = tid; p < a.P; p += DNT) {
                    const int q = p < A ? p : (p < A + a.Pa ? oA + (p - A) : oC + (p - A - a.Pa));
                    a.out.final_params[chain * a.P + p] = params[q];
                }
            }
            if constexpr (ICM) {
                if (a.icm_final) for (int p = tid; p < icm.P; p += DNT) a.icm_final[chain * a.P_icm + p] = arena[a.a_icm[IB_P] + p];
            }
            __syncthreads();
            if (tid == 0) {
                if (a.out.stats) {
                    a.out.stats[chain * 4 + 0] = episodes_run; a.out.stats[chain * 4 + 1] = train_steps;
                    a.out.stats[chain * 4 + 2] = learn_calls; a.out.stats[chain * 4 + 3] = test_steps;
                }
                ppo_write_record(rec, a.ep_end, 0, *st_fold, n_actn, n_testn, n_test_ep, time_step, n_rows, train_steps, test_steps, episodes_run,
                                 learn_calls, pows, stdv);
                if constexpr (ICM) for (int i = 0; i < 2; ++i) rec[22 + i] = __double_as_longlong(icm_pows[i]);
            }
            return;
        }
    }
    test_phase();
    if (tid == 0) {
        double sm = 0.0;
        for (int i = 0; i < T; ++i) sm += ret[i];
        a.out.score[chain] = sm / (double)T;
        if (a.out.final_returns) for (int i = 0; i < T; ++i) a.out.final_returns[chain * T + i] = ret[i];
        if (a.out.stats) {
            a.out.stats[chain * 4 + 0] = episodes_run; a.out.stats[chain * 4 + 1] = train_steps;
            a.out.stats[chain * 4 + 2] = learn_calls; a.out.stats[chain * 4 + 3] = test_steps;
        }
        for (int e = episodes_run; e < cfg.train_episodes; ++e) {      // episodes that never ran: NaN / 0
            if (a.out.episode_test_mean) a.out.episode_test_mean[chain * cfg.train_episodes + e] = __builtin_nan("");
            if (a.out.episode_len) a.out.episode_len[chain * cfg.train_episodes + e] = 0;
        }
    }
    if (a.out.final_params) {
        for (int p = tid; p < a.P; p += DNT) {
            const int q = p < A ? p : (p < A + a.Pa ? oA + (p - A) : oC + (p - A - a.Pa));
            a.out.final_params[chain * a.P + p] = params[q];
        }
    }
    if constexpr (ICM) {
        if (a.icm_final) for (int p = tid; p < icm.P; p += DNT) a.icm_final[chain * a.P_icm + p] = arena[a.a_icm[IB_P] + p];
    }
    if (a.out.status && status != 0) atomicMin(&a.out.status[chain], status);
    if constexpr (SEG) {
        int *st_fold = reinterpret_cast<int *>(misc + MISC_STATUS_FOLD);
        if (status != 0) atomicMin(st_fold, status);
        __syncthreads();
        if (tid == 0) {
            ppo_write_record(rec, a.ep_end, 1, *st_fold, n_actn, n_testn, n_test_ep, time_step, n_rows, train_steps, test_steps, episodes_run,
                             learn_calls, pows, stdv);
            if constexpr (ICM) for (int i = 0; i < 2; ++i) rec[22 + i] = __double_as_longlong(icm_pows[i]);
        }
    }
}
