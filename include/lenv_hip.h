/*
 * lenv_hip.h -- C-ABI of liblenv_hip.so: the MI355X (gfx950) implementation of the NES
 * inner-loop hot path of automl/learning_environments.
 *
 * The reference has no FFI; its boundary for this path is the Python object API
 * (envs/env_wrapper.py:16-70 EnvWrapper.step, agents/GTN_worker.py:76-108 GTN_Worker.run,
 * agents/GTN_master.py:81-116 GTN_Master.run).  These entry points are what a ctypes binding
 * added to those Python classes calls (INTEGRATION.md shows the stubs).  Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller unless marked HOST;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous
 *     on that stream, never allocate, never synchronise, and are graph-capturable;
 *   - return value: 0 = ok, negative = LENV_ERR_* (no exceptions cross the ABI);
 *   - no internal threads, no global mutable state, no environment variables: everything that steers a launch is in its cfg;
 *     re-entrant per stream.
 *
 * Flat parameter layout of an MLP (models/model_utils.py:4-39), identical to the reference's
 * state-dict order with PReLU slopes removed: W0[H,in] b0[H] {W_l[H,H] b_l[H]} Wout[out,H] bout[out].
 * SE theta = state_net | reward_net | done_net (envs/virtual_env.py:23-31).
 */
#ifndef LENV_HIP_H
#define LENV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LENV_ABI_VERSION 7

enum {
    LENV_OK = 0,
    LENV_ERR_INVALID = -1,      /* bad argument / inconsistent sizes */
    LENV_ERR_UNSUPPORTED = -2,  /* shape or option outside what the kernels implement (NotImplementedError) */
    LENV_ERR_WORKSPACE = -3,    /* workspace too small */
    LENV_ERR_LAUNCH = -4,       /* HIP launch failed (hipGetLastError) */
    LENV_ERR_NO_DEVICE = -5
};

enum { LENV_ACT_IDENTITY = 0, LENV_ACT_RELU = 1, LENV_ACT_LEAKYRELU = 2, LENV_ACT_TANH = 3, LENV_ACT_PRELU = 4 };
enum { LENV_ENV_CARTPOLE = 0, LENV_ENV_ACROBOT = 1, LENV_ENV_CHEETAH_STANDIN = 2, LENV_ENV_MOUNTAINCAR = 3, LENV_ENV_PENDULUM = 4, LENV_ENV_CMC = 5 };
enum { LENV_RNG_COUNTER = 0, LENV_RNG_TAPE = 1 };
/* lenv_ddqn_cfg / lenv_td3_cfg `kernel_variant` bits (0 = the fastest kernel that takes the launch; the bits exist for A/B timing and for
 * the parity tests that hold the kernels against each other -- every variant produces the same bits):
 * NO_WAVECHAIN keeps the GEMM-queue kernel where a wave-chain kernel exists, GENERIC skips the shape-specialised instantiations,
 * TEAM_NARROW keeps whole forward items per lane in DDQN teams of three and more (default there: every item cut over the idle lanes),
 * NO_EARLY_GRAD keeps the published CartPole DDQN shape on the pass-major forward deal with one workgroup barrier between the minibatch
 * forward and the gradient (default there: chunk-aligned deal, a gradient chunk starts when the waves that hold its items are done). */
enum { LENV_VARIANT_NO_WAVECHAIN = 1, LENV_VARIANT_GENERIC = 2, LENV_VARIANT_TEAM_NARROW = 4,
       LENV_VARIANT_NO_DIRECT = 8,     /* NO_DIRECT: the GEMM-queue kernels keep narrow nets on the product queue too (A/B timing, kernel-vs-kernel tests) */
       LENV_VARIANT_NO_EARLY_GRAD = 16 };
/* lenv_inner_out::status of a chain whose gradient wave gave up waiting for the "forward done" tags of its chunk's waves (the bounded
 * wait of the early-gradient DDQN instantiation: an internal error, no correct run reaches the budget) */
enum { LENV_STATUS_EARLY_GRAD_WAIT = -11 };

/* models/model_utils.py:4-39 */
typedef struct {
    int32_t in_dim, hidden, layers, out_dim, act;
    float prelu;
    /* `use_layer_norm` of models/model_utils.py:22-37: ONE shared nn.LayerNorm(hidden) (eps 1e-5) after every hidden Linear but
     * the first, before the activation; its weight and bias [hidden] follow the second Linear in the flat vector
     * (Module.parameters() order).  Honoured by lenv_mlp_num_params / lenv_mlp_forward / lenv_se_step_population (the three SE nets of
     * a VirtualEnv.step).  The fused loops take the AGENT's LayerNorm through their own cfg fields (lenv_ddqn_cfg::q_layer_norm,
     * lenv_td3_cfg::use_layer_norm, lenv_td3d_cfg::use_layer_norm); the synthetic env's nets inside the DDQN /
     * DuelingDDQN loop: lenv_ddqn_cfg::se_layer_norm; the TD3-family and tabular loops: rn_layer_norm / se_layer_norm of their cfgs). */
    int32_t use_layer_norm;
} lenv_mlp_desc;

/* agents/DDQN.py:15-38, agents/base_agent.py:9-26, envs/env_factory.py:45-59 */
typedef struct {
    int32_t env_id;
    int32_t state_dim;
    int32_t num_actions;
    int32_t max_steps;
    int32_t se_hidden, se_layers, se_act;
    float se_prelu;
    int32_t q_hidden, q_layers, q_act;
    float q_prelu;
    int32_t batch_size, rb_size;
    int32_t train_episodes, test_episodes, init_episodes;
    int32_t early_out_num;
    int32_t grad_chunk;   /* samples per gradient micro-chunk; 0 = ceil(batch/16) */
    int32_t rng_mode;
    int32_t agent_kind;   /* 0 = DDQN (agents/DDQN.py), 1 = DuelingDDQN (agents/DuelingDDQN.py) */
    int32_t feature_dim;  /* DuelingDDQN: width of the feature vector / of the two head hidden layers */
    double solved_reward;
    double gamma, lr, tau;
    double eps_init, eps_min, eps_decay;
    double adam_beta1, adam_beta2, adam_eps;
    /* Deterministic stand-in for the wall-clock time-out of BaseAgent.train/test (agents/base_agent.py:30-47,90-97,177-184):
     * "elapsed" = env steps (train + test) this chain has taken.  <= 0: no budget.  At the start of a training episode with
     * elapsed > step_budget the per-episode reward list is padded with its minimum so far (-1e9 if empty) and training
     * stops; the final test gets the remainder and pads its returns the same way (so a chain that timed out in training
     * scores -1e9, as the reference does).  All four fused inner loops implement it. */
    int64_t step_budget;
    /* Intrinsic Curiosity Module inside learn() (select_agent "ddqn_icm" / "duelingddqn_icm": agents/DDQN.py:40-58,74-76,
     * models/icm_baseline.py:8-172; config section `icm`).  icm_enabled != 0: every learn step first trains the ICM on the
     * minibatch (one Adam step with icm_lr) and adds eta * mean_f (features(s') - forward(s, a))^2 to the minibatch rewards.
     * Only lenv_dueling_se_inner_loop_icm takes such a cfg (GEMM-tiled kernel; fresh ICM parameters per chain). */
    int32_t icm_enabled, icm_feature_dim, icm_hidden;
    /* `use_layer_norm` of the ENV's config section with se_layers >= 2 (models/model_utils.py:22-37): the shared nn.LayerNorm behind hidden
     * Linear 2..L of each of the three SE nets (synthetic_env_type 1: of the reward net).  NES perturbs and updates nn.Linear parameters only (agents/GTN_worker.py:156-175,
     * agents/GTN_master.py:281-296): the module keeps its initial affine (weight 1, bias 0) and theta stays the Linear parameters.
     * GEMM-tiled kernel only (lenv_dueling_se_inner_loop*); nothing to do with one hidden layer. */
    int32_t se_layer_norm;
    double icm_lr, icm_beta, icm_eta;
    /* gtn.synthetic_env_type: 0 = the agent trains on the VirtualEnv (theta = the three SE nets); 1 = on a RewardEnv over the
     * REAL env (envs/reward_env.py:61-133, default_config_cartpole_reward_env.yaml): real transitions, reward through the
     * reward network theta (state_dim -> se_hidden x se_layers -> 1, se_act; a 1-input dummy for type 0), reward_env_type 0, 1, 2, 5 or 6
     * (the real CartPole / Acrobot step carries no info vector).  GEMM-tiled kernel only (lenv_dueling_se_inner_loop*). */
    int32_t synthetic_env_type, reward_env_type;
    /* same_action_num (agents/base_agent.py:20,104,194; envs/env_wrapper.py:24-29,56-61): env steps per chosen action -- a VirtualEnv
     * repeats the step whatever the done flag says and sums the fp32 rewards, a real env's repeats stop at done (python-float sum);
     * 0 and 1 both mean 1.  Values > 1: GEMM-tiled kernel only (lenv_dueling_se_inner_loop*, plain-DQN mode for DDQN). */
    int32_t same_action_num;
    /* Workgroups per chain (a TEAM: the members split the minibatch / the gradient tiles of a learn step and meet at barriers; same
     * bits for every size).  0 = automatic: the largest team for which every workgroup of the launch is resident at once on an
     * otherwise idle device (checked with the occupancy API at launch); 1 = one workgroup per chain; G > 1 = at most G.  A launch
     * whose members cannot all be resident is never made with a team (the entry falls back to 1).  Team launches need the device to
     * themselves: a member that waits longer than ~0.25 s for the others (another kernel holds the CUs) gives up, every chain of the
     * launch reports status -10 within that time, and the caller repeats the launch with team_size 1 (engine.py does). */
    int32_t team_size;
    int32_t kernel_variant;   /* LENV_VARIANT_* bits, 0 = fastest */
    /* `use_layer_norm` of the agent's config section (models/model_utils.py:22-37): ONE shared nn.LayerNorm(hidden) (eps 1e-5) behind every
     * hidden Linear but the first of the Q-net (agent_kind 0) / of the DuelingDDQN's feature stream (its heads have one hidden layer: none
     * there); its weight | bias sit behind the second Linear in the parameter vector (Module.parameters() order), fresh agents start them at
     * 1 | 0.  Nothing to do with one hidden layer.  GEMM-tiled kernel (lenv_dueling_se_inner_loop*); forward and backward in the loop. */
    int32_t q_layer_norm;
    /* ABI 7.  test_mode = which BaseAgent.train call the loop is (agents/base_agent.py:64,134-148):
     *   0 = train(env, test_env=real_env), GTN_Worker.calc_score (agents/GTN_worker.py:195-199): test_episodes real-env test episodes after
     *       every training episode feed the meter; early-out = the real rule on it (mean of the last early_out_num entries >= solved_reward);
     *   1 = train(env, test_env=None), what every downstream evaluation calls (experiments/syn_env_evaluate_cartpole_vary_hp_2.py:38-41):
     *       NO per-episode tests; the meter is fed by the training env's own episode reward (the fp32 sum of the step rewards,
     *       base_agent.py:121,138); break_env = the training env (:141-146): a VirtualEnv stops on
     *       |avg - avg_last| / (|avg_last| + 1e-9) < early_out_virtual_diff once episode >= init_episodes + early_out_num
     *       (base_agent.py:49-56; AverageMeter.get_mean_last, utils.py:97-105), a RewardEnv / the real env (synthetic_env_type 1) on
     *       avg >= solved_reward.  out->episode_test_mean[] then holds the training episode rewards (the function's reward_train list);
     *       the final test and the score are unchanged.  Training on the REAL env (experiments/syn_env_run_vary_hp.py:47-54, mode 0) =
     *       synthetic_env_type 1 with reward_env_type 0 (envs/reward_env.py:80-81: the real reward passes through; theta is not read). */
    int32_t test_mode;
    double early_out_virtual_diff;
} lenv_ddqn_cfg;

/* RNG tapes (parity mode).  Per-chain rows: element [c*stride + n]; all DEVICE pointers. */
typedef struct {
    const double *eps_uniform;  int64_t eps_uniform_stride;   /* random.random()         agents/DDQN.py:98 */
    const int32_t *rand_action; int64_t rand_action_stride;   /* action_space.sample()   envs/env_wrapper.py:88 */
    const int32_t *replay_idx;  int64_t replay_idx_stride;    /* np.random.randint       utils.py:35 */
    const double *train_reset;  int64_t train_reset_stride;   /* rows of 4 doubles       envs/virtual_env.py:36 */
    const double *test_reset;   int64_t test_reset_stride;    /* rows of 4 doubles */
} lenv_tapes;

/* Outputs of the fused inner loop; every pointer may be NULL except `score`. */
typedef struct {
    double *score;              /* [chains] statistics.mean(final test returns)   GTN_worker.py:209 */
    int64_t *stats;             /* [chains,4] episodes_run, train_steps, learn_steps, test_steps */
    int32_t *status;            /* [chains] 0 ok, <0 internal error: -2..-5 tape underrun (eps / action / replay / reset), -6 replay index out of range, -7 unexpected LDS placement, -8 per-chain hyper-parameter outside cfg's maxima, -10 a team member gave up (team_size), -11 LENV_STATUS_EARLY_GRAD_WAIT */
    double *episode_test_mean;  /* [chains,train_episodes]  reward_list_train (NaN past early-out) */
    int32_t *episode_len;       /* [chains,train_episodes] */
    double *final_returns;      /* [chains,test_episodes] */
    float *final_online;        /* [chains,P_agent] trained Q-net (canonical flat layout) */
    /* optional per-step trace, rows [chains,trace_cap] */
    int64_t trace_cap;
    int32_t *trace_action;      /* action | explored<<16 */
    float *trace_state;         /* [chains,trace_cap,S] */
    float *trace_next_state;    /* [chains,trace_cap,S] */
    float *trace_reward_done;   /* [chains,trace_cap,2] */
} lenv_inner_out;

int lenv_abi_version(void);
/* sizeof of the ABI structs as the library was compiled (a binding checks its mirror against it): which = 0 lenv_mlp_desc, 1 lenv_ddqn_cfg,
 * 2 lenv_ql_cfg, 3 lenv_td3_cfg, 4 lenv_td3d_cfg, 5 lenv_tapes, 6 lenv_inner_out, 7 lenv_ql_out, 8 lenv_td3_tapes, 9 lenv_td3_out,
 * 10 lenv_td3d_tapes, 11 lenv_chain_hp, 12 lenv_icm_io, 13 lenv_td3d_rn_cfg, 14 lenv_ppo_cfg, 15 lenv_ppo_tapes, 16 lenv_ppo_out; anything else:
 * LENV_ERR_INVALID.  HOST. */
int64_t lenv_struct_size(int32_t which);
const char *lenv_error_string(int code);
/* number of parameters of an MLP / of the three-net SE */
int64_t lenv_mlp_num_params(const lenv_mlp_desc *d /*HOST*/);

/*
 * Population-batched VirtualEnv step: replaces EnvWrapper.step -> VirtualEnv.step
 * (envs/env_wrapper.py:16-47, envs/virtual_env.py:43-54) for `chains` perturbed SEs at once,
 * W_c = theta + sign[c]*eps[worker[c]] (agents/GTN_worker.py:165-175; eps may be NULL).
 * state [chains,n_per_chain,S], action [chains,n_per_chain] (index), outputs same leading shape.
 */
int lenv_se_step_population(const lenv_mlp_desc *state_net /*HOST*/, const lenv_mlp_desc *reward_net /*HOST*/,
                            const lenv_mlp_desc *done_net /*HOST*/, const float *theta, const float *eps,
                            const int32_t *worker, const float *sign, int64_t chains, int32_t n_per_chain,
                            const float *state, const int32_t *action, float *next_state, float *reward,
                            float *done, void *stream);

/*
 * The same step for ACTION VECTORS (the continuous-action SEs: Pendulum, MountainCarContinuous, HalfCheetah), with the `same_action_num`
 * repeat of EnvWrapper.step's virtual branch (envs/env_wrapper.py:28-30) inside the launch.  Descriptor checks, eps == NULL, the LayerNorm
 * layout and the raw done-net output as in lenv_se_step_population.  action [chains,n_per_chain,A] is the row the nets see (input row =
 * [action | state], envs/virtual_env.py:43-54; a one-hot row gives lenv_se_step_population's bits).  repeat >= 1 (else LENV_ERR_INVALID):
 * that many SE steps with the same action, each fed the previous next state; reward = the fp32 sum left to right, next_state / done of the
 * last step, no break on done.  Every element of W_c is fmaf(sign[c], eps[worker[c]][i], theta[i]); every dot product the canonical order.
 * Two kernels: W_c resident in LDS when it fits 160 KiB in the padded layout of the kernel (rows of round8(n_in) + 4 floats) next to the
 * buffers of one block of 8 rows -- ask lenv_se_step_vec_path rather than estimating it --, else streamed through LDS in K-panels against
 * blocks of rows (a weight leaves HBM once per chain, repeat and block of 8 / 16 / 32 rows).  chains == 0 returns LENV_OK after the
 * pointer checks, like lenv_se_step_population; chains >= 2^31 is LENV_ERR_UNSUPPORTED.  Takes every shape lenv_mlp_forward takes with
 * hidden <= 256, layers 1..3 and S + A <= 256; beyond that LENV_ERR_UNSUPPORTED.
 */
int lenv_se_step_population_vec(const lenv_mlp_desc *state_net /*HOST*/, const lenv_mlp_desc *reward_net /*HOST*/,
                                const lenv_mlp_desc *done_net /*HOST*/, const float *theta, const float *eps,
                                const int32_t *worker, const float *sign, int64_t chains, int32_t n_per_chain, int32_t repeat,
                                const float *state, const float *action, float *next_state, float *reward,
                                float *done, void *stream);
/* HOST: which kernel that launch runs: 0 = resident, 1 = streaming, or a negative LENV_ERR_* (the launch's own checks). */
int32_t lenv_se_step_vec_path(const lenv_mlp_desc *state_net /*HOST*/, const lenv_mlp_desc *reward_net /*HOST*/,
                              const lenv_mlp_desc *done_net /*HOST*/, int32_t n_per_chain);

/*
 * DDQN TD forward over replay minibatches (agents/DDQN.py:63-85): for every chain, gathers rows
 * idx[c,b] of its replay buffer (row = [s(S), a, s'(S), r, done], stride row_stride floats) and writes
 * q_sa[c,b] = Q(s)[a], y[c,b] = r + gamma * Q_target(s')[argmax Q(s')] * (1 - done).
 * online/target: [chains,P_agent] flat Critic_DQN parameters (models/actor_critic.py:84-91).
 */
int lenv_qnet_td_forward(const lenv_mlp_desc *qnet /*HOST*/, const float *online, const float *target,
                         const float *replay, int64_t replay_cap, int32_t row_stride, const int32_t *idx,
                         int64_t chains, int32_t batch, double gamma, float *q_sa, float *y, void *stream);

/*
 * Fused inner loop = GTN_Worker.calc_score (agents/GTN_worker.py:187-221) for `chains` independent
 * chains, one workgroup per chain: fresh DDQN agent (agent_init [chains,P_agent]), BaseAgent.train on the
 * perturbed SE with per-episode real-env tests and early-out (agents/base_agent.py:64-153), final
 * BaseAgent.test (agents/base_agent.py:155-227).  rng_keys [chains] (counter mode) / tapes (tape mode).
 * The replay buffers, the per-episode meter and the Adam bias-correction table (8 B per possible learn step, filled by a
 * prologue kernel on `stream`) live in `workspace` (lenv_ddqn_se_workspace_bytes): the entry allocates nothing.
 */
size_t lenv_ddqn_se_workspace_bytes(const lenv_ddqn_cfg *cfg /*HOST*/, int64_t chains);
/* LDS bytes one chain needs for this cfg (incl. grad_chunk), or a negative LENV_ERR_* when unsupported / > 160 KiB */
int64_t lenv_ddqn_se_lds_bytes(const lenv_ddqn_cfg *cfg /*HOST*/);
/* How the minibatch forward of this cfg is laid out (diagnostic, host only): *items = forward items (sample, pass) that spill
 * beyond the first eight waves of the workgroup, *parts = the number of pieces each of them is cut into over the hidden-unit pairs
 * (0 = plain layout: nothing spills, too much spills, the net is too narrow to cut, or the shared rows do not fit LDS). */
int lenv_ddqn_se_forward_split(const lenv_ddqn_cfg *cfg /*HOST*/, int32_t *items, int32_t *parts);
/* The chunk-aligned deal of the forward items of the early-gradient instantiation (diagnostic, host only, no device call): for a cfg that a
 * counter-mode launch with one workgroup per chain and without a step trace runs on that instantiation (the published CartPole shape,
 * kernel_variant without GENERIC / NO_EARLY_GRAD, VirtualEnv, test_mode 0) the return value is the number of gradient chunks n > 0,
 * item_of_lane[t] (768 words, one per thread of the workgroup) = pass * batch_size + sample of the forward item whose output layer thread t
 * runs -- a whole item on the first eight waves, the chain of a spilled item (always pass 2) on the lanes behind them -- or -1, and
 * chunk_wave_mask[c] (n words) = bit w set when wave w = t / 64 holds an item of a sample of chunk c: the waves whose "forward done" tags
 * the gradient of chunk c waits for.  Every other cfg: 0 = no early gradient, nothing is written.  Negative: LENV_ERR_*. */
int lenv_ddqn_se_forward_deal(const lenv_ddqn_cfg *cfg /*HOST*/, int32_t *item_of_lane, int32_t *chunk_wave_mask);
/* Workgroups per chain lenv_ddqn_se_inner_loop would use for a counter-mode launch of `chains` chains on the current device: > 1 when
 * the launch leaves enough CUs idle for every member of every chain to be resident (shards of a population spread over several
 * GPUs); the members deal the minibatch by whole gradient micro-chunks and meet once per learn step -- same bits for every team
 * size.  cfg->team_size caps / forces the size (1 = never).  Status -10 = a member gave up waiting (see team_size). */
int lenv_ddqn_se_team_size(const lenv_ddqn_cfg *cfg /*HOST*/, int64_t chains);
int lenv_ddqn_se_inner_loop(const lenv_ddqn_cfg *cfg /*HOST*/, const float *theta, const float *eps,
                            const int32_t *worker, const float *sign, const float *agent_init,
                            const uint64_t *rng_keys, const lenv_tapes *tapes /*HOST struct of device ptrs, may be NULL*/,
                            int64_t chains, void *workspace, size_t workspace_bytes,
                            const lenv_inner_out *out /*HOST struct of device ptrs*/, void *stream);

/*
 * Config 4: fused inner loop for the tabular agents (Q-learning, SARSA, and their count-based variants) on a potential-shaped
 * RewardEnv over a grid MDP (agents/QL.py:13-106, agents/SARSA.py:12-91, envs/reward_env.py:61-133, envs/gridworld.py:38-110), one wave per chain.
 * The MDP is given as transition tables next_state/reward/done [n_states, n_actions] (device pointers, shared by all
 * chains); theta = flat reward_net parameters (PReLU slope excluded), perturbed per chain as theta + sign*eps[worker].
 * shaped_override [n_states*n_actions] (optional) replaces the reward-net evaluation by a given shaped-reward table.
 */
typedef struct {
    int32_t n_states, n_actions, start_state, max_steps;
    int32_t rn_hidden, rn_layers, rn_act;
    float rn_prelu;
    int32_t reward_env_type;            /* 0,1,2,5,6 */
    int32_t train_episodes, test_episodes, init_episodes, early_out_num, batch_size;
    int32_t rng_mode;
    int32_t agent_kind;                 /* 0 QL (agents/QL.py:37-75), 1 SARSA (agents/SARSA.py:36-60: bootstrap on a freshly drawn
                                           eps-greedy next action) */
    int32_t count_based;                /* ql_cb / sarsa_cb (agents/agent_utils.py:57-64): reward += beta / (sqrt(n(s,a)) + 1e-9) */
    double solved_reward, alpha, gamma, eps_init, eps_min, eps_decay, beta;
    int64_t step_budget;                /* env-step stand-in for time_remaining, see lenv_ddqn_cfg::step_budget */
    int32_t same_action_num;            /* env steps per chosen action (base_agent.py:104,194; env_wrapper.py:56-61: stop at done, python-float
                                           reward sum); 0 and 1 both mean 1 */
    int32_t rn_layer_norm;              /* the ENV section's `use_layer_norm` with rn_layers >= 2, as lenv_ddqn_cfg::se_layer_norm (ABI 6; was padding) */
    int32_t test_mode;                  /* ABI 7: as lenv_ddqn_cfg::test_mode (1 = BaseAgent.train without a test env) */
    double early_out_virtual_diff;      /* read by lenv_ql_se_inner_loop with test_mode 1 (the virtual rule); lenv_ql_rn_inner_loop never reads it: a grid
                                           RewardEnv is not a VirtualEnv (the real rule applies) */
} lenv_ql_cfg;

typedef struct {
    double *score;              /* [chains] */
    int64_t *stats;             /* [chains,4] episodes_run, train_steps, learn_steps, test_steps */
    int32_t *status;            /* [chains] */
    double *episode_test_mean;  /* [chains,train_episodes] */
    int32_t *episode_len;       /* [chains,train_episodes] */
    double *final_returns;      /* [chains,test_episodes] */
    double *q_table;            /* [chains,n_states*n_actions] final fp64 Q-table */
    float *shaped;              /* [chains,n_states*n_actions] shaped reward of every (s,a) */
    int64_t trace_cap;
    int32_t *trace_action;      /* [chains,trace_cap] action | explored<<16 */
    int32_t *trace_state;       /* [chains,trace_cap,2] state, next_state */
    float *trace_reward_done;   /* [chains,trace_cap,2] */
} lenv_ql_out;

int lenv_ql_rn_inner_loop(const lenv_ql_cfg *cfg /*HOST*/, const float *theta, const float *eps, const int32_t *worker,
                          const float *sign, const float *shaped_override, const int32_t *next_state, const double *reward,
                          const uint8_t *done, const uint64_t *rng_keys, const lenv_tapes *tapes /*HOST, may be NULL*/,
                          int64_t chains, const lenv_ql_out *out /*HOST struct of device ptrs*/, void *stream);
/* The same loop for a population of agents with their own hyper-parameters (experiments/GTNC_evaluate_gridworld_transfer_vary_hp.py:92-123:
 * every agent draws alpha and gamma): chain c learns with alpha[c] and bootstraps with gamma[c] (fp64, the python floats of the reference),
 * and, because BaseAgent.train hands gamma to the env (base_agent.py:86), its shaped-reward table of reward types 1 / 2 -- and its row of
 * out->shaped -- uses (float)gamma[c].  A NULL array = cfg's value for every chain; lenv_ql_rn_inner_loop is the NULL / NULL call.
 * (Added under ABI 7: a new entry point only, no struct changed.) */
int lenv_ql_rn_inner_loop_hp(const lenv_ql_cfg *cfg /*HOST*/, const double *alpha /*DEVICE [chains], may be NULL*/,
                             const double *gamma /*DEVICE [chains], may be NULL*/, const float *theta, const float *eps, const int32_t *worker,
                             const float *sign, const float *shaped_override, const int32_t *next_state, const double *reward,
                             const uint8_t *done, const uint64_t *rng_keys, const lenv_tapes *tapes /*HOST, may be NULL*/,
                             int64_t chains, const lenv_ql_out *out /*HOST struct of device ptrs*/, void *stream);

/*
 * The tabular agents on a gridworld VirtualEnv (synthetic_env_type 0): GTN_Worker.calc_score (agents/GTN_worker.py:187-221) with
 * env = VirtualEnv over a Discrete observation space, one workgroup per chain.  theta = state_net | reward_net | done_net (the nn.Linear
 * parameters only), each net Linear(n_actions + n_states, H) | [Linear(H, H)] | Linear(H, out) with the shape in cfg's rn_hidden / rn_layers
 * (1 or 2) / rn_act / rn_prelu; perturbed per chain as theta + sign*eps[worker].  Every training step evaluates the three nets on
 * [one_hot(action) | raw state vector] (envs/virtual_env.py:43-54; the raw state-net output is fed back, the agent sees its argmax: the first maximum, a NaN counting as the maximum as in torch.argmax),
 * same_action_num steps per action regardless of done with an fp32 reward sum (envs/env_wrapper.py:17-49), no TimeLimit; reward and done
 * reach the agent raw (bootstrap mask done < 0.5, episode end done > 0.5).  next_state / reward / done are the REAL grid's tables: the
 * per-episode tests and the final test walk them.  test_mode 1: the SE's own episode reward feeds the meter and the virtual early-out rule
 * (early_out_virtual_diff) applies.  reward_env_type is not read; rn_layer_norm with two hidden layers is refused.  lenv_ql_out as for
 * lenv_ql_rn_inner_loop (trace_state: the agent-visible indices; trace_reward_done: the summed reward and the raw done; `shaped` is not
 * written).  trace_se [chains, trace_cap, n_states + 2] (optional): raw next-state vector | reward | done of the LAST SE step of each agent
 * step.  The staged theta lives in LDS while it fits (lenv_ql_se_lds_bytes <= 160 KiB), otherwise in `workspace`
 * (lenv_ql_se_workspace_bytes; 0 when LDS holds it).  The three queries return LENV_ERR_UNSUPPORTED for a cfg the loop refuses.
 * (Added under ABI 7: new entry points only, no struct changed -- a binding built against the earlier ABI 7 header keeps working.)
 */
int64_t lenv_ql_se_num_params(const lenv_ql_cfg *cfg /*HOST*/);
int64_t lenv_ql_se_lds_bytes(const lenv_ql_cfg *cfg /*HOST*/);
int64_t lenv_ql_se_workspace_bytes(const lenv_ql_cfg *cfg /*HOST*/, int64_t chains);
int lenv_ql_se_inner_loop(const lenv_ql_cfg *cfg /*HOST*/, const float *theta, const float *eps, const int32_t *worker, const float *sign,
                          const int32_t *next_state, const double *reward, const uint8_t *done, const uint64_t *rng_keys,
                          const lenv_tapes *tapes /*HOST, may be NULL*/, int64_t chains, const lenv_ql_out *out /*HOST struct of device ptrs*/,
                          float *trace_se, void *workspace, int64_t workspace_bytes, void *stream);

/*
 * RewardEnv shaping for a population of perturbed reward networks on a grid MDP (envs/reward_env.py:67-133): phi_out
 * [chains,n_states] (optional) = reward_net(one_hot(s)), shaped_out [chains,n_states*n_actions] = what RewardEnv.step
 * returns as reward for (s,a).  Only n_states/n_actions/rn_* /reward_env_type/gamma of cfg are read.
 */
int lenv_rn_shape_population(const lenv_ql_cfg *cfg /*HOST*/, const float *theta, const float *eps, const int32_t *worker,
                             const float *sign, int64_t chains, const int32_t *next_state, const double *reward,
                             float *phi_out, float *shaped_out, void *stream);

/*
 * Real-environment reset/step for n independent instances (replaces gym==0.17.3 CartPole-v0 / Acrobot-v1
 * reset()/step() + gym.wrappers.TimeLimit behind EnvWrapper.reset/step, envs/env_wrapper.py:49-85).
 * state [n,4] float64 (gym's internal state), elapsed [n] TimeLimit counters, obs [n,S] fp32 observations.
 * Reset states are U(-lim,lim)^4 drawn from the counter RNG: value = f(keys[i], episode[i]).
 */
int lenv_real_env_reset(int32_t env_id, const uint64_t *keys, const int64_t *episode, int64_t n, double *state,
                        float *obs, int32_t *elapsed, void *stream);
int lenv_real_env_step(int32_t env_id, int32_t max_steps, int64_t n, const int32_t *action, double *state,
                       int32_t *elapsed, float *obs, float *reward, float *done, void *stream);

/*
 * Fused inner loop for DuelingDDQN agents on a synthetic environment (cfg.agent_kind == 1; agents/DuelingDDQN.py:59-110,
 * models/actor_critic.py:94-122; BASELINE config 3).  Same contract and outputs as lenv_ddqn_se_inner_loop; the agent's
 * parameters / Adam state / activations live in the workspace (lenv_dueling_se_workspace_bytes), agent_init is
 * [chains, lenv_dueling_num_params(cfg)] in state-dict order feature_stream | value_stream | advantage_stream.
 * cfg.agent_kind == 0 selects the plain-DQN mode: a DDQN (agents/DDQN.py:60-94) whose Critic_DQN (models/actor_critic.py:
 * 84-91) has q_layers 1-2 hidden layers of up to 128 units -- the shapes lenv_ddqn_se_inner_loop refuses, e.g. the
 * 6-128-128-3 net of default_config_acrobot.yaml; cfg.feature_dim is ignored, cfg.grad_chunk must be 0 (one sequential
 * batch gradient), agent_init is [chains, lenv_dueling_num_params(cfg)] in the Critic_DQN state-dict order.
 */
/*
 * Per-chain hyper-parameters of the *_vary agents (agents/DDQN_vary.py:26-59, agents/DuelingDDQN_vary.py:24-69: every agent
 * the worker builds draws its own lr / batch_size / hidden_size / hidden_layer).  Device arrays [chains]; with them the
 * cfg carries the MAXIMA (batch_size, q_hidden, q_layers: workspace, LDS and the row stride of agent_init / final_online
 * are sized from cfg) and chain c runs with the c-th entries -- its agent_init row holds lenv_dueling_num_params at ITS
 * shapes, the rest of the row is ignored.  q_layers = max(1, hidden_layer) as in lenv_ddqn_cfg.  A chain whose values
 * exceed cfg's reports status -8.
 */
typedef struct lenv_chain_hp {
    const double *lr;
    const int32_t *batch_size, *q_hidden, *q_layers;
} lenv_chain_hp;

size_t lenv_dueling_se_workspace_bytes(const lenv_ddqn_cfg *cfg /*HOST*/, int64_t chains);
int64_t lenv_dueling_num_params(const lenv_ddqn_cfg *cfg /*HOST*/);
int lenv_dueling_se_inner_loop(const lenv_ddqn_cfg *cfg /*HOST*/, const float *theta, const float *eps,
                               const int32_t *worker, const float *sign, const float *agent_init,
                               const uint64_t *rng_keys, const lenv_tapes *tapes /*HOST, may be NULL*/, int64_t chains,
                               void *workspace, size_t workspace_bytes, const lenv_inner_out *out /*HOST*/, void *stream);
/* Workgroups per chain a production launch (counter RNG, no trace, no hp, no ICM) of this cfg will use: the wave-chain kernel of the
 * published Acrobot SE + DuelingDDQN shape runs a chain on a TEAM of 2 workgroups when 8 * ceil(chains / 8) * 2 of them are resident at
 * once (one per CU), with test_mode 0 and 1 alike, and so does its plain-DQN Acrobot shape; every other launch: 1.  cfg->team_size 1
 * forces 1.  Same bits either way. */
int lenv_dueling_team_size(const lenv_ddqn_cfg *cfg /*HOST*/, int64_t chains);
/* Fresh agents (nn.Linear default init, the draw of lenv_nes_draw) for chains with their own shapes: row c of agent_init
 * [chains, lenv_dueling_num_params(cfg)] gets the parameters of a (hp->q_hidden[c], hp->q_layers[c]) network, keyed by
 * rng_keys[c].  hp == NULL: every chain has cfg's shapes (== lenv_nes_draw's agent_init for the same keys). */
int lenv_dueling_agent_init_hp(const lenv_ddqn_cfg *cfg /*HOST*/, const lenv_chain_hp *hp /*HOST struct of device arrays*/,
                               const uint64_t *rng_keys, int64_t chains, float *agent_init, void *stream);
/* ICM agents: icm_init [chains, lenv_icm_num_params(cfg)] = fresh ICMModel parameters per chain in state-dict order
 * (features_model, inverse_model, forward_pre_model, residual_block1..4 {fc1, fc2}, forward_post_model); icm_final (may be
 * NULL) receives them after the last learn step.  hp != NULL: the *_icm_vary agents (per-chain hyper-parameters of the agent;
 * the ICM keeps cfg's shapes and learning rate).  cfg->icm_enabled == 0: identical to lenv_dueling_se_inner_loop_hp. */
typedef struct lenv_icm_io {
    const float *icm_init;
    float *icm_final;
} lenv_icm_io;
int64_t lenv_icm_num_params(const lenv_ddqn_cfg *cfg /*HOST*/);
int lenv_dueling_se_inner_loop_icm(const lenv_ddqn_cfg *cfg /*HOST*/, const lenv_chain_hp *hp /*HOST, may be NULL*/,
                                   const lenv_icm_io *icm /*HOST struct of device arrays*/, const float *theta, const float *eps,
                                   const int32_t *worker, const float *sign, const float *agent_init, const uint64_t *rng_keys,
                                   const lenv_tapes *tapes /*HOST*/, int64_t chains, void *workspace, size_t workspace_bytes,
                                   const lenv_inner_out *out /*HOST*/, void *stream);
/* the same with per-chain hyper-parameters (hp == NULL: identical to lenv_dueling_se_inner_loop) */
int lenv_dueling_se_inner_loop_hp(const lenv_ddqn_cfg *cfg /*HOST*/, const lenv_chain_hp *hp /*HOST struct of device arrays*/,
                                  const float *theta, const float *eps, const int32_t *worker, const float *sign,
                                  const float *agent_init, const uint64_t *rng_keys, const lenv_tapes *tapes /*HOST*/,
                                  int64_t chains, void *workspace, size_t workspace_bytes, const lenv_inner_out *out /*HOST*/,
                                  void *stream);
/* The same inner loop in EPISODE SEGMENTS (ABI 7, a function only; the DDQN / DuelingDDQN sibling of lenv_td3_rn_inner_loop_segment): a
 * launch runs episodes [episode_begin, episode_end) of every chain and leaves a resume record per chain; the next launch (episode_begin =
 * the last episode_end) goes on from it.  Always the generic GEMM-queue kernel, one workgroup per chain (never the shape-specialised,
 * wave-chain or team kernels, nor the register-resident lenv_ddqn_se_inner_loop).  For every split 0 = e0 < e1 < .. < ek = train_episodes the
 * k launches leave every lenv_inner_out array, icm_final and the step trace bit-identical to one lenv_dueling_se_inner_loop_icm / _hp launch
 * on that kernel.
 *   episode_begin == 0: the arena is initialised from agent_init / icm_init; the record is written, never read.
 *   episode_begin  > 0: nothing in the arena is initialised (online and target nets, Adam state, replay ring, early-out meter, ICM parameters
 *     and their Adam state); the perturbed SE / reward net is staged again from theta / eps (deterministic: the same bits).  The caller passes
 *     the same workspace (untouched in between), out arrays, tapes, hp, icm and theta / eps / worker / sign as to the earlier segments.  A
 *     chain whose record does not say "next episode == episode_begin" writes status -10 and does nothing else.
 * The closing part (final agent.test, score, final_returns, the NaN / time-out padding of unrun episodes, final_online, icm_final) runs once
 * per chain, in the segment in which the chain ends (train_episodes reached, early out, step_budget time-out); the chain is then `finished`
 * and later segments leave it and its outputs untouched.  A segment that ends with the chain unfinished writes the cumulative stats and
 * final_online (a checkpoint) and nothing else of the closing part.
 * Refused with LENV_ERR_INVALID: !(0 <= episode_begin < episode_end <= cfg->train_episodes), resume == NULL, and whatever
 * lenv_dueling_se_inner_loop_icm refuses.  workspace_bytes: lenv_dueling_se_workspace_bytes.
 * The record (opaque to callers), int64 words per chain:
 *    0 next episode to run            1 finished (0 / 1)               2 status so far (0 ok, else the minimum of the chain's codes)
 *    3 timed_out_at (-1: no time-out) 4 n_act (random actions drawn)   5 learn_it (learn calls; replay-index draws = learn_it * batch)
 *    6 n_test_ep (test episodes run = test resets drawn)               7 train_steps (agent steps = epsilon uniforms drawn; ring position
 *      = train_steps % capacity)      8 test_steps                     9 episodes_run
 *   10 trace cursor: rows of the step trace written, before the trace_cap clamp (one row per agent step: always equal to word 7)
 *   11 bit pattern of the double eps_g (the epsilon of the last episode run)
 *   12..13 bit patterns of the doubles beta1^t, beta2^t of the agent's Adam      14..15 the same of the ICM's Adam (1.0 without an ICM)
 *   16..31 reserved (0)
 * Everything else the loop carries lives in the arena (the early-out meter included); the kernel's LDS control words are all rewritten
 * inside an episode before they are read (the flag guarding the carried phi(s) of reward types 1 / 2 is cleared by the episode's reset;
 * test_mode 1 sums an episode's training reward in a register that starts at 0 with the episode), so none crosses a boundary.
 * Status of a FAILING chain and the double meaning of -10: as documented at lenv_td3_rn_inner_loop_segment. */
#define LENV_DUELING_RESUME_WORDS 32
int lenv_dueling_se_inner_loop_segment(const lenv_ddqn_cfg *cfg /*HOST*/, const lenv_chain_hp *hp /*HOST, may be NULL*/,
                                       const lenv_icm_io *icm /*HOST, NULL iff !cfg->icm_enabled*/, const float *theta, const float *eps,
                                       const int32_t *worker, const float *sign, const float *agent_init, const uint64_t *rng_keys,
                                       const lenv_tapes *tapes /*HOST, may be NULL*/, int64_t chains, void *workspace, size_t workspace_bytes,
                                       const lenv_inner_out *out /*HOST*/, int32_t episode_begin, int32_t episode_end,
                                       int64_t *resume /*DEVICE [chains, LENV_DUELING_RESUME_WORDS]*/, void *stream);

/*
 * Config 5: fused inner loop for a TD3 agent on a RewardEnv over a continuous-state real env (agents/TD3.py:63-135,
 * envs/reward_env.py:61-133).  Real env = the documented HalfCheetah-v3 STAND-IN (17 obs / 6 actions, see
 * tools/gen_cheetah_standin.py; MuJoCo is unavailable).  theta = flat reward_net parameters (17 -> H -> 1, PReLU slope
 * excluded); agent_init [chains, P] = actor | critic_1 | critic_2 in state-dict order (lenv_td3_num_params).
 */
typedef struct {
    int32_t env_id, state_dim, action_dim, max_steps;
    int32_t rn_hidden, rn_layers, rn_act;
    float rn_prelu;
    int32_t reward_env_type;                 /* 0-8, 101, 102 (envs/reward_env.py:29-59) */
    int32_t info_dim;                        /* length of the real env's info vector (4 for the stand-in; used by types 3,4,7,8,101,102) */
    int32_t hidden, layers, act;             /* actor / critic MLPs (models/actor_critic.py:11-19,64-71) */
    float prelu;
    int32_t batch_size, rb_size, train_episodes, test_episodes, init_episodes, early_out_num, policy_delay, rng_mode;
    double solved_reward, gamma, lr, tau, action_std, policy_std, policy_std_clip, max_action;
    double adam_beta1, adam_beta2, adam_eps;
    int64_t step_budget;                     /* env-step stand-in for time_remaining, see lenv_ddqn_cfg::step_budget */
    /* TD3(icm=True), select_agent "td3_icm" (agents/TD3.py:44-60,68-70): as lenv_ddqn_cfg's icm_* fields; continuous actions,
     * so the action vector is the ICM's input and its inverse loss is an MSE.  Only lenv_td3_rn_inner_loop_icm takes it. */
    int32_t icm_enabled, icm_feature_dim, icm_hidden;
    /* `use_layer_norm` of the td3 section (models/model_utils.py:22-37): ONE shared nn.LayerNorm(hidden) behind every hidden Linear but the
     * first of the actor and of each critic (three modules, one per net), weight | bias behind the net's second Linear */
    int32_t use_layer_norm;
    double icm_lr, icm_beta, icm_eta;
    /* virtual_env != 0 (gtn.synthetic_env_type 0, default_config_halfcheetah.yaml): the agent trains on a VirtualEnv
     * (envs/virtual_env.py:43-54) instead of the RewardEnv: theta = state_net | reward_net | done_net, each
     * (action_dim + state_dim) -> rn_hidden x rn_layers (1-3) -> {state_dim, 1, 1} with rn_act; the learned done flag (> 0.5)
     * ends a training episode.  Tests run on the real (stand-in) env as before. */
    int32_t virtual_env;
    /* same_action_num (agents/base_agent.py:20,104,194; envs/env_wrapper.py:24,57): env steps per chosen action -- the rewards of
     * the repeats are summed, a real env's repeats stop at done; 0 and 1 both mean 1 (MountainCarContinuous configs ship 2) */
    int32_t same_action_num;
    int32_t team_size;        /* workgroups per chain, as lenv_ddqn_cfg::team_size (0 = automatic, 1 = never a team, G = at most G) */
    int32_t kernel_variant;   /* LENV_VARIANT_* bits, 0 = fastest */
    /* ABI 6.  `use_layer_norm` of the ENV's config section with rn_layers >= 2: the reward net (RewardEnv) / the three SE nets (VirtualEnv)
     * carry the shared nn.LayerNorm behind hidden Linear 2..L.  As lenv_ddqn_cfg::se_layer_norm: NES perturbs nn.Linear modules only, theta / eps
     * stay the Linear parameters, the kernel normalises with the constructor's weight 1 / bias 0. */
    int32_t rn_layer_norm;
    int32_t test_mode;                  /* ABI 7: as lenv_ddqn_cfg::test_mode (1 = BaseAgent.train without a test env) */
    double early_out_virtual_diff;
} lenv_td3_cfg;

/* RNG tapes (parity mode); per-chain rows, strides in ROWS (rows of A floats / B ints / S doubles as noted) */
typedef struct {
    const float *rand_action;  int64_t rand_action_stride;    /* rows of A: env.get_random_action()      env_wrapper.py:87-90 */
    const float *act_noise;    int64_t act_noise_stride;      /* rows of A: randn in select_train_action TD3.py:123 */
    const float *test_noise;   int64_t test_noise_stride;     /* rows of A: randn in select_test_action  TD3.py:128, one row per
                                                                 * chosen action in the reference's order (episode by episode) */
    const float *policy_noise; int64_t policy_noise_stride;   /* rows of A: randn_like(actions) in learn TD3.py:75 */
    const int32_t *replay_idx; int64_t replay_idx_stride;     /* elements */
    const double *train_reset; int64_t train_reset_stride;    /* rows of the env's own state: 17 (stand-in), 2 (Pendulum: theta, */
    const double *test_reset;  int64_t test_reset_stride;     /* theta_dot; MountainCarContinuous: position, velocity) */
} lenv_td3_tapes;

typedef struct {
    double *score;              /* [chains] */
    int64_t *stats;             /* [chains,4] episodes_run, train_steps, learn_steps, test_steps */
    int32_t *status;            /* [chains] 0 ok; -3..-8 as lenv_inner_out::status (-7, -8 here also: noise / policy-noise tape underrun); -9 Gumbel tape underrun (lenv_td3d_inner_loop) */
    double *episode_test_mean;  /* [chains,train_episodes] */
    int32_t *episode_len;       /* [chains,train_episodes] */
    double *final_returns;      /* [chains,test_episodes] */
    float *final_params;        /* [chains,P] */
    int64_t trace_cap;
    float *trace_action;        /* [chains,trace_cap,A] */
    float *trace_state;         /* [chains,trace_cap,S] */
    float *trace_next_state;    /* [chains,trace_cap,S] */
    float *trace_reward;        /* [chains,trace_cap] shaped reward */
} lenv_td3_out;

size_t lenv_td3_rn_workspace_bytes(const lenv_td3_cfg *cfg /*HOST*/, int64_t chains);
int64_t lenv_td3_num_params(const lenv_td3_cfg *cfg /*HOST*/, int64_t *actor_params /*HOST out*/, int64_t *critic_params /*HOST out*/);
int lenv_td3_rn_inner_loop(const lenv_td3_cfg *cfg /*HOST*/, const float *theta, const float *eps, const int32_t *worker,
                           const float *sign, const float *agent_init, const uint64_t *rng_keys,
                           const lenv_td3_tapes *tapes /*HOST, may be NULL*/, int64_t chains, void *workspace,
                           size_t workspace_bytes, const lenv_td3_out *out /*HOST*/, void *stream);
/* TD3_vary (agents/TD3_vary.py:24-58): per-chain lr / batch_size / hidden_size / hidden_layer through the lenv_chain_hp arrays: q_hidden ->
 * cfg.hidden, q_layers -> cfg.layers; cfg carries the maxima, agent_init rows hold actor | critic_1 | critic_2 at the chain's
 * own shapes (row stride lenv_td3_num_params(cfg)).  hp == NULL: identical to lenv_td3_rn_inner_loop. */
int lenv_td3_rn_inner_loop_hp(const lenv_td3_cfg *cfg /*HOST*/, const lenv_chain_hp *hp /*HOST struct of device arrays*/,
                              const float *theta, const float *eps, const int32_t *worker, const float *sign,
                              const float *agent_init, const uint64_t *rng_keys, const lenv_td3_tapes *tapes /*HOST*/,
                              int64_t chains, void *workspace, size_t workspace_bytes, const lenv_td3_out *out /*HOST*/, void *stream);
/* TD3 with an ICM: icm as in lenv_dueling_se_inner_loop_icm (icm_init rows of lenv_td3_icm_num_params(cfg) floats);
 * hp may be NULL (td3_icm) or the per-chain hyper-parameters (td3_icm_vary) */
int64_t lenv_td3_icm_num_params(const lenv_td3_cfg *cfg /*HOST*/);
int lenv_td3_rn_inner_loop_icm(const lenv_td3_cfg *cfg /*HOST*/, const lenv_chain_hp *hp /*HOST, may be NULL*/,
                               const lenv_icm_io *icm /*HOST struct of device arrays*/, const float *theta, const float *eps,
                               const int32_t *worker, const float *sign, const float *agent_init, const uint64_t *rng_keys,
                               const lenv_td3_tapes *tapes /*HOST*/, int64_t chains, void *workspace, size_t workspace_bytes,
                               const lenv_td3_out *out /*HOST*/, void *stream);
/* The same inner loop in EPISODE SEGMENTS (ABI 7, a function only): a launch runs episodes [episode_begin, episode_end) of every chain and
 * leaves a resume record per chain; the next launch (episode_begin = the last episode_end) goes on from it.  Always the generic GEMM-queue
 * kernel, one workgroup per chain (never the wave-chain / shape-specialised / product-queue-free instantiations).  For every split
 * 0 = e0 < e1 < .. < ek = train_episodes the k launches leave every lenv_td3_out array, icm_final and the traces bit-identical to one
 * lenv_td3_rn_inner_loop_icm / _hp launch on that kernel.
 *   episode_begin == 0: the arena is initialised from agent_init / icm_init; the record is written, never read.
 *   episode_begin  > 0: nothing is initialised; the caller passes the same workspace (untouched in between), out arrays, tapes, hp, icm and
 *     theta / eps / worker / sign as to the earlier segments.  A chain whose record does not say "next episode == episode_begin" writes
 *     status -10 and does nothing else.
 * The closing part (final agent.test, score, final_returns, the NaN / time-out padding of unrun episodes, icm_final) runs once per chain,
 * in the segment in which the chain ends (train_episodes reached, early out, step_budget time-out); the chain is then `finished` and later
 * segments leave it and its outputs untouched.  A segment that ends with the chain unfinished writes the cumulative stats and final_params
 * (a checkpoint) and nothing else of the closing part.
 * Refused with LENV_ERR_INVALID: !(0 <= episode_begin < episode_end <= cfg->train_episodes), resume == NULL, and whatever
 * lenv_td3_rn_inner_loop_icm refuses.  workspace_bytes: lenv_td3_rn_workspace_bytes.
 * The record (opaque to callers), int64 words per chain:
 *    0 next episode to run            1 finished (0 / 1)               2 status so far (0 ok, else the minimum of the chain's codes)
 *    3 timed_out_at (-1: no time-out) 4 n_rand (random actions drawn)  5 n_actn (train-action noise rows drawn)
 *    6 n_testn (test noise rows)      7 n_test_ep (test episodes run)  8 learn_it (TD3.learn calls)
 *    9 train_steps (agent steps; ring position = train_steps % capacity)   10 test_steps   11 episodes_run
 *   12 trace cursor: rows of the step trace written, before the trace_cap clamp (one row per agent step: always equal to word 9)
 *   13..16 bit patterns of the doubles beta1^t, beta2^t of the critic optimizer, then of the actor optimizer
 *   17..18 bit patterns of the ICM optimizer's beta1^t, beta2^t (1.0 without an ICM)      19..31 reserved (0)
 * The early-out meter (the per-episode test means) lives in the arena.
 * Status of a FAILING chain: a thread keeps the code of its latest failure and the launch reports the minimum over the threads; a series of
 * segments folds that minimum at every boundary and starts every thread of the next segment from it, so after different kinds of failure in
 * different segments a series can report a smaller code than the single launch would (-7 then -3: -7 instead of -3).  Both are non-zero.
 * Status -10 here means "the record names another episode"; on the team launches of the other entry points the same value means that a
 * team member gave up waiting (lenv_ddqn_cfg::team_size): a caller that retries -10 with team_size 1 must not do so after a segment launch. */
#define LENV_TD3_RESUME_WORDS 32
int lenv_td3_rn_inner_loop_segment(const lenv_td3_cfg *cfg /*HOST*/, const lenv_chain_hp *hp /*HOST, may be NULL*/,
                                   const lenv_icm_io *icm /*HOST, NULL iff !cfg->icm_enabled*/, const float *theta, const float *eps,
                                   const int32_t *worker, const float *sign, const float *agent_init, const uint64_t *rng_keys,
                                   const lenv_td3_tapes *tapes /*HOST, may be NULL*/, int64_t chains, void *workspace, size_t workspace_bytes,
                                   const lenv_td3_out *out /*HOST*/, int32_t episode_begin, int32_t episode_end,
                                   int64_t *resume /*DEVICE [chains, LENV_TD3_RESUME_WORDS]*/, void *stream);
/* Workgroups per chain a production launch (counter RNG, no trace, no hp, no ICM) of this cfg will use: the wave-chain kernel of the
 * published HalfCheetah RewardEnv + TD3 shape runs a chain on a TEAM of 6, 3 or 2 workgroups when 8 * ceil(chains / 8) * G of them
 * are resident at once (one per CU), with test_mode 0 and 1 alike, and so do its other shapes; every other launch: 1.  cfg->team_size
 * caps it.  Same bits for every G. */
int lenv_td3_rn_team_size(const lenv_td3_cfg *cfg /*HOST*/, int64_t chains);
int lenv_td3_agent_init_hp(const lenv_td3_cfg *cfg /*HOST*/, const lenv_chain_hp *hp, const uint64_t *rng_keys, int64_t chains,
                           float *agent_init, void *stream);

/*
 * TD3_discrete_vary: fused inner loop for TD3 on a DISCRETE action space through a Gumbel-softmax actor, trained on a VirtualEnv and
 * tested on the real env (agents/TD3_discrete_vary.py:16-117,159-177; models/actor_critic.py:22-35 Actor_TD3_discrete;
 * agents/base_agent.py:64-227 with discretize_action: the replay buffer keeps the action VECTOR, the env gets its argmax;
 * envs/env_wrapper.py:16-47 one-hot of that index in front of the three SE nets, envs/virtual_env.py:43-54).
 * use_layer_norm (models/model_utils.py:22-37): ONE nn.LayerNorm(hidden) shared by the hidden Linear layers 2..L of a net, in front
 * of the activation.  Flat parameters of a net in Module.parameters() order: W0 b0 [W1 b1 [LNw LNb] W2 b2 ...] Wout bout;
 * agent_init / final_params rows = actor | critic_1 | critic_2.  theta = state_net | reward_net | done_net as in lenv_ddqn_cfg.
 */
typedef struct {
    int32_t env_id, state_dim, action_dim, max_steps;   /* LENV_ENV_CARTPOLE 4 / 2, LENV_ENV_ACROBOT 6 / 3, LENV_ENV_MOUNTAINCAR 2 / 3 */
    int32_t se_hidden, se_layers, se_act;
    float se_prelu;
    int32_t hidden, layers, act;                         /* actor S -> A and critics (S + A) -> 1 (models/model_utils.py:4-39) */
    float prelu;
    int32_t use_layer_norm;
    int32_t gumbel_hard;                                 /* gumbel_softmax_hard: straight-through one-hot forward (actor_critic.py:31,35) */
    int32_t batch_size, rb_size, train_episodes, test_episodes, init_episodes, early_out_num, policy_delay, rng_mode;
    double solved_reward, gamma, lr, tau, action_std, policy_std, policy_std_clip, max_action;
    double gumbel_temp;                                  /* gumbel_softmax_temp, annealed to 1/20 of it over the first 2000 learn calls (:59-68) */
    double adam_beta1, adam_beta2, adam_eps;
    int64_t step_budget;                                 /* env-step stand-in for time_remaining, see lenv_ddqn_cfg::step_budget */
    int32_t se_layer_norm;                               /* ABI 6: the ENV section's `use_layer_norm`, as lenv_ddqn_cfg::se_layer_norm */
    int32_t test_mode;                  /* ABI 7: as lenv_ddqn_cfg::test_mode (1 = BaseAgent.train without a test env) */
    double early_out_virtual_diff;
} lenv_td3d_cfg;

/* RNG tapes (parity mode); per-chain rows, strides in ROWS (rows of A floats / one int / four doubles as noted) */
typedef struct {
    const int32_t *rand_action; int64_t rand_action_stride;    /* Discrete.sample() of the init episodes (env_wrapper.py:87-92) */
    const float *act_noise;     int64_t act_noise_stride;      /* rows of A: randn(action_dim) in select_train_action :167 */
    const float *test_noise;    int64_t test_noise_stride;     /* rows of A: the same in select_test_action :171 */
    const float *policy_noise;  int64_t policy_noise_stride;   /* rows of A, B per learn call: randn_like(actions) :76 */
    const float *gumbel_act;    int64_t gumbel_act_stride;     /* rows of A: Gumbel(0,1) draws of F.gumbel_softmax in select_train_action */
    const float *gumbel_test;   int64_t gumbel_test_stride;    /* rows of A: ... in select_test_action */
    const float *gumbel_target; int64_t gumbel_target_stride;  /* rows of A, B per learn call: actor_target(next_states) :77 */
    const float *gumbel_actor;  int64_t gumbel_actor_stride;   /* rows of A, B per policy update: actor(states) :101 */
    const int32_t *replay_idx;  int64_t replay_idx_stride;     /* elements, B per learn call */
    const double *train_reset;  int64_t train_reset_stride;    /* rows of 4: the reset env's own state */
    const double *test_reset;   int64_t test_reset_stride;
} lenv_td3d_tapes;

size_t lenv_td3d_workspace_bytes(const lenv_td3d_cfg *cfg /*HOST*/, int64_t chains);
int64_t lenv_td3d_num_params(const lenv_td3d_cfg *cfg /*HOST*/, int64_t *actor_params /*HOST out*/, int64_t *critic_params /*HOST out*/);
int64_t lenv_td3d_se_num_params(const lenv_td3d_cfg *cfg /*HOST*/);
/* hp (may be NULL): per-chain lr / batch_size / hidden_size / hidden_layer of vary_hyperparameters (:119-157); cfg carries the
 * maxima, agent_init rows hold the nets at the chain's own shapes (row stride lenv_td3d_num_params(cfg)).  out: lenv_td3_out
 * (trace_action rows hold the action vectors the replay buffer got). */
int lenv_td3d_inner_loop(const lenv_td3d_cfg *cfg /*HOST*/, const lenv_chain_hp *hp /*HOST struct of device arrays, may be NULL*/,
                         const float *theta, const float *eps, const int32_t *worker, const float *sign, const float *agent_init,
                         const uint64_t *rng_keys, const lenv_td3d_tapes *tapes /*HOST, may be NULL*/, int64_t chains, void *workspace,
                         size_t workspace_bytes, const lenv_td3_out *out /*HOST*/, void *stream);
/*
 * TD3_discrete_vary trained on RewardEnv(real env) (envs/reward_env.py:61-133), or on the real env itself (reward_env_type 0: the real
 * reward passes through, syn_env_run_vary_hp.py mode 0): the chain steps the real env's fp64 physics (TimeLimit: done at max_steps) and
 * shapes its reward with the perturbed reward net, as lenv_rn_shape_rows does.  The cfg's se_* fields are not read; theta / eps rows are the
 * reward net's flat parameters (RewardEnv.build_reward_net: S -> rn_hidden x rn_layers -> 1, a 1-input dummy for type 0) in
 * Module.parameters() order.  The early out is the real rule (also with test_mode 1).
 */
typedef struct {
    int32_t synthetic_env_type;         /* 1 (RewardEnv); anything else: LENV_ERR_UNSUPPORTED */
    int32_t reward_env_type;            /* 0, 1, 2, 5, 6; the info-vector types have no info here: LENV_ERR_UNSUPPORTED */
    int32_t rn_hidden, rn_layers, rn_act;   /* the ENV section's hidden_size / hidden_layer / activation_fn */
    float rn_prelu;                     /* the reward net's (never perturbed) nn.PReLU slope */
    int32_t rn_layer_norm;              /* the ENV section's use_layer_norm: with rn_layers >= 2 and reward_env_type != 0 LENV_ERR_UNSUPPORTED */
} lenv_td3d_rn_cfg;

size_t lenv_td3d_rn_workspace_bytes(const lenv_td3d_cfg *cfg /*HOST*/, const lenv_td3d_rn_cfg *rn /*HOST*/, int64_t chains);
/* parameters of the reward net (the length of theta and of an eps row) */
int64_t lenv_td3d_rn_num_params(const lenv_td3d_cfg *cfg /*HOST*/, const lenv_td3d_rn_cfg *rn /*HOST*/);
/* as lenv_td3d_inner_loop; tapes: train_reset rows are the real env's reset states */
int lenv_td3d_rn_inner_loop(const lenv_td3d_cfg *cfg /*HOST*/, const lenv_td3d_rn_cfg *rn /*HOST*/,
                            const lenv_chain_hp *hp /*HOST struct of device arrays, may be NULL*/, const float *theta, const float *eps,
                            const int32_t *worker, const float *sign, const float *agent_init, const uint64_t *rng_keys,
                            const lenv_td3d_tapes *tapes /*HOST, may be NULL*/, int64_t chains, void *workspace, size_t workspace_bytes,
                            const lenv_td3_out *out /*HOST*/, void *stream);
/* The two TD3_discrete_vary inner loops in EPISODE SEGMENTS (ABI 7, functions only; the siblings of lenv_td3_rn_inner_loop_segment): a launch
 * runs episodes [episode_begin, episode_end) of every chain on the SEG instantiations of the same kernel and leaves a resume record per chain;
 * the next launch (episode_begin = the last episode_end) goes on from it.  For every split 0 = e0 < e1 < .. < ek = train_episodes the k launches
 * leave every lenv_td3_out array and the traces bit-identical to one lenv_td3d_inner_loop / lenv_td3d_rn_inner_loop launch.
 *   episode_begin == 0: the arena is initialised from agent_init; the record is written, never read.
 *   episode_begin  > 0: nothing in the arena is initialised (parameters, targets, Adam m / v, the replay ring, the early-out meter); the perturbed
 *     SE / reward net is staged again from theta / eps / worker / sign.  The caller passes the same workspace (untouched in between), out
 *     arrays, tapes, hp and theta / eps / worker / sign as to the earlier segments.  A chain whose record does not say "next episode ==
 *     episode_begin" writes status -10 and does nothing else; a chain whose record says finished returns at once.
 * The closing part (final test, score, final_returns, the NaN / time-out padding of unrun episodes, final_params) runs once per chain, in the
 * segment in which the chain ends (train_episodes reached, early out, step_budget time-out).  A segment that ends with the chain unfinished
 * writes the cumulative stats and final_params (a checkpoint) and nothing else of the closing part.
 * Refused with LENV_ERR_INVALID, before `chains == 0` is accepted: !(0 <= episode_begin < episode_end <= cfg->train_episodes), resume == NULL,
 * and whatever the continued entry refuses, with its code (a cfg it does not support: LENV_ERR_UNSUPPORTED, also for zero chains).
 * workspace_bytes: lenv_td3d_workspace_bytes / lenv_td3d_rn_workspace_bytes.
 * The record (opaque to callers), int64 words per chain:
 *    0 next episode to run            1 finished (0 / 1)               2 status so far (0 ok, else the minimum of the chain's codes)
 *    3 timed_out_at (-1: no time-out) 4 n_rand (random actions drawn)  5 n_actn (train-action Gumbel / noise rows drawn)
 *    6 n_testn (test rows drawn from the tapes)  7 n_test_ep (test episodes run)  8 learn_it (learn calls)
 *    9 train_steps (agent steps; ring position = train_steps % capacity)   10 test_steps   11 episodes_run
 *   12 trace cursor: rows of the step trace written, before the trace_cap clamp (one row per agent step: always equal to word 9)
 *   13..16 bit patterns of the doubles beta1^t, beta2^t of the critic optimizer, then of the actor optimizer
 *   17 policy_it (delayed policy updates made: the row counter of the actor's Gumbel draws)
 *   18 bit pattern (low 32 bits) of the annealed Gumbel temperature as the acting steps read it: the schedule value of the LAST learn call,
 *      which is one schedule step behind the value at learn_it               19..31 reserved (0)
 * The early-out meter (the per-episode test means) lives in the arena.
 * Status of a failing chain and the double meaning of -10: as documented at lenv_td3_rn_inner_loop_segment. */
#define LENV_TD3D_RESUME_WORDS 32
int lenv_td3d_inner_loop_segment(const lenv_td3d_cfg *cfg /*HOST*/, const lenv_chain_hp *hp /*HOST struct of device arrays, may be NULL*/,
                                 const float *theta, const float *eps, const int32_t *worker, const float *sign, const float *agent_init,
                                 const uint64_t *rng_keys, const lenv_td3d_tapes *tapes /*HOST, may be NULL*/, int64_t chains, void *workspace,
                                 size_t workspace_bytes, const lenv_td3_out *out /*HOST*/, int32_t episode_begin, int32_t episode_end,
                                 int64_t *resume /*DEVICE [chains, LENV_TD3D_RESUME_WORDS]*/, void *stream);
int lenv_td3d_rn_inner_loop_segment(const lenv_td3d_cfg *cfg /*HOST*/, const lenv_td3d_rn_cfg *rn /*HOST*/,
                                    const lenv_chain_hp *hp /*HOST struct of device arrays, may be NULL*/, const float *theta, const float *eps,
                                    const int32_t *worker, const float *sign, const float *agent_init, const uint64_t *rng_keys,
                                    const lenv_td3d_tapes *tapes /*HOST, may be NULL*/, int64_t chains, void *workspace, size_t workspace_bytes,
                                    const lenv_td3_out *out /*HOST*/, int32_t episode_begin, int32_t episode_end,
                                    int64_t *resume /*DEVICE [chains, LENV_TD3D_RESUME_WORDS]*/, void *stream);
/* fresh agents: nn.Linear default init from the chain key's counter stream, LayerNorm weight 1 / bias 0 */
int lenv_td3d_agent_init(const lenv_td3d_cfg *cfg /*HOST*/, const lenv_chain_hp *hp /*may be NULL*/, const uint64_t *rng_keys,
                         int64_t chains, float *agent_init, void *stream);

/*
 * PPO on a RewardEnv over a continuous real env (agents/PPO.py:14-188, models/actor_critic.py:38-61,74-81, envs/reward_env.py:61-133):
 * one 512-thread workgroup per chain runs PPO.train(env=reward_env, test_env=real_env) and the final agent.test(real_env) of
 * GTN_Worker.calc_score (agents/GTN_worker.py:187-221).  Real envs: the HalfCheetah-v3 STAND-IN, Pendulum-v0, MountainCarContinuous-v0
 * (those of the TD3 cfg); reward_env_type as there, 0 = the real env itself: theta is not read.
 *   - acting, train and test alike (actor_critic.py:45-49): a = tanh(net_old(s)) + std_old * z, z ~ N(0,1)^A, std_old clamped in place to
 *     >= 0.001 first; the action is neither rescaled nor clipped;
 *   - a row (s, a, r, done) per chosen action; PPO.learn runs once time_step / max_steps > update_episodes (a double comparison;
 *     time_step += same_action_num per row) on ALL rows since the last call -- lenv_ppo_rows(cfg) of them, possibly in the middle of
 *     an episode -- and time_step restarts at 0;
 *   - learn: discounted returns by one backward scan that restarts only where done > 0.5, normalised with the unbiased std; ppo_epochs
 *     full-batch Adam steps (one step counter over action_std, actor.net, critic.net) on the clipped surrogate + vf_coef * MSE -
 *     ent_coef * entropy; Actor_PPO.evaluate clamps action_std to >= 0.01 AFTER the log-probabilities and BEFORE the entropy, and the
 *     gradient sees the clamped value wherever autograd saved the parameter itself;
 *   - no time-out (PPO.train never calls time_is_up), no init_episodes gate on acting or learning; after every episode test_episodes
 *     real-env episodes feed the meter, early out by the real rule from init_episodes on.
 * Flat agent parameters (agent_init, final_params, learn_params rows): action_std [A] | actor.net (S -> A) | critic.net (S -> 1), each net
 * in the MLP layout above.  Supported: hidden <= 128, layers 1-2, lenv_ppo_rows(cfg) in [2, 2048], test_episodes <= 64, no agent PReLU, LDS within
 * 160 KiB: anything else is LENV_ERR_UNSUPPORTED from every query below.  The cfg has no LayerNorm fields: the kernel normalises nowhere, and a
 * binding refuses `use_layer_norm` in the ppo section, or in the ENV section of a reward net with two or more hidden layers, itself
 * (config.ppo_cfg_from_config does).
 */
typedef struct {
    int32_t env_id, state_dim, action_dim, max_steps;
    int32_t rn_hidden, rn_layers, rn_act;
    float rn_prelu;
    int32_t reward_env_type, info_dim;
    int32_t hidden, layers, act;             /* actor.net / critic.net (the ppo section's hidden_size, max(1, hidden_layer), activation_fn) */
    float prelu;
    int32_t train_episodes, test_episodes, init_episodes, early_out_num;
    int32_t ppo_epochs, same_action_num, rng_mode;
    int32_t reserved;                        /* 0 */
    double solved_reward, gamma, lr, action_std, vf_coef, ent_coef, eps_clip, update_episodes;
    double adam_beta1, adam_beta2, adam_eps;
} lenv_ppo_cfg;

/* RNG tapes (parity mode); per-chain rows, strides in ROWS */
typedef struct {
    const float *act_noise;    int64_t act_noise_stride;      /* rows of A: the _standard_normal draw of actor_old.forward while training */
    const float *test_noise;   int64_t test_noise_stride;     /* rows of A: the same inside BaseAgent.test, episode by episode */
    const double *train_reset; int64_t train_reset_stride;    /* rows of the env's own state (17 / 2 / 2 doubles) */
    const double *test_reset;  int64_t test_reset_stride;
} lenv_ppo_tapes;

typedef struct {
    double *score;              /* [chains] */
    int64_t *stats;             /* [chains,4] episodes_run, rows collected, learn calls, test_steps */
    int32_t *status;            /* [chains] 0 ok; -4 more rows than lenv_ppo_rows between two learn calls (an internal error: learn fires at that
                                 * count), -5 reset tape underrun, -7 noise tape underrun */
    double *episode_test_mean;  /* [chains,train_episodes] */
    int32_t *episode_len;       /* [chains,train_episodes] */
    double *final_returns;      /* [chains,test_episodes] */
    float *final_params;        /* [chains,P] */
    int64_t trace_cap;
    float *trace_action;        /* [chains,trace_cap,A] */
    float *trace_state;         /* [chains,trace_cap,S] */
    float *trace_next_state;    /* [chains,trace_cap,S] */
    float *trace_reward;        /* [chains,trace_cap] shaped reward of the row */
    float *trace_done;          /* [chains,trace_cap] */
    int64_t learn_cap;          /* learn calls recorded per chain */
    int32_t *learn_step;        /* [chains,learn_cap] rows collected over the whole run when the call fired (0 = no such call) */
    float *learn_params;        /* [chains,learn_cap,P] parameters after the call (may be NULL) */
} lenv_ppo_out;

/* rows one learn call sees, or a negative LENV_ERR_*.  HOST. */
int64_t lenv_ppo_rows(const lenv_ppo_cfg *cfg /*HOST*/);
/* P = A + actor_params + critic_params, or a negative LENV_ERR_*.  HOST. */
int64_t lenv_ppo_num_params(const lenv_ppo_cfg *cfg /*HOST*/, int64_t *actor_params /*HOST out*/, int64_t *critic_params /*HOST out*/);
/* parameters of the reward net (length of theta and of an eps row; 0 for reward_env_type 0), or a negative LENV_ERR_*.  HOST. */
int64_t lenv_ppo_rn_num_params(const lenv_ppo_cfg *cfg /*HOST*/);
/* dynamic LDS bytes one chain needs for this cfg (staging buffers, command queue, a one-hidden-layer reward net, the rollout's rows), or a
 * negative LENV_ERR_* -- UNSUPPORTED when they exceed the 160 KiB of a CU (a wide reward net on many inputs).  HOST. */
int64_t lenv_ppo_rn_lds_bytes(const lenv_ppo_cfg *cfg /*HOST*/);
/* workspace bytes for `chains` chains, or a negative LENV_ERR_* (UNSUPPORTED: a shape or option outside the list above).  HOST. */
int64_t lenv_ppo_rn_workspace_bytes(const lenv_ppo_cfg *cfg /*HOST*/, int64_t chains);
int lenv_ppo_rn_inner_loop(const lenv_ppo_cfg *cfg /*HOST*/, const float *theta, const float *eps, const int32_t *worker,
                           const float *sign, const float *agent_init, const uint64_t *rng_keys,
                           const lenv_ppo_tapes *tapes /*HOST, may be NULL*/, int64_t chains, void *workspace,
                           size_t workspace_bytes, const lenv_ppo_out *out /*HOST*/, void *stream);
/* The same inner loop in EPISODE SEGMENTS (ABI 7, a function only): a launch runs episodes [episode_begin, episode_end) of every chain and
 * leaves a resume record per chain; the next launch (episode_begin = the last episode_end) goes on from it.  For every split
 * 0 = e0 < e1 < .. < ek = train_episodes the k launches leave every lenv_ppo_out array (score, stats, status, episode_test_mean, episode_len,
 * final_returns, final_params, the five trace arrays, learn_step, learn_params) bit-identical to one lenv_ppo_rn_inner_loop launch.
 *   episode_begin == 0: the arena is initialised from agent_init; the record is written, never read.
 *   episode_begin  > 0: nothing in the arena is initialised; the caller passes the same workspace (untouched in between), out arrays, tapes
 *     and theta / eps / worker / sign / rng_keys as to the earlier segments.  A chain whose record does not say
 *     "next episode == episode_begin" writes status -10 and does nothing else.
 * The closing part (final agent.test, score, final_returns, the NaN / 0 padding of unrun episodes, the final stats) runs once per chain, in the
 * segment in which the chain ends (train_episodes reached or early out); the chain is then `finished` and later segments return at once and
 * leave it and its outputs untouched.  A segment that ends with the chain unfinished writes the cumulative stats and final_params (a
 * checkpoint) and nothing else of the closing part.
 * Refused with LENV_ERR_INVALID, before the `chains == 0` return: !(0 <= episode_begin < episode_end <= cfg->train_episodes), resume == NULL,
 * and whatever lenv_ppo_rn_inner_loop refuses (an unsupported cfg: its own code).  workspace_bytes: lenv_ppo_rn_workspace_bytes.
 * The record (opaque to callers), int64 words per chain:
 *    0 next episode to run            1 finished (0 / 1)               2 status so far (0 ok, else the minimum of the chain's codes)
 *    3 n_actn (train-action noise rows drawn)   4 n_testn (test noise rows)   5 n_test_ep (test episodes run)
 *    6 time_step (env steps since the last learn call: PPO.py:100's counter)   7 n_rows (rows waiting in the on-policy buffer)
 *    8 train_steps (agent steps; also the trace cursor before the trace_cap clamp)   9 test_steps   10 episodes_run
 *   11 learn_calls (PPO.learn calls; also the learn_step / learn_params cursor before the learn_cap clamp)
 *   12..13 bit patterns of the doubles beta1^t, beta2^t of the optimizer
 *   14..21 bit patterns (low 32 bits) of actor_old's action_std[0..8) as the next action has to see it: clamped to >= 0.001 by the
 *          actions taken so far, equal to actor's after a learn call; entries >= action_dim are 0
 *   22..23 lenv_ppo_icm_inner_loop_segment: bit patterns of the ICM optimizer's beta1^t, beta2^t (1.0 before the module's first step);
 *          0 in a record of lenv_ppo_rn_inner_loop_segment                                               24..31 reserved (0)
 * The parameters, the Adam moments, the partly filled on-policy row buffer and the early-out meter live in the arena.
 * Status of a FAILING chain: a thread keeps the code of its latest failure and the launch reports the minimum over the threads; a series of
 * segments folds that minimum at every boundary and starts every thread of the next segment from it, so after different kinds of failure in
 * different segments a series can report a smaller code than the single launch would.  Both are non-zero. */
#define LENV_PPO_RESUME_WORDS 32
int lenv_ppo_rn_inner_loop_segment(const lenv_ppo_cfg *cfg /*HOST*/, const float *theta, const float *eps, const int32_t *worker,
                                   const float *sign, const float *agent_init, const uint64_t *rng_keys,
                                   const lenv_ppo_tapes *tapes /*HOST, may be NULL*/, int64_t chains, void *workspace,
                                   size_t workspace_bytes, const lenv_ppo_out *out /*HOST*/, int32_t episode_begin, int32_t episode_end,
                                   int64_t *resume /*DEVICE [chains, LENV_PPO_RESUME_WORDS]*/, void *stream);

/* PPO with an Intrinsic Curiosity Module, PPO(icm=True) (agents/PPO.py:46-62,144-145,183-184; the `ppo_icm` agent of the transfer scripts'
 * mode -1) -- ABI 7, functions only: lenv_ppo_cfg is unchanged and the module's five settings (the config's `icm` section) are scalar
 * arguments.  The inner loop is lenv_ppo_rn_inner_loop's with, inside every PPO.learn call on its n rows,
 *   - rewards[i] += eta * mean_f (features(s'_i) - forward(s_i, a_i))^2 for ALL n rows before the return scan, computed with the module as
 *     the previous call left it (the fresh module in the first call); s' is the observation the agent step ended in;
 *   - ONE Adam step of the module (lr icm_lr, cfg's adam_beta1 / adam_beta2 / adam_eps, a step counter of its own) on all n rows after the
 *     last epoch: loss (1 - icm_beta) * MSE(inverse(s, s'), a) + icm_beta * MSE(forward(s, a), features(s')).
 * The module is the one of lenv_td3_rn_inner_loop_icm (continuous actions: the action vector is the input); icm->icm_init
 * [chains, lenv_ppo_icm_num_params] = fresh parameters per chain in that layout, icm->icm_final (may be NULL) receives them with the closing
 * part and, like final_params, as a checkpoint at the end of an unfinished segment.  trace_reward stays the shaped reward at collection time
 * and learn_params rows stay the agent's P parameters.
 * Admitted: what lenv_ppo_rn_inner_loop admits, with icm_feature_dim and icm_hidden in 1..128.  Refused before any launch and before the
 * `chains == 0` return: LENV_ERR_INVALID for icm == NULL or icm->icm_init == NULL, LENV_ERR_UNSUPPORTED for a dimension outside 1..128, and
 * whatever the ICM-less entry refuses with its code.  One kernel serves both launch entries: lenv_ppo_icm_inner_loop runs the segment
 * [0, train_episodes) with its records kept in the workspace; lenv_ppo_icm_inner_loop_segment is lenv_ppo_rn_inner_loop_segment's contract
 * (every split leaves every output, icm_final included, bit-identical to the single launch; record words 22..23 above).  The workspace holds
 * per chain the ICM-less arena, the next-observation rows and the module's parameters, Adam moments and activations for
 * lenv_ppo_rows(cfg) rows. */
/* parameters of the module (the length of an icm_init row), or a negative LENV_ERR_*.  HOST. */
int64_t lenv_ppo_icm_num_params(const lenv_ppo_cfg *cfg /*HOST*/, int32_t icm_feature_dim, int32_t icm_hidden);
int64_t lenv_ppo_icm_workspace_bytes(const lenv_ppo_cfg *cfg /*HOST*/, int32_t icm_feature_dim, int32_t icm_hidden, int64_t chains);
int lenv_ppo_icm_inner_loop(const lenv_ppo_cfg *cfg /*HOST*/, int32_t icm_feature_dim, int32_t icm_hidden, double icm_lr, double icm_beta,
                            double icm_eta, const lenv_icm_io *icm /*HOST struct of device arrays*/, const float *theta, const float *eps,
                            const int32_t *worker, const float *sign, const float *agent_init, const uint64_t *rng_keys,
                            const lenv_ppo_tapes *tapes /*HOST, may be NULL*/, int64_t chains, void *workspace, size_t workspace_bytes,
                            const lenv_ppo_out *out /*HOST*/, void *stream);
int lenv_ppo_icm_inner_loop_segment(const lenv_ppo_cfg *cfg /*HOST*/, int32_t icm_feature_dim, int32_t icm_hidden, double icm_lr,
                                    double icm_beta, double icm_eta, const lenv_icm_io *icm /*HOST struct of device arrays*/,
                                    const float *theta, const float *eps, const int32_t *worker, const float *sign, const float *agent_init,
                                    const uint64_t *rng_keys, const lenv_ppo_tapes *tapes /*HOST, may be NULL*/, int64_t chains,
                                    void *workspace, size_t workspace_bytes, const lenv_ppo_out *out /*HOST*/, int32_t episode_begin,
                                    int32_t episode_end, int64_t *resume /*DEVICE [chains, LENV_PPO_RESUME_WORDS]*/, void *stream);

/*
 * Batched forward of one MLP in the flat layout above: y [rows,out] = net(x [rows,in]) (models/model_utils.py:31-39;
 * behind Critic_DQN / Actor_TD3.net / Critic_Q / reward_net calls of the one-step API).
 */
int lenv_mlp_forward(const lenv_mlp_desc *d /*HOST*/, const float *params, const float *x, int64_t rows, float *y, void *stream);

/*
 * RewardEnv on a vector-state real env, one-step API (envs/reward_env.py:29-133).
 * lenv_rn_num_params: parameters of build_reward_net for a reward type -- MLP on state_dim (types 1,2,5,6) or
 * state_dim+info_dim (3,4,7,8) inputs, Linear(info_dim,1,bias=False) for 101/102, 0 for type 0; LENV_ERR_UNSUPPORTED for an
 * unknown type (the reference raises NotImplementedError).  HOST.
 * lenv_rn_shape_rows: RewardEnv._calc_reward for `rows` transitions: s, s2 [rows,state_dim], info [rows,info_dim] (the
 * real env's info values in dict order, fp32; may be NULL for the types that do not read it -- otherwise a missing info
 * is LENV_ERR_INVALID, the reference's ValueError), r [rows] the real reward rounded to fp32; out [rows] fp32.
 */
int64_t lenv_rn_num_params(int32_t type, int32_t state_dim, int32_t info_dim, int32_t hidden, int32_t layers);
int lenv_rn_shape_rows(int32_t type, const lenv_mlp_desc *rn /*HOST, types 1-8*/, int32_t state_dim, int32_t info_dim, double gamma,
                       const float *theta, const float *s, const float *s2, const float *info, const float *r, int64_t rows,
                       float *out, void *stream);

/*
 * One RewardEnv step for a whole NES population in one launch (the non-virtual half of EnvWrapper.step_population): chain c steps its own
 * instance of a vector-state real env on its action up to `repeat` times -- the same_action_num loop of EnvWrapper._step_real
 * (envs/env_wrapper.py:48-70): stop after the step that reports done, the TimeLimit at max_steps counts as done -- and shapes every step's
 * reward with the reward net W_c, W_c[i] = fmaf(sign[c], eps[worker[c]][i], theta[i]) (eps may be NULL: the plain theta; type 0 reads
 * neither).  The shaped rewards are added in fp64, like the .item() floats Python adds, and rounded once.
 * env_id: LENV_ENV_CARTPOLE / ACROBOT / MOUNTAINCAR (action int32 [chains], state [chains,4] fp64) or LENV_ENV_PENDULUM / CMC /
 * CHEETAH_STANDIN (action float [chains,A], state [chains,2 | 2 | 17]); state, elapsed [chains]: the contract of lenv_real_env_step /
 * lenv_cont_env_step, updated in place.  type, rn, state_dim, info_dim, gamma, theta's layout: as in lenv_rn_shape_rows (1-4 hidden layers,
 * hidden <= 256, <= 64 net inputs, the shared LayerNorm's weight | bias behind the second Linear); eps rows have theta's length.  The info
 * vector is the stand-in's own (info_dim 4).  Outputs: obs [chains,state_dim] the last observation, reward [chains] the sum, done [chains]
 * the last step's flag.  With repeat 1 the outputs are bit for bit those of the env step entry followed by lenv_rn_shape_rows on the
 * chain's W_c: the same device functions run.
 * LENV_ERR_INVALID: a NULL action / state / elapsed / obs / reward / done, theta NULL for a type other than 0, rn NULL for types 1-8,
 * chains < 0, repeat < 1, eps without worker / sign, state_dim that is not the env's, an info type on an env without an info vector (the
 * reference's ValueError) or with an info_dim that is not the stand-in's.  LENV_ERR_UNSUPPORTED: an unknown type or env_id, a net outside
 * the shapes above, repeat > 64, chains >= 2^31.  chains == 0 returns LENV_OK after the pointer checks and before the descriptor is looked
 * at, like lenv_se_step_population.
 */
int lenv_rn_step_population(int32_t env_id, int32_t max_steps, int32_t type, const lenv_mlp_desc *rn /*HOST, types 1-8*/,
                            int32_t state_dim, int32_t info_dim, double gamma,
                            const float *theta, const float *eps, const int32_t *worker, const float *sign,
                            int64_t chains, int32_t repeat, const void *action /* int32 [chains] | float [chains,A] */,
                            double *state, int32_t *elapsed, float *obs, float *reward, float *done, void *stream);

/*
 * BaseAgent.test (agents/base_agent.py:155-227) of a population of trained DDQN / DuelingDDQN agents in one launch, as a call of its own:
 * agent i runs T = cfg->test_episodes greedy episodes (DDQN.select_test_action / DuelingDDQN.select_test_action, ties towards the lower
 * index) on the real env cfg->env_id (CartPole-v0, Acrobot-v1, MountainCar-v0).  The operations are those of the fused loops' closing test:
 * the action same_action_num times or until done, TimeLimit at max_steps env steps, each agent step's reward the fp64 sum of its repeats
 * rounded once to fp32 and added onto an fp32 episode return -- so on the final_online rows of a fused launch, with that launch's keys and
 * episode_offset = the test episodes it ran before its closing test, `returns` are that launch's final_returns bit for bit.
 * params [agents, P]: rows in the layout of lenv_dueling_se_inner_loop's final_online for the same cfg, P = lenv_dueling_num_params(cfg)
 * (agent_kind 0: the Critic_DQN state dict, which is also the register-resident kernel's final_online; agent_kind 1: feature_stream |
 * value_stream | advantage_stream; the shared LayerNorm's weight | bias behind the second Linear).  Episode e of agent i resets from the
 * counter draw (rng_keys[i], test-reset stream, episode_offset[i] + e) -- episode_offset NULL = 0 -- or, when reset_states [agents, T, 4] is
 * given, from reset_states[i][e] (the fp64 state words of lenv_real_env_reset).
 * Outputs: returns [agents, T] fp64 (the fp32 episode returns), env_steps [agents, T] env steps taken, agent_steps [agents, T] actions
 * chosen (what BaseAgent.test appends to episode_length_list, base_agent.py:213).  The row arrays -- all five or none -- receive the
 * transitions, the third value BaseAgent.test returns: agent step n of episode e of agent i in slot [i][e][n] of
 * row_state / row_next_state [agents, T, cap, state_dim], row_action (int32) / row_reward / row_done [agents, T, cap],
 * cap = lenv_agent_test_rows_cap(cfg): the observation acted on, the action, the observation after the last repeat, the fp32 reward, the
 * done flag with TimeLimit included.  Slots at or beyond agent_steps[i][e] are not written.
 * Of cfg only env_id, state_dim, num_actions, max_steps, q_hidden, q_layers, q_act, q_prelu, agent_kind, feature_dim, q_layer_norm,
 * test_episodes and same_action_num are read.  Admitted: the generic kernel's envelope -- q_layers 1..3, q_hidden 1..512, feature_dim 1..128
 * (agent_kind 1), test_episodes 1..128, same_action_num 0..64, q_act other than PReLU, (env_id, state_dim, num_actions) one of the three
 * envs; anything else LENV_ERR_UNSUPPORTED.  LENV_ERR_INVALID: agents < 0, a NULL cfg / params / rng_keys / returns / env_steps /
 * agent_steps, row arrays given in part, agent_kind other than 0 / 1, max_steps < 1.  agents == 0: LENV_OK after these checks.  No workspace.
 */
/* HOST: rows one test episode can produce = ceil(max_steps / max(same_action_num, 1)); negative LENV_ERR_* as the launch would return */
int64_t lenv_agent_test_rows_cap(const lenv_ddqn_cfg *cfg);
int lenv_agent_test_population(const lenv_ddqn_cfg *cfg /*HOST*/, const float *params /*[agents, P]*/,
                               const uint64_t *rng_keys /*[agents]*/, const int64_t *episode_offset /*[agents] or NULL = 0*/,
                               const double *reset_states /*[agents, T, 4] or NULL*/, int64_t agents,
                               double *returns /*[agents, T]*/, int32_t *env_steps /*[agents, T]*/, int32_t *agent_steps /*[agents, T]*/,
                               float *row_state /*[agents, T, cap, S]*/, int32_t *row_action /*[agents, T, cap]*/, float *row_next_state,
                               float *row_reward /*[agents, T, cap]*/, float *row_done, void *stream);

/*
 * BaseAgent.test of a population of trained TD3 / PPO agents in one launch, as a call of its own: the continuous-control half of
 * lenv_agent_test_population.  kind = LENV_ACTOR_TD3 (cfg is a lenv_td3_cfg; agents "td3" and "td3_vary" with vary_hp off) or LENV_ACTOR_PPO
 * (cfg is a lenv_ppo_cfg); any other kind is LENV_ERR_UNSUPPORTED -- TD3_discrete_vary (a Gumbel-softmax actor with an annealed temperature)
 * and the gridworld agents have none.  Agent i runs T = cfg->test_episodes episodes on the real env cfg->env_id (the HalfCheetah-v3 stand-in,
 * Pendulum-v0, MountainCarContinuous-v0) with the operations of the fused loops' closing test:
 *   TD3 (TD3.select_test_action): a = clamp(max_action * tanh(actor(s)) + (z * (float)action_std) * max_action, +-max_action),
 *       z = normal(rng_keys[i], TD3 test-noise stream, ((episode_offset[i] + e) * max_steps + agent_step) * A + k);
 *   PPO (actor_old.forward): a = tanh(net(s)) + z * max(action_std, 0.001f), action_std = the first A words of the row (a final_params row
 *       carries the trained, unclamped parameter: actor_old's copy differs from it by this clamp alone),
 *       z = normal(rng_keys[i], PPO test-noise stream, ((episode_offset[i] + e) * cap + agent_step) * A + k);
 * the action same_action_num times or until done, TimeLimit at max_steps env steps, each agent step's reward the fp64 sum of its repeats
 * rounded once to fp32 and added onto an fp32 episode return -- so on the final_params rows of a fused counter-mode launch, with that launch's
 * keys and episode_offset = the test episodes it ran before its closing test, `returns` are that launch's final_returns bit for bit.
 * params [agents, P]: rows in the layout of the fused loops' final_params for the same cfg.  TD3: actor | critic_1 | critic_2,
 * P = lenv_td3_num_params, only the actor is read.  PPO: action_std [A] | actor.net | critic.net, P = lenv_ppo_num_params.  One shape per
 * launch: a caller groups the agents of a *_vary population by drawn shape.
 * Episode e of agent i resets from the counter draw (rng_keys[i], test-reset stream, episode_offset[i] + e) -- episode_offset NULL = 0 -- or,
 * when reset_states [agents, T, SD] is given, from reset_states[i][e] (the fp64 state words of lenv_cont_env_reset: SD = 17 / 2 / 2).  noise
 * [agents, T, cap, A] (may be NULL): z of agent step n of episode e is noise[i][e][n][k] and the keys' noise streams are not drawn.
 * Outputs as lenv_agent_test_population: returns [agents, T] fp64 (the fp32 episode returns), env_steps / agent_steps [agents, T]; the row
 * arrays -- all five or none -- row_state / row_next_state [agents, T, cap, state_dim], row_action [agents, T, cap, action_dim] fp32,
 * row_reward / row_done [agents, T, cap], cap = lenv_actor_test_rows_cap(kind, cfg).  Slots at or beyond agent_steps[i][e] are not written.
 * Of cfg only env_id, state_dim, action_dim, max_steps, test_episodes, same_action_num, hidden, layers, act and -- TD3 -- use_layer_norm,
 * action_std, max_action are read.  Admitted: what the fused entry of the same kind admits for its actor and its test -- TD3: layers 1..3,
 * hidden 1..512, test_episodes * state_dim <= 512; PPO: layers 1..2, hidden 1..128, test_episodes 1..64; same_action_num 0..64, act other
 * than PReLU, (env_id, state_dim, action_dim) one of the three envs; anything else LENV_ERR_UNSUPPORTED.  LENV_ERR_INVALID: agents < 0, a NULL
 * cfg / params / rng_keys / returns / env_steps / agent_steps, row arrays given in part, max_steps < 1.  agents == 0: LENV_OK after these
 * checks.  No workspace.
 */
enum { LENV_ACTOR_TD3 = 0, LENV_ACTOR_PPO = 1 };
/* HOST: rows one test episode can produce = ceil(max_steps / max(same_action_num, 1)); negative LENV_ERR_* as the launch would return */
int64_t lenv_actor_test_rows_cap(int kind, const void *cfg /*HOST: lenv_td3_cfg / lenv_ppo_cfg*/);
int lenv_actor_test_population(int kind, const void *cfg /*HOST*/, const float *params /*[agents, P]*/,
                               const uint64_t *rng_keys /*[agents]*/, const int64_t *episode_offset /*[agents] or NULL = 0*/,
                               const double *reset_states /*[agents, T, SD] or NULL*/, const float *noise /*[agents, T, cap, A] or NULL*/,
                               int64_t agents, double *returns /*[agents, T]*/, int32_t *env_steps /*[agents, T]*/,
                               int32_t *agent_steps /*[agents, T]*/, float *row_state /*[agents, T, cap, S]*/,
                               float *row_action /*[agents, T, cap, A]*/, float *row_next_state, float *row_reward /*[agents, T, cap]*/,
                               float *row_done, void *stream);

/*
 * BaseAgent.test of a population of trained TD3_discrete_vary agents (Gumbel-softmax actors) in one launch, as a call of its own: the
 * discrete-action sibling of lenv_actor_test_population.  Agent i runs T = cfg->test_episodes episodes on the real env cfg->env_id
 * (CartPole-v0, Acrobot-v1, MountainCar-v0) with the operations of the closing test of lenv_td3d_inner_loop / lenv_td3d_rn_inner_loop
 * (TD3_discrete_vary.select_test_action, agents/TD3_discrete_vary.py:169-171; base_agent.py:155-227 with discretize_action):
 *   a = gumbel_softmax(actor(s) * max_action + g, temp, gumbel_hard) + z * (float)action_std      the action VECTOR the row keeps,
 *   the env gets the first maximum of a; n = ((episode_offset[i] + e) * max_steps + step) * A + k,
 *   g = gumbel(rng_keys[i], Gumbel test stream, n), z = normal(rng_keys[i], TD3 test-noise stream, n),
 *   temp = np.linspace(gumbel_temp, gumbel_temp / 20, 2000)[min(max(learn_calls[i] - 1, 0), 1999)] in fp32: the fused loop reads the
 *   temperature before it counts a learn call, so after L calls it holds the value of index L - 1 (with none: index 0).  learn_calls
 *   [agents] (NULL = 0) is column 2 of a fused launch's stats.
 * Each step's reward is rounded to fp32 onto an fp32 episode return; the episode ends at the env's done or after max_steps steps
 * (TimeLimit) -- so on the final_params rows of a fused counter-mode launch, with that launch's keys, learn_calls = its learn steps and
 * episode_offset = the test episodes it ran before its closing test, `returns` are that launch's final_returns bit for bit.
 * params [agents, P]: actor | critic_1 | critic_2, P = lenv_td3d_num_params(cfg); only the actor is read.  One shape per launch.
 * Episode e of agent i resets from the counter draw (rng_keys[i], test-reset stream, episode_offset[i] + e) -- episode_offset NULL = 0 -- or,
 * when reset_states [agents, T, 4] is given, from reset_states[i][e] (the fp64 state words of lenv_real_env_reset).  gumbel / noise
 * [agents, T, cap, A] (each may be NULL, each may be given without the other): g / z of step n of episode e is tape[i][e][n][k] and that
 * stream is not drawn.
 * Outputs as lenv_actor_test_population: returns [agents, T] fp64 (the fp32 episode returns), env_steps = agent_steps [agents, T] (one env
 * step per action); the row arrays -- all five or none -- row_state / row_next_state [agents, T, cap, state_dim], row_action
 * [agents, T, cap, action_dim] fp32, row_reward / row_done [agents, T, cap] (done with TimeLimit included), cap =
 * lenv_td3d_test_rows_cap(cfg) = max_steps.  Slots at or beyond agent_steps[i][e] are not written.
 * Of cfg only env_id, state_dim, action_dim, max_steps, test_episodes, hidden, layers, act, use_layer_norm, gumbel_hard, gumbel_temp,
 * action_std and max_action are read.  Admitted: what lenv_td3d_inner_loop admits for its actor and its test -- layers 1..3, hidden 1..512,
 * test_episodes 1..64, gumbel_temp > 0, act other than PReLU, (env_id, state_dim, action_dim) one of the three envs; anything else
 * LENV_ERR_UNSUPPORTED.  LENV_ERR_INVALID: agents < 0, a NULL cfg / params / rng_keys / returns / env_steps / agent_steps, row arrays given
 * in part, max_steps < 1.  agents == 0: LENV_OK after these checks.  No workspace.
 */
/* HOST: rows one test episode can produce = max_steps; negative LENV_ERR_* as the launch would return */
int64_t lenv_td3d_test_rows_cap(const lenv_td3d_cfg *cfg);
int lenv_td3d_test_population(const lenv_td3d_cfg *cfg /*HOST*/, const float *params /*[agents, P]*/,
                              const uint64_t *rng_keys /*[agents]*/, const int64_t *episode_offset /*[agents] or NULL = 0*/,
                              const int64_t *learn_calls /*[agents] or NULL = 0*/, const double *reset_states /*[agents, T, 4] or NULL*/,
                              const float *gumbel /*[agents, T, cap, A] or NULL*/, const float *noise /*[agents, T, cap, A] or NULL*/,
                              int64_t agents, double *returns /*[agents, T]*/, int32_t *env_steps /*[agents, T]*/,
                              int32_t *agent_steps /*[agents, T]*/, float *row_state /*[agents, T, cap, S]*/,
                              float *row_action /*[agents, T, cap, A]*/, float *row_next_state, float *row_reward /*[agents, T, cap]*/,
                              float *row_done, void *stream);

/*
 * BaseAgent.test of a population of trained tabular agents (QL, SARSA and their count-based variants: one select_test_action) in one
 * launch, as a call of its own.  Agent i, Q-table q_table[i] (fp64 [n_states * n_actions], the q_table output of lenv_ql_rn_inner_loop /
 * lenv_ql_se_inner_loop), runs T = cfg->test_episodes greedy episodes on the grid MDP given as the transition tables
 * next_state / reward / done [n_states, n_actions] (shared by all agents) with the operations of the fused loops' closing test: start at
 * start_state, the first maximum of the fp32-cast Q row, the action same_action_num times or until done, TimeLimit at max_steps env steps
 * (envs/env_factory.py:65-89 wraps every gridworld), each agent step's reward the fp64 sum of its repeats rounded once to fp32 and added
 * onto an fp32 episode return -- so on the q_table rows of a fused launch `returns` are that launch's final_returns bit for bit.
 * Outputs as lenv_agent_test_population: returns [agents, T] fp64, env_steps / agent_steps [agents, T]; the row arrays -- all five or none --
 * row_state / row_action / row_next_state (int32 state and action indices), row_reward / row_done (fp32) [agents, T, cap], cap =
 * lenv_ql_test_rows_cap(cfg); row_done has TimeLimit included.  Slots at or beyond agent_steps[i][e] are not written.
 * Of cfg only n_states, n_actions, start_state, max_steps, test_episodes and same_action_num are read.  Admitted: n_actions 1..8,
 * test_episodes 1..128, same_action_num 0..64, start_state inside 0..n_states-1; anything else LENV_ERR_UNSUPPORTED.  LENV_ERR_INVALID:
 * agents < 0, a NULL cfg / q_table / table / returns / env_steps / agent_steps, row arrays given in part, max_steps < 1.  agents == 0:
 * LENV_OK after these checks.  One thread per (agent, episode); no workspace.
 */
/* HOST: rows one test episode can produce = ceil(max_steps / max(same_action_num, 1)); negative LENV_ERR_* as the launch would return */
int64_t lenv_ql_test_rows_cap(const lenv_ql_cfg *cfg);
int lenv_ql_test_population(const lenv_ql_cfg *cfg /*HOST*/, const double *q_table /*[agents, n_states * n_actions]*/,
                            const int32_t *next_state, const double *reward, const uint8_t *done /*[n_states, n_actions], shared*/,
                            int64_t agents, double *returns /*[agents, T]*/, int32_t *env_steps /*[agents, T]*/,
                            int32_t *agent_steps /*[agents, T]*/, int32_t *row_state /*[agents, T, cap]*/, int32_t *row_action,
                            int32_t *row_next_state, float *row_reward, float *row_done, void *stream);

/* HalfCheetah-v3 STAND-IN reset / step for n instances (state [n,17] float64, action [n,6], obs [n,17]); same contract as
 * lenv_real_env_reset / lenv_real_env_step. */
int lenv_cheetah_standin_reset(const uint64_t *keys, const int64_t *episode, int64_t n, double *state, float *obs,
                               int32_t *elapsed, void *stream);
int lenv_cheetah_standin_step(int32_t max_steps, int64_t n, const float *action, double *state, int32_t *elapsed,
                              float *obs, float *reward, float *done, void *stream);

/* The continuous real envs of the TD3 path by id (LENV_ENV_CHEETAH_STANDIN: state [n,17], action [n,6], obs [n,17];
 * LENV_ENV_PENDULUM = gym 0.17.3 Pendulum-v0: state [n,2] = (theta, theta_dot), action [n,1], obs [n,3]; LENV_ENV_CMC =
 * MountainCarContinuous-v0: state [n,2] = (position, velocity), action [n,1], obs [n,2], done at the flag); replaces
 * gym.make(...).reset / .step + TimeLimit behind EnvWrapper (envs/env_wrapper.py:58-75).  Other ids: LENV_ERR_UNSUPPORTED. */
int lenv_cont_env_reset(int32_t env_id, const uint64_t *keys, const int64_t *episode, int64_t n, double *state, float *obs,
                        int32_t *elapsed, void *stream);
int lenv_cont_env_step(int32_t env_id, int32_t max_steps, int64_t n, const float *action, double *state, int32_t *elapsed,
                       float *obs, float *reward, float *done, void *stream);

/*
 * Supervised fit of `models` VirtualEnvs on recorded transitions: the "Supervised Learning / MBRL Baseline" of the reference's README, whose
 * experiments/syn_env_evaluate_cartpole_mbrl_baseline.py leaves fit_mbrl_baseline() unimplemented.  The three descs are the state, reward and
 * done net of a VirtualEnv (envs/virtual_env.py:16-33); theta [models, P] holds their parameters in the SE layout state | reward | done
 * (P = lenv_se_fit_num_params), adam_m / adam_v [models, P] the moments; all three are read and written.  x [N, in_dim] are the nets' inputs
 * cat(action, state), y_state [N, S], y_reward [N], y_done [N] the targets.
 *
 * Model m takes the Adam steps step_begin .. step_end-1 (torch.optim.Adam's single-tensor step, torch defaults for what is not an argument;
 * beta^t by repeated multiplication in double from step 0, so a fit cut into consecutive calls that hand theta and the moments on is the fit
 * in one call) on loss_k = F.mse_loss(net_k(x_b), y_k_b), one loss per net: the nets share no parameter, so this is one Adam over their sum.
 * Step t uses `batch` rows drawn with replacement: batch_idx [models, step_end-step_begin, batch] where given (tape mode; an index outside
 * [0, N) reads the nearest row), else row u64_to_below(rng_u64(rng_keys[m], 15, t * batch + j), N) for j < batch (counter mode).  Exactly one
 * of rng_keys / batch_idx is given.  loss [models, step_end-step_begin, 3] (may be NULL) receives the three means BEFORE the step.
 *
 * Arithmetic order (restated on the CPU by tests/se_fit_ref.c, which the kernel equals bit for bit): the forward is lenv_mlp_forward's, so a
 * fitted model steps exactly as lenv_mlp_forward / lenv_se_step_population compute it; the squared errors are summed by an fmaf chain over
 * rows ascending and outputs ascending inside a row, then divided by (float)(batch * out_dim); dL/dy = (float)(2.0 / (double)(batch * out_dim))
 * * e; every weight and bias gradient is a chain over the minibatch rows in ascending order.
 *
 * Shapes: equal in_dim (1..32), hidden (1..128), layers (1..2) and act (identity, relu, leakyrelu, tanh) on the three descs, state out_dim
 * 1..32, reward and done out_dim 1, batch 1..256; LENV_ERR_UNSUPPORTED beyond that: PReLU (torch would train the slope, theta has no place
 * for it), use_layer_norm, three hidden layers, models or N >= 2^31.  One workgroup per (model, net); a net's parameters, moments and
 * gradient stay in LDS where they fit behind the minibatch activations (lenv_se_fit_lds_bytes), else the gradient lives in the workspace
 * (lenv_se_fit_workspace_bytes, 0 for a launch that needs none; `workspace` may then be NULL): the bits are the same on either path.
 * LENV_ERR_INVALID: a NULL desc, a NULL data array with N > 0, N < 1 with step_end > step_begin, step_begin < 0, step_end < step_begin,
 * models < 0, a NULL theta / adam_m / adam_v with models > 0, both or neither of rng_keys / batch_idx.  LENV_ERR_WORKSPACE: a workspace
 * smaller than the query's.  models == 0 or step_end == step_begin: LENV_OK after these checks, without a launch.
 */
int64_t lenv_se_fit_num_params(const lenv_mlp_desc *state_net /*HOST*/, const lenv_mlp_desc *reward_net /*HOST*/, const lenv_mlp_desc *done_net /*HOST*/);
int64_t lenv_se_fit_lds_bytes(const lenv_mlp_desc *state_net /*HOST*/, const lenv_mlp_desc *reward_net /*HOST*/, const lenv_mlp_desc *done_net /*HOST*/,
                              int32_t batch);
int64_t lenv_se_fit_workspace_bytes(const lenv_mlp_desc *state_net /*HOST*/, const lenv_mlp_desc *reward_net /*HOST*/,
                                    const lenv_mlp_desc *done_net /*HOST*/, int32_t batch, int64_t models);
int lenv_se_fit_population(const lenv_mlp_desc *state_net /*HOST*/, const lenv_mlp_desc *reward_net /*HOST*/, const lenv_mlp_desc *done_net /*HOST*/,
                           const float *x, const float *y_state, const float *y_reward, const float *y_done, int64_t N, int32_t batch,
                           int64_t step_begin, int64_t step_end, double lr, double beta1, double beta2, double adam_eps,
                           const uint64_t *rng_keys, const int32_t *batch_idx, int64_t models, float *theta, float *adam_m, float *adam_v,
                           float *loss, void *workspace, size_t workspace_bytes, void *stream);

/* Counter-RNG key of a chain (same function as the oracle's): kind 0 = theta, 1 = theta+eps, 2 = theta-eps. HOST. */
/* out[c][i] = (2u - 1) * bounds[i], u = unit(rng(rng_keys[c], rng_stream, i)), i < p: freshly initialised parameter vectors
 * (nn.Linear default init with bounds[i] = 1/sqrt(fan_in)) keyed by the chains' counter-RNG keys.  rng_stream 10 reproduces
 * lenv_nes_draw's agent_init; ICM modules (lenv_dueling_se_inner_loop_icm) are drawn from stream 12. */
int lenv_chain_uniform_init(const uint64_t *rng_keys, int64_t chains, uint32_t rng_stream, int64_t p, const float *bounds, float *out,
                            void *stream);
/* one uniform in [0,1) of a chain's counter RNG (HOST function, no device work): unit(rng(key, stream, index)) */
double lenv_rng_unit(uint64_t key, uint32_t stream, uint64_t index);
uint64_t lenv_chain_key(uint64_t seed, uint64_t generation, uint64_t worker, uint64_t kind);

/*
 * GTN_Worker.calc_best_score (agents/GTN_worker.py:234-254) for `pop` workers from the per-chain scores
 * laid out [pop,3] = (orig, add, sub): result[p] = {score_best, score_orig, sign, 0} (double).
 */
int lenv_nes_worker_best(const double *chain_scores, int64_t pop, int32_t mirrored, double *result, void *stream);
/* the same for num_grad_evals = G evaluations per direction (agents/GTN_worker.py:90-104,234-242): chain_scores [pop,1+2G] =
 * (orig, add_1..add_G, sub_1..sub_G); grad_eval_type 0 = 'mean' (statistics.mean: the exactly rounded mean), 1 = 'minmax'
 * (min of both lists, as the reference computes it); anything else LENV_ERR_UNSUPPORTED. */
int lenv_nes_worker_best_multi(const double *chain_scores, int64_t pop, int32_t num_grad_evals, int32_t mirrored,
                               int32_t grad_eval_type, double *result, void *stream);

/*
 * One NES generation's stochastic inputs in a single launch, all from the counter RNG (reproduced by every rank and by the
 * CPU oracle): eps [pop, p_theta] = N(0,1) * noise_std (GTN_Worker.get_random_noise, agents/GTN_worker.py:156-163);
 * agent_init [chains, p_agent] = U(-bound_i, bound_i) (the nn.Linear default init of the fresh agent every calc_score builds,
 * agents/agent_utils.py:15-66); rng_keys [chains] = lenv_chain_key(seed, generation, worker_lo + c / chains_per_worker,
 * c % chains_per_worker).  Any of the three outputs may be NULL.
 */
int lenv_nes_draw(uint64_t seed, uint64_t generation, int64_t pop, int64_t p_theta, float noise_std, float *eps,
                  int64_t chains, int32_t chains_per_worker, int64_t worker_lo, int64_t p_agent, const float *bounds,
                  float *agent_init, uint64_t *rng_keys, void *stream);

/* The same with the generation read from device memory (generation_dev[0]) when the kernel runs: a captured generation
 * (HIP graph) is replayed for generation after generation without touching its kernel arguments; lenv_nes_rank_update_keep
 * advances the counter. */
int lenv_nes_draw_dev(uint64_t seed, const int64_t *generation_dev, int64_t pop, int64_t p_theta, float noise_std, float *eps,
                      int64_t chains, int32_t chains_per_worker, int64_t worker_lo, int64_t p_agent, const float *bounds,
                      float *agent_init, uint64_t *rng_keys, void *stream);

/* result[w][3] = min(status[0..n)) for w < pop: this rank's worst chain status rides in the fitness records through the
 * all-gather (replaces the second host read-back of a generation). */
int lenv_nes_status_fold(const int32_t *status, int64_t n, double *result, int64_t pop, void *stream);

/*
 * GTN_Master.score_transform + update_env (agents/GTN_master.py:197-298) on device.
 * gathered [pop,4] as produced by lenv_nes_worker_best (after the all-gather); rank_table [pop] doubles =
 * weight by rank for the rank-only transforms 1,2,3 (host-computed with the reference's numpy formulas);
 * weights_out [pop] receives score_transform_list; theta [P] is updated in place:
 * theta <- theta*(1-wd); for i in worker order: theta += (ss*w_i) * (sign_i*eps_i).
 */
int lenv_nes_rank_update(int32_t score_transform_type, const double *gathered, const double *rank_table, int64_t pop,
                         float *theta, const float *eps, int64_t p_theta, double step_size, int32_t nes_step_size,
                         double weight_decay, double *weights_out, void *stream);

/* lenv_nes_rank_update for a generation that runs as ONE captured graph (draw -> fused inner loop -> worker_best -> status_fold
 * -> rank update) with the host read-back behind it: theta_prev [P] (may be NULL) receives theta as it was before the update --
 * what GTN_Master.save_good_model saves and what stays when the run quits on "solved" (agents/GTN_master.py:95-101,118-131:
 * the reference decides both BEFORE update_env) -- and generation_dev[0] (may be NULL) is incremented for the next replay. */
int lenv_nes_rank_update_keep(int32_t score_transform_type, const double *gathered, const double *rank_table, int64_t pop,
                              float *theta, const float *eps, int64_t p_theta, double step_size, int32_t nes_step_size,
                              double weight_decay, double *weights_out, float *theta_prev, int64_t *generation_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif
